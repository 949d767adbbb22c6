"""
Model.device_green_function measurements: prints one table.

The models of tools/bench_transport.py -- 16 orbitals, hoppings that reach L = 1, 2, 4 cells along the stacking axis (principal layers
of N = 16, 32 and 64 rows) -- with its device of M = 8 layers of random Hermitian barriers of norm 0.5, on its path of 256 in-plane
points at 64 energies of the line Im z = 0.05, best of --reps after a warm-up:

1. wall time of the call and its stages per call (tbk_device_green_timing): H(k) with the principal layers, the decimation with both
   sweeps (one launch), the copies of the results to the host;
2. Model.transmission on the same inputs, wall and kernel: the difference of the kernels is the price of the stack and of the backward
   sweep;
3. 56 N^3 flops per iteration of the decimation plus (40 + 64) N^3 per layer over the kernel's time, as a fraction of
   tbk_mfma_f64_peak measured in the same run;
4. the host route there was before: Model.surface_green_function on the GPU (bottom and top as full matrices), then NumPy -- per (k, z)
   the self-energies as products and both sweeps with numpy.linalg.inv and @ -- on --baseline-points of the 256 points, scaled to all.

    OMP_NUM_THREADS=16 python tools/bench_device_green.py [--reps 3] [--quick]
"""

import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tbmodels_amd import _lib  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position
from bench_surface import layered_model, _best  # noqa: E402  pylint: disable=wrong-import-position


def host_route(model, kpar, z, L, V):
    """today's route without Model.device_green_function: the surface functions from the GPU, both sweeps in NumPy; (ldos, left, right)"""
    got = model.surface_green_function(kpar, z)
    pts = np.concatenate([sm.sample_points(kp, 2, L, 3) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    M, N = V.shape[0], V.shape[1]
    one = np.eye(N)
    out = np.empty((3, len(kpar), len(z), M, N))
    for k, samples in enumerate(ham):
        H00, H01 = sm.principal(sm.layers_from_samples(samples))
        H10 = H01.conj().T
        for i, zz in enumerate(z):
            sigma_r = H01 @ got.bottom[k, i] @ H10
            sigma_l = H10 @ got.top[k, i] @ H01
            gamma_r = 1j * (sigma_r - sigma_r.conj().T)
            gamma_l = 1j * (sigma_l - sigma_l.conj().T)
            D = H00 + sigma_l + V[0]
            g, hq = [], [None]
            P = None
            for p in range(M):
                if p == M - 1:
                    D = D + sigma_r
                g.append(np.linalg.inv(zz * one - D))
                if p > 0:
                    hq.append(H10 @ P)
                P = g[p] if p == 0 else g[p] @ hq[p]
                if p < M - 1:
                    D = H00 + V[p + 1] + H10 @ (g[p] @ H01)
            G = C = g[M - 1]
            for p in range(M - 1, -1, -1):
                if p < M - 1:
                    X = g[p] @ H01
                    G = g[p] + (X @ G) @ (H10 @ g[p])
                    C = X @ C
                F = P if p == M - 1 else G if p == 0 else G @ hq[p]
                out[0, k, i, p] = -np.diagonal(G).imag / np.pi
                out[1, k, i, p] = ((F @ gamma_l) * F.conj()).real.sum(axis=1) / (2 * np.pi)
                out[2, k, i, p] = ((C @ gamma_r) * C.conj()).real.sum(axis=1) / (2 * np.pi)
    return out


def _stages(model, getter, call, reps):
    lib, handle = _lib.lib(), model._staged()  # pylint: disable=protected-access
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(getter(handle, ms, ctypes.byref(calls), 1))
    for _ in range(reps):
        call()
    _lib.check(getter(handle, ms, ctypes.byref(calls), 1))
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    return [x / max(1, calls.value) for x in ms]


def measure(n, L, M, n_k, n_z, reps, baseline_points, peak_tflops):
    model = layered_model(n, L, 4000 + L)
    N = n * L
    V = tm.random_device(N, M, 4100 + L)
    kpar = np.stack([np.linspace(0.0, 0.5, n_k), np.linspace(0.0, 0.25, n_k)], axis=1)
    z = np.linspace(-2.5, 2.5, n_z) + 0.05j
    call = lambda: model.device_green_function(kpar, z, device=V)  # noqa: E731
    plain = lambda: model.transmission(kpar, z, device=V)  # noqa: E731
    call()  # warm-up
    plain()
    wall, result = _best(call, reps)
    wall_t, trans = _best(plain, reps)
    st = _stages(model, _lib.lib().tbk_device_green_timing, call, reps)
    st_t = _stages(model, _lib.lib().tbk_transmission_timing, plain, reps)
    assert np.array_equal(trans.transmission, result.transmission)
    its = result.iterations
    flops = N ** 3 * (56.0 * float(its.sum()) + 104.0 * M * its.size)
    share = flops / (st[1] * 1e-3) / (peak_tflops * 1e12) if st[1] > 0 else float("nan")
    pick = np.linspace(0, n_k - 1, baseline_points).astype(int)
    t0 = time.perf_counter()
    ref = host_route(model, kpar[pick], z, L, V)
    base = (time.perf_counter() - t0) * n_k / len(pick)
    diff = max(np.abs(ref[0] - result.ldos[pick]).max(), np.abs(ref[1] - result.left[pick]).max(), np.abs(ref[2] - result.right[pick]).max())
    print("| %d | %d | %d | %d | %d x %d | %.1f | %.2f | %.2f | %.2f | %.1f | %.2f | %.2f | %.1f | %.3f | %.0f | %.0f | %.1e | %.3f |"
          % (n, L, N, M, n_k, n_z, wall * 1e3, st[0], st[1], st[2], wall_t * 1e3, st_t[1], st[1] / st_t[1], its.mean(), share, base * 1e3, base / wall, diff,
             result.ldos.max()))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="16 points x 8 energies (a smoke run of the tool)")
    ap.add_argument("--layers", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--length", type=int, default=8, help="M, the principal layers of the device")
    ap.add_argument("--baseline-points", type=int, default=4)
    args = ap.parse_args()
    tf = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
    print("library: %s" % _lib.LIB_PATH)
    print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
    print("| orbitals | L | N | M | points x energies | call ms | H(k) + layers ms | decimation + sweeps ms | output ms | transmission call ms "
          "| transmission kernel ms | kernel / transmission kernel | mean iterations | kernel / MFMA peak (56 N^3 per iteration + 104 N^3 per layer) "
          "| surface_green_function + NumPy ms (scaled from %d points) | ratio | max|difference| | max ldos |" % args.baseline_points)
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    n_k, n_z = (16, 8) if args.quick else (256, 64)
    for L in args.layers:
        measure(16, L, args.length, n_k, n_z, args.reps, min(args.baseline_points, n_k), tf.value)


if __name__ == "__main__":
    main()
