"""
Model.surface_green_function measurements: prints one table.

Synthetic 3-D models of 16 orbitals whose hoppings reach L = 1, 2, 4, 5 cells along the stacking axis (principal layers of N = 16, 32,
64 and 80 rows, the last on the library route) on a path of 256 in-plane points at 64 energies of the line Im z = 0.05,
spectral=True (what a surface spectral map asks for), best of --reps after a warm-up:

1. wall time of the call and its stages per call (tbk_surface_timing): H(k) with the principal layers, the decimation, the copies of
   the results to the host;
2. iterations per (k, z) and the decimation's 56 N^3 flops per iteration (the three closing inversions are not counted) over its time
   as a fraction of tbk_mfma_f64_peak measured in the same run;
3. the same call with the library route forced (TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER) and its decimation stage;
4. the route there was before: Model.hamilton at the 2 L + 1 samples per point, then NumPy -- the discrete Fourier sum, and per (k, z) a
   loop of numpy.linalg.inv and @ with the same stopping rule -- on --baseline-points of the 256 points, scaled to all of them.

    OMP_NUM_THREADS=16 python tools/bench_surface.py [--reps 3] [--quick]
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

import tbmodels_amd  # noqa: E402  pylint: disable=wrong-import-position
from tbmodels_amd import _lib  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position


def layered_model(n, L, seed):
    """n orbitals, random hoppings (0, 0, m), m = 0 ... L, and (1, 0, 0), (0, 1, 0), (1, 1, 1), scaled to a spectrum inside [-2, 2]"""
    rng = np.random.default_rng(seed)
    vectors = [(0, 0, m) for m in range(L + 1)] + [(1, 0, 0), (0, 1, 0), (1, 1, 1)]
    hop = rng.normal(size=(len(vectors), n, n)) + 1j * rng.normal(size=(len(vectors), n, n))
    hop[0] = (hop[0] + hop[0].conj().T) / 4
    r_vec = np.array(vectors)
    total = sum(np.linalg.norm(m, 2) for m in sm.full_hoppings(r_vec, hop).values())
    return tbmodels_amd.Model.from_packed(r_vec, hop * (2.0 / total), pos=np.zeros((n, 3)))


def numpy_route(model, kpar, z, L):
    """the parent's only route: hamilton, then NumPy; returns -Im diag / pi of the three functions"""
    pts = np.concatenate([sm.sample_points(kp, 2, L, 3) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    out = np.empty((3, len(kpar), len(z), model.size * L))
    for k, samples in enumerate(ham):
        H00, H01 = sm.principal(sm.layers_from_samples(samples))
        one = np.eye(H00.shape[0])
        threshold = sm.U_ROUND * sm.norm_inf(H01)
        for i, zz in enumerate(z):
            es, et, e = H00, H00, H00
            alpha, beta = H01, H01.conj().T
            while True:
                g = np.linalg.inv(zz * one - e)
                t = g @ alpha
                p2, a_new = beta @ t, alpha @ t
                t = g @ beta
                p3, b_new = alpha @ t, beta @ t
                et, es, e = et + p2, es + p3, e + p2 + p3
                alpha, beta = a_new, b_new
                if max(sm.norm_inf(alpha), sm.norm_inf(beta)) <= threshold:
                    break
            for j, m in enumerate((es, et, e)):
                out[j, k, i] = -np.diagonal(np.linalg.inv(zz * one - m)).imag / np.pi
    return out


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(n, L, n_k, n_z, reps, baseline_points, peak_tflops):
    model = layered_model(n, L, 4000 + L)
    N = n * L
    kpar = np.stack([np.linspace(0.0, 0.5, n_k), np.linspace(0.0, 0.25, n_k)], axis=1)
    z = np.linspace(-2.5, 2.5, n_z) + 0.05j
    call = lambda: model.surface_green_function(kpar, z, spectral=True)  # noqa: E731
    call()  # warm-up
    wall, result = _best(call, reps)
    lib, handle = _lib.lib(), model._staged()  # pylint: disable=protected-access
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_surface_timing(handle, ms, ctypes.byref(calls), 1))
    for _ in range(reps):
        call()
    _lib.check(lib.tbk_surface_timing(handle, ms, ctypes.byref(calls), 1))
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    st = [x / max(1, calls.value) for x in ms]
    its = result.iterations
    flops = 56.0 * N ** 3 * float(its.sum())
    share = flops / (st[1] * 1e-3) / (peak_tflops * 1e12) if st[1] > 0 else float("nan")
    # the library route on request (above 64 rows it is the route anyway)
    forced = layered_model(n, L, 4000 + L)
    forced.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    by_library = lambda: forced.surface_green_function(kpar, z, spectral=True)  # noqa: E731
    by_library()
    wall_lib, result_lib = _best(by_library, reps)
    handle_lib = forced._staged()  # pylint: disable=protected-access
    _lib.check(lib.tbk_model_set_option(handle_lib, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_surface_timing(handle_lib, ms, ctypes.byref(calls), 1))
    by_library()
    _lib.check(lib.tbk_surface_timing(handle_lib, ms, ctypes.byref(calls), 1))
    lib_ms = ms[1] / max(1, calls.value)
    diff_lib = max(np.abs(result_lib[4 + j] - result[4 + j]).max() for j in range(3))
    pick = np.linspace(0, n_k - 1, baseline_points).astype(int)
    t0 = time.perf_counter()
    ref = numpy_route(model, kpar[pick], z, L)
    base = (time.perf_counter() - t0) * n_k / len(pick)
    diff = max(np.abs(ref[j] - result[4 + j][pick]).max() for j in range(3))
    print("| %d | %d | %d | %s | %d x %d | %.1f | %.2f | %.2f | %.2f | %d ... %d (mean %.1f) | %.3f | %.1f | %.1f | %.1e | %.0f | %.0f | %.1e |"
          % (n, L, N, "library" if N > 64 else "own kernel", n_k, n_z, wall * 1e3, st[0], st[1], st[2], its.min(), its.max(), its.mean(), share,
             wall_lib * 1e3, lib_ms, diff_lib, base * 1e3, base / wall, diff))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="16 points x 8 energies (a smoke run of the tool)")
    ap.add_argument("--layers", type=int, nargs="*", default=[1, 2, 4, 5])
    ap.add_argument("--baseline-points", type=int, default=4)
    args = ap.parse_args()
    tf = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
    print("library: %s" % _lib.LIB_PATH)
    print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
    print("| orbitals | L | N | route | points x energies | call ms | H(k) + layers ms | decimation ms | output ms | iterations | decimation / MFMA peak "
          "(56 N^3 flops per iteration) | call, library route forced ms | its decimation ms | max|own - library| "
          "| hamilton + NumPy ms (scaled from %d points) | ratio | max|difference| |" % args.baseline_points)
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    n_k, n_z = (16, 8) if args.quick else (256, 64)
    for L in args.layers:
        measure(16, L, n_k, n_z, args.reps, min(args.baseline_points, n_k), tf.value)


if __name__ == "__main__":
    main()
