"""
Model.device_current measurements: prints one table.

The models and the device of tools/bench_device_green.py -- 16 orbitals, hoppings that reach L = 1, 2, 4 cells along the stacking axis
(principal layers of N = 16, 32 and 64 rows), M = 8 layers of random Hermitian barriers of norm 0.5 -- on its path of 256 in-plane points
at 64 energies of the line Im z = 0.05, best of --reps after a warm-up:

1. wall time of the call and its stages per call (tbk_device_current_timing): H(k) with the principal layers, the decimation with both
   sweeps and the current steps (one launch), the copies of the results to the host;
2. Model.device_green_function on the same inputs, wall and kernel: the difference of the kernels is the price of the current steps;
3. the host route there was before: Model.device_green_function(green=True) on the GPU, then NumPy -- per (k, z) the broadenings from
   Model.surface_green_function, and per layer two products and an element pass for each lead -- on --baseline-points of the 256 points,
   scaled to all;
4. with --bonds the same call with bonds=True (K and J leave the GPU as well).

    OMP_NUM_THREADS=16 python tools/bench_device_current.py [--reps 3] [--quick] [--bonds]
"""

import argparse
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
from bench_device_green import _stages  # noqa: E402  pylint: disable=wrong-import-position


def host_route(model, kpar, z, L, V):
    """today's route without Model.device_current: F_p and C_p of device_green_function(green=True) and the surface functions from the
    GPU, the currents in NumPy; (current_left, current_right) and the seconds of the GPU calls alone"""
    t0 = time.perf_counter()
    got = model.device_green_function(kpar, z, device=V, green=True)
    lead = model.surface_green_function(kpar, z)
    on_gpu = time.perf_counter() - t0
    pts = np.concatenate([sm.sample_points(kp, 2, L, 3) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    M, N = V.shape[0], V.shape[1]
    out = np.empty((2, len(kpar), len(z), M - 1, N))
    for k, samples in enumerate(ham):
        _, H01 = sm.principal(sm.layers_from_samples(samples))
        H10 = H01.conj().T
        for i in range(len(z)):
            sigma_r = H01 @ lead.bottom[k, i] @ H10
            sigma_l = H10 @ lead.top[k, i] @ H01
            for side, (B, sigma) in enumerate(((got.first[k, i], sigma_l), (got.last[k, i], sigma_r))):
                gamma = 1j * (sigma - sigma.conj().T)
                A = np.einsum("pik,pjk->pij", B[:-1] @ gamma, B[1:].conj())
                out[side, k, i] = (2.0 * (H01.real * A.imag - H01.imag * A.real)).sum(axis=2)
    return out, on_gpu


def measure(n, L, M, n_k, n_z, reps, baseline_points, bonds):
    model = layered_model(n, L, 4000 + L)
    N = n * L
    V = tm.random_device(N, M, 4100 + L)
    kpar = np.stack([np.linspace(0.0, 0.5, n_k), np.linspace(0.0, 0.25, n_k)], axis=1)
    z = np.linspace(-2.5, 2.5, n_z) + 0.05j
    call = lambda: model.device_current(kpar, z, device=V, bonds=bonds)  # noqa: E731
    plain = lambda: model.device_green_function(kpar, z, device=V)  # noqa: E731
    call()  # warm-up
    plain()
    wall, result = _best(call, reps)
    wall_g, green = _best(plain, reps)
    st = _stages(model, _lib.lib().tbk_device_current_timing, call, reps)
    st_g = _stages(model, _lib.lib().tbk_device_green_timing, plain, reps)
    assert np.array_equal(green.ldos, result.ldos) and np.array_equal(green.transmission, result.transmission)
    added = st[1] - st_g[1]
    pick = np.linspace(0, n_k - 1, baseline_points).astype(int)
    t0 = time.perf_counter()
    ref, on_gpu = host_route(model, kpar[pick], z, L, V)
    base = (time.perf_counter() - t0) * n_k / len(pick)
    diff = max(np.abs(ref[0] - result.current_left[pick]).max(), np.abs(ref[1] - result.current_right[pick]).max())
    total = result.current_left.sum(axis=3)
    print("| %d | %d | %d | %d | %d x %d | %s | %.1f | %.2f | %.2f | %.2f | %.1f | %.2f | %.3f | %.3f | %.2f | %.0f | %.0f | %.0f | %.1e | %.2e |"
          % (n, L, N, M, n_k, n_z, "yes" if bonds else "no", wall * 1e3, st[0], st[1], st[2], wall_g * 1e3, st_g[1], st[1] / st_g[1], wall / wall_g, added,
             base * 1e3, on_gpu * n_k / len(pick) * 1e3, base / wall, diff, np.abs(total - result.transmission[..., None]).max()))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="16 points x 8 energies (a smoke run of the tool)")
    ap.add_argument("--layers", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--length", type=int, default=8, help="M, the principal layers of the device")
    ap.add_argument("--baseline-points", type=int, default=4)
    ap.add_argument("--bonds", action="store_true", help="bonds=True: K and J are formed and leave the GPU")
    args = ap.parse_args()
    print("library: %s" % _lib.LIB_PATH)
    print("| orbitals | L | N | M | points x energies | bonds | call ms | H(k) + layers ms | decimation + sweeps + currents ms | output ms "
          "| device_green_function call ms | device_green_function kernel ms | kernel / device_green_function's | call / device_green_function's "
          "| added kernel ms | device_green_function(green=True) + NumPy ms (scaled from %d points) | of which on the GPU ms | ratio "
          "| max|difference| | max|interface total - T| |" % args.baseline_points)
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    n_k, n_z = (16, 8) if args.quick else (256, 64)
    for L in args.layers:
        measure(16, L, args.length, n_k, n_z, args.reps, min(args.baseline_points, n_k), args.bonds)


if __name__ == "__main__":
    main()
