"""
Model.transmission_ensemble measurements: prints two tables.  One ensemble call against the loop of S
Model.transmission calls on the same devices in the same run -- the only route there was before -- best of --reps after a warm-up.

1. The models of tools/bench_transport.py -- 16 orbitals, hoppings that reach L = 1, 2, 4 cells along the stacking axis (N = 16, 32,
   64) -- with S = 64 devices of M = 8 layers of on-site energies uniform in [-0.5, 0.5), 64 in-plane points at 16 energies of the
   line Im z = 0.05: wall time and stages (tbk_transmission_ensemble_timing / tbk_transmission_timing summed over the loop), the
   kernel ratio against (iterations 56 + M 40) / (M 40), and whether the bits agree.
2. A one-dimensional wire (NK = 1) of N = 16, 32, 64 rows at 64 energies with S = 256 devices through
   tbk_transmission_ensemble_from_matrices: sample_chunk = S (one workgroup per energy, no split), sample_chunk = 0 (the groups fill
   the device) and the loop of tbk_transmission_from_matrices.

    OMP_NUM_THREADS=16 python tools/bench_ensemble.py [--reps 3] [--quick]
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
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position
from bench_surface import layered_model, _best  # noqa: E402  pylint: disable=wrong-import-position


def _stages(model, getter, call, reps):
    lib, handle = _lib.lib(), model._staged()  # pylint: disable=protected-access
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(getter(handle, ms, ctypes.byref(calls), 1))
    for _ in range(reps):
        call()
    _lib.check(getter(handle, ms, ctypes.byref(calls), 1))
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    return [x / reps for x in ms]  # per ensemble call, or per whole loop


def whole_calls(n, L, M, S, n_k, n_z, reps):
    model = layered_model(n, L, 4000 + L)
    N = n * L
    onsite = np.random.default_rng(4200 + L).uniform(-0.5, 0.5, (S, M, N))
    kpar = np.stack([np.linspace(0.0, 0.5, n_k), np.linspace(0.0, 0.25, n_k)], axis=1)
    z = np.linspace(-2.5, 2.5, n_z) + 0.05j
    ensemble = lambda: model.transmission_ensemble(kpar, z, onsite)  # noqa: E731
    loop = lambda: [model.transmission(kpar, z, device=onsite[s]) for s in range(S)]  # noqa: E731
    ensemble()
    wall_e, got = _best(ensemble, reps)
    loop()
    wall_l, singles = _best(loop, reps)
    st_e = _stages(model, _lib.lib().tbk_transmission_ensemble_timing, ensemble, reps)
    st_l = _stages(model, _lib.lib().tbk_transmission_timing, loop, reps)
    same = all(np.array_equal(singles[s].transmission, got.transmission[:, :, s]) for s in range(S))
    its = got.iterations
    predicted = (56.0 * its.mean() + 40.0 * M) / (40.0 * M)
    print("| %d | %d | %d | %d | %d x %d x %d | %.1f | %.2f | %.2f | %.2f | %.1f | %.2f | %.2f | %.2f | %.1f | %.2f | %.1f | %.2f | %s |"
          % (n, L, N, M, n_k, n_z, S, wall_e * 1e3, st_e[0], st_e[1], st_e[2], wall_l * 1e3, st_l[0], st_l[1], st_l[2], its.mean(), predicted,
             wall_l / wall_e, st_l[1] / st_e[1] if st_e[1] > 0 else float("nan"), "equal" if same else "DIFFERENT"))
    sys.stdout.flush()


def _from_matrices(H00, H01, onsite, z, sample_chunk):
    n_k, N = H00.shape[0], H00.shape[-1]
    T = np.empty((n_k, len(z), onsite.shape[0]))
    its = np.empty((n_k, len(z)), dtype=np.int32)
    _lib.check(_lib.lib().tbk_transmission_ensemble_from_matrices(0, N, n_k, _lib.ptr(H00), _lib.ptr(H01), onsite.shape[1], onsite.shape[0], None,
                                                                  _lib.ptr(onsite), len(z), _lib.ptr(z), 64, 0, sample_chunk, _lib.ptr(its), _lib.ptr(T)))
    return T, its


def _single(H00, H01, V, z):
    n_k, N = H00.shape[0], H00.shape[-1]
    T = np.empty((n_k, len(z)))
    its = np.empty((n_k, len(z)), dtype=np.int32)
    _lib.check(_lib.lib().tbk_transmission_from_matrices(0, N, n_k, _lib.ptr(H00), _lib.ptr(H01), V.shape[0], _lib.ptr(V), len(z), _lib.ptr(z), 64, 0,
                                                         _lib.ptr(its), _lib.ptr(T), None))
    return T


def wire(N, M, S, n_z, reps):
    _, H00, H01 = tm.random_case(N, 1, 1, 4300 + N)
    H00, H01 = np.ascontiguousarray(H00), np.ascontiguousarray(H01)
    onsite = np.random.default_rng(4400 + N).uniform(-0.5, 0.5, (S, M, N))
    z = np.ascontiguousarray(np.linspace(-2.5, 2.5, n_z) + 0.05j)
    dense = np.zeros((S, M, N, N), dtype=np.complex128)
    dense[:, :, np.arange(N), np.arange(N)] = onsite
    one = lambda: _from_matrices(H00, H01, onsite, z, S)  # noqa: E731
    split = lambda: _from_matrices(H00, H01, onsite, z, 0)  # noqa: E731
    loop = lambda: [_single(H00, H01, dense[s], z) for s in range(S)]  # noqa: E731
    one()
    t_one, (T_one, its) = _best(one, reps)
    split()
    t_split, (T_split, _) = _best(split, reps)
    loop()
    t_loop, singles = _best(loop, reps)
    same = np.array_equal(T_one, T_split) and all(np.array_equal(singles[s], T_split[:, :, s]) for s in range(S))
    print("| %d | %d | 1 x %d x %d | %.1f | %.2f | %.2f | %.2f | %.2f | %.1f | %s |"
          % (N, M, n_z, S, its.mean(), t_one * 1e3, t_split * 1e3, t_loop * 1e3, t_one / t_split, t_loop / t_split, "equal" if same else "DIFFERENT"))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="8 points x 4 energies x 8 samples, and 8 energies x 16 samples (a smoke run of the tool)")
    ap.add_argument("--layers", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--length", type=int, default=8, help="M, the principal layers of the device")
    args = ap.parse_args()
    print("library: %s" % _lib.LIB_PATH)
    n_k, n_z, S = (8, 4, 8) if args.quick else (64, 16, 64)
    print("| orbitals | L | N | M | points x energies x samples | ensemble call ms | its H(k) + layers ms | its decimation + sweeps ms | its output ms "
          "| loop of S transmission calls ms | its H(k) + layers ms | its decimation + sweep ms | its output ms | mean iterations "
          "| predicted kernel ratio (iterations 56 + M 40) / (M 40) | call ratio loop / ensemble | kernel ratio loop / ensemble | bits |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for L in args.layers:
        whole_calls(16, L, args.length, S, n_k, n_z, args.reps)
    n_z, S = (8, 16) if args.quick else (64, 256)
    print()
    print("| N | M | points x energies x samples | mean iterations | sample_chunk = S ms | sample_chunk = 0 ms | loop of S tbk_transmission_from_matrices ms "
          "| unsplit / split | loop / split | bits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for N in (16, 32, 64):
        wire(N, args.length, S, n_z, args.reps)


if __name__ == "__main__":
    t0 = time.perf_counter()
    main()
    print("total %.1f s" % (time.perf_counter() - t0))
