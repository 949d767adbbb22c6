"""
Model.transmission_channels measurements: the time of one tbk_transmission_channels_from_matrices call over
that of tbk_transmission_ensemble_from_matrices on the same input, in the same run, best of --reps after a warm-up -- what the
closing (two Cholesky factors, two products, the Jacobi and the sort per sample) costs on top of the decimation and the sweep.

The layers are those of tools/transport_model.py's random crystals with N = 16, 32, 64 rows, 64 in-plane points at 16 energies of
the line Im z = 0.05; the devices M = 1 and 32 layers of on-site energies uniform in [-0.5, 0.5), S = 1 and 64 samples.  Both calls
stage the same arrays and differ in the kernel and in N doubles per sample on the way back.

    OMP_NUM_THREADS=16 python tools/bench_channels.py [--reps 3] [--quick]
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
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    best = float("inf")
    for _ in range(reps):
        start = time.perf_counter()
        call()
        best = min(best, time.perf_counter() - start)
    return best


def one(N, M, S, n_k, n_z, reps):
    _, H00, H01 = tm.random_case(N, 1, n_k, 7000 + N)
    H00, H01 = np.ascontiguousarray(H00), np.ascontiguousarray(H01)
    onsite = np.random.default_rng(7100 + N + M).uniform(-0.5, 0.5, (S, M, N))
    z = np.ascontiguousarray(np.linspace(-2.5, 2.5, n_z) + 0.05j)
    T = np.empty((n_k, n_z, S))
    T2 = np.empty_like(T)
    channels = np.empty((n_k, n_z, S, N))
    its = np.empty((n_k, n_z), dtype=np.int32)
    lib = _lib.lib()

    def ensemble():
        _lib.check(lib.tbk_transmission_ensemble_from_matrices(0, N, n_k, _lib.ptr(H00), _lib.ptr(H01), M, S, None, _lib.ptr(onsite), n_z, _lib.ptr(z), 64,
                                                               0, 0, _lib.ptr(its), _lib.ptr(T)))

    def with_channels():
        _lib.check(lib.tbk_transmission_channels_from_matrices(0, N, n_k, _lib.ptr(H00), _lib.ptr(H01), M, S, None, _lib.ptr(onsite), n_z, _lib.ptr(z), 64,
                                                               0, 0, _lib.ptr(its), _lib.ptr(T2), _lib.ptr(channels)))

    ensemble()
    with_channels()
    t_e = _best(ensemble, reps)
    t_c = _best(with_channels, reps)
    same = np.array_equal(T, T2)
    gap = float(np.abs(channels.sum(axis=-1) - T).max())
    print("  N = %2d  M = %2d  S = %2d  iterations %2d ... %2d:  ensemble %9.3f ms   channels %9.3f ms   ratio %5.2f   T bits %s   max|sum T_n - T| = %.1e"
          % (N, M, S, its.min(), its.max(), 1e3 * t_e, 1e3 * t_c, t_c / t_e, "equal" if same else "DIFFER", gap), flush=True)
    return t_c / t_e


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=3)
    parser.add_argument("--quick", action="store_true", help="16 points at 4 energies")
    args = parser.parse_args()
    n_k, n_z = (16, 4) if args.quick else (64, 16)
    print("tbk_transmission_channels_from_matrices over tbk_transmission_ensemble_from_matrices: %d points, %d energies, best of %d" % (n_k, n_z, args.reps))
    for N in (16, 32, 64):
        for M in (1, 32):
            for S in (1, 64):
                one(N, M, S, n_k, n_z, args.reps)


if __name__ == "__main__":
    main()
