"""
Model.eigh measurements: prints one table.

1. The TBK_T_EIG stage per matrix, device-resident (tbk_eigh_device), for the own Jacobi kernel and for the rocSOLVER
   branch (the same handles with TBK_EIG_ROCSOLVER), at n in {8, 14, 32, 64} x nk in {1, 64, 4096, 65536}.  The matrices
   are H(k) of seeded dense models (synthetic.dense_model_arrays, 16 lattice vectors) at random k-points.
2. Whole calls: Model.eigh against Model.eigenval for the silicon model at one k-point (host buffers, the Z2Pack call
   shape), and for the 64-orbital / 4096-R headline model (bench.py cfg2) at 100 000 k-points, device-resident
   (tbk_eigh_device against tbk_eigenval_device).
3. Sweeps of the Jacobi iteration (a NumPy replay of the kernel's algorithm on a few of the same matrices: the kernel does
   not report them) and the executed-flop fraction of the FP64 vector peak: a sweep is n - 1 rounds of three passes (rows of
   A, columns of A, columns of V) over n / 2 pairs x NP elements, 20 flops per (pair, element) item of a pass.

    python tools/bench_eigh.py [--reps 5] [--quick]
"""

import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tbmodels_amd  # noqa: E402  pylint: disable=wrong-import-position
from tbmodels_amd import _lib, synthetic  # noqa: E402  pylint: disable=wrong-import-position

FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X, FP64 vector (AMD specification)


def _padded(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


def jacobi_sweeps(mat):
    """Sweeps the kernel's algorithm takes on `mat` (round-robin pairs on the padded size, relative skip criterion, stop
    after the first sweep that rotates nothing); NumPy replay of csrc/tbk_eigh.hip for the record."""
    n, NP = len(mat), _padded(len(mat))
    a = np.array(mat, dtype=complex)
    for sweep in range(1, 31):
        rotated = 0
        for r in range(NP - 1):
            pairs = []
            for k in range(NP // 2):
                x, y = (NP - 1, r) if k == 0 else ((r + k) % (NP - 1), (r - k + NP - 1) % (NP - 1))
                p, q = min(x, y), max(x, y)
                if q >= n:
                    continue
                app, aqq, apq = a[p, p].real, a[q, q].real, a[p, q]
                beta = abs(apq)
                if beta <= np.finfo(float).eps * np.sqrt(abs(app)) * np.sqrt(abs(aqq)):
                    continue
                zeta = (aqq - app) / (2 * beta)
                t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                pairs.append((p, q, c, t * c * apq / beta, app - t * beta, aqq + t * beta))
            for p, q, c, se, _, _ in pairs:
                u, v = a[p].copy(), a[q].copy()
                a[p], a[q] = c * u - se * v, np.conj(se) * u + c * v
            for p, q, c, se, dp, dq in pairs:
                u, v = a[:, p].copy(), a[:, q].copy()
                a[:, p], a[:, q] = c * u - np.conj(se) * v, se * u + c * v
                a[p, p], a[q, q], a[p, q], a[q, p] = dp, dq, 0, 0
            rotated += len(pairs)
        if rotated == 0:
            return sweep
    return 30


def _device_array(lib, nbytes):
    ptr = ctypes.c_void_p()
    _lib.check(lib.tbk_device_malloc(0, max(1, nbytes), ctypes.byref(ptr)))
    return ptr


def _eig_stage_us(lib, handle, d_k, nk, d_e, d_u, reps):
    """TBK_T_EIG per matrix (us), mean over `reps` device-resident calls after one warm-up."""
    ms = (ctypes.c_double * _lib.TBK_T_COUNT)()
    n = (ctypes.c_int64 * _lib.TBK_T_COUNT)()
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_eigh_device(handle, d_k, nk, 2, None, d_e, d_u))
    _lib.check(lib.tbk_eigenval_check(handle))
    _lib.check(lib.tbk_get_timing(handle, ms, n, 1))
    for _ in range(reps):
        _lib.check(lib.tbk_eigh_device(handle, d_k, nk, 2, None, d_e, d_u))
    _lib.check(lib.tbk_eigenval_check(handle))
    _lib.check(lib.tbk_get_timing(handle, ms, n, 1))
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    return ms[_lib.TBK_T_EIG] * 1e3 / reps / nk


def stage_table(lib, sizes, nks, reps):
    print("## TBK_T_EIG per matrix (us): own Jacobi kernel vs rocSOLVER (zheev), device-resident tbk_eigh_device")
    print("| n | NP | nk | Jacobi us/matrix | rocSOLVER us/matrix | Jacobi / rocSOLVER | sweeps | Jacobi % of FP64 vector peak |")
    print("|---|---|---|---|---|---|---|---|")
    for n in sizes:
        r_vec, hop, _ = synthetic.dense_model_arrays(n, 16, synthetic.MODEL_SEED + 500 + n)
        model = tbmodels_amd.Model.from_packed(r_vec, hop)
        handle = model._staged()
        k_all = synthetic.random_kpoints(max(nks), seed=n)
        sample = model.hamilton(k_all[:3])
        sweeps = max(jacobi_sweeps(h) for h in sample)
        NP = _padded(n)
        flops = sweeps * (n - 1) * 3 * (n // 2) * NP * 20
        for nk in nks:
            k = np.ascontiguousarray(k_all[:nk])
            d_k, d_e, d_u = (_device_array(lib, b) for b in (k.nbytes, nk * n * 8, nk * n * n * 16))
            try:
                _lib.check(lib.tbk_memcpy_h2d(0, d_k, _lib.ptr(k), k.nbytes))
                _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_AUTO))
                own = _eig_stage_us(lib, handle, d_k, nk, d_e, d_u, reps)
                _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER))
                roc = _eig_stage_us(lib, handle, d_k, nk, d_e, d_u, max(1, reps // 2) if nk >= 4096 else reps)
                _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_AUTO))
            finally:
                for ptr in (d_k, d_e, d_u):
                    lib.tbk_device_free(0, ptr)
            frac = flops / (own * 1e-6) / (FP64_VECTOR_PEAK_TFLOPS * 1e12) * 100
            print("| %d | %d | %d | %.3f | %.3f | %.2f | %d | %.2f |" % (n, NP, nk, own, roc, own / roc, sweeps, frac))
            sys.stdout.flush()


def one_k_latency(reps):
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    model = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    model.pin_staging()
    k = data["known_kpoints"][4]
    out = {}
    for name, call in (("eigenval", lambda: model.eigenval(k)), ("eigh", lambda: model.eigh(k)),
                       ("eigh convention 1", lambda: model.eigh(k, convention=1))):
        for _ in range(20):
            call()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        out[name] = (time.perf_counter() - t0) / reps * 1e6
    print("\n## silicon, one k-point per call, host buffers (us per call, mean of %d)" % reps)
    for name, us in out.items():
        print("- Model.%s: %.1f us" % (name, us))


def headline(lib, nk, reps):
    r_vec, hop, _ = synthetic.dense_model_arrays(64, 4096, synthetic.MODEL_SEED + 2)  # bench.py cfg2
    model = tbmodels_amd.Model.from_packed(r_vec, hop)
    handle = model._staged()
    k = np.ascontiguousarray(synthetic.random_kpoints(nk))
    d_k, d_e, d_u = (_device_array(lib, b) for b in (k.nbytes, nk * 64 * 8, nk * 64 * 64 * 16))
    ms = {}
    try:
        _lib.check(lib.tbk_memcpy_h2d(0, d_k, _lib.ptr(k), k.nbytes))
        calls = (("eigenval", lambda: lib.tbk_eigenval_device(handle, d_k, nk, d_e)),
                 ("eigh", lambda: lib.tbk_eigh_device(handle, d_k, nk, 2, None, d_e, d_u)))
        for name, call in calls:
            _lib.check(call())
            _lib.check(lib.tbk_eigenval_check(handle))
            t0 = time.perf_counter()
            for _ in range(reps):
                _lib.check(call())
            _lib.check(lib.tbk_eigenval_check(handle))
            ms[name] = (time.perf_counter() - t0) / reps * 1e3
    finally:
        for ptr in (d_k, d_e, d_u):
            lib.tbk_device_free(0, ptr)
    print("\n## 64 orbitals, 4096 lattice vectors (bench.py cfg2), %d k-points, device-resident (ms per call, mean of %d)" % (nk, reps))
    for name, v in ms.items():
        print("- %s: %.2f ms (%.3f us per k-point)" % (name, v, v * 1e3 / nk))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="fewer sizes (a smoke run of the tool)")
    args = ap.parse_args()
    lib = _lib.lib()
    sizes, nks = ((8, 64), (1, 64)) if args.quick else ((8, 14, 32, 64), (1, 64, 4096, 65536))
    stage_table(lib, sizes, nks, args.reps)
    one_k_latency(200 if args.quick else 2000)
    headline(lib, 4096 if args.quick else 100_000, args.reps)


if __name__ == "__main__":
    main()
