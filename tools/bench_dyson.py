"""
Model.green_function(self_energy=...) measurements: prints one table.

Synthetic dense models of 16, 32, 64 and 80 orbitals (16 hopping vectors) on a 24^3 mesh -- the mesh tools/bench_green.py takes for
its dense model -- with the local function (R = 0) at 16 energies of the retarded line and a causal random self-energy, best of
--reps after a warm-up:

1. wall time of the dressed call and its stages per call: H(k) (tbk_get_timing, summed) and the three of tbk_green_dressed_timing,
   the phase tables, the inversions, the contractions over k + the sums of their slices;
2. the inversions' 8 n^3 NK NZ flops over their time as a fraction of tbk_mfma_f64_peak measured in the same run;
3. the same call with the library route forced (TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER; 80 orbitals take it anyway): its inversion
   stage (forming, rocsolver_zgetrf / zgetri_strided_batched, scatter);
4. Model.green_function of the same mesh, energies and vectors WITHOUT a self-energy, which pays one eigensolve per mesh point that
   the dressed call does not, and its eigensolver stages.

A variant build of the library is measured by pointing TBK_LIBTBK at it (tools/build_variants.sh).

    python tools/bench_dyson.py [--reps 3] [--quick]
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
from tbmodels_amd import _lib, synthetic  # noqa: E402  pylint: disable=wrong-import-position
import dyson_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def _stages(model, call, reps):
    """(H(k) and eigensolver ms, [phase, inversions, contractions] ms) per call of the dressed family"""
    lib, handle = _lib.lib(), model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_green_dressed_timing(handle, ms, ctypes.byref(calls), 1))
    model.timing(reset=True)
    for _ in range(reps):
        call()
    _lib.check(lib.tbk_green_dressed_timing(handle, ms, ctypes.byref(calls), 1))
    pipeline = sum(value[0] for value in model.timing(reset=True).values()) / reps
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    return pipeline, [x / max(1, calls.value) for x in ms]


def measure(n, mesh, n_z, reps, peak_tflops):
    r_vec, hop, _ = synthetic.dense_model_arrays(n, 16, synthetic.MODEL_SEED + 3000 + n)
    z = np.linspace(-3.0, 3.0, n_z) + 0.1j
    sigma = np.ascontiguousarray(dyson_model.causal_case(n, 1, z, 3100 + n)[1])
    origin = [0, 0, 0]
    n_k = int(np.prod(mesh))
    own = tbmodels_amd.Model.from_packed(r_vec, hop)
    dressed = lambda m: (lambda: m.green_function(mesh, z, R=origin, self_energy=sigma))  # noqa: E731
    dressed(own)()  # warm-up
    t_own, result = _best(dressed(own), reps)
    hk_ms, st = _stages(own, dressed(own), reps)
    share = 8.0 * n ** 3 * n_k * n_z / (st[1] * 1e-3) / (peak_tflops * 1e12) if st[1] > 0 else float("nan")
    # without a self-energy: the parent's call for the same transform
    own.green_function(mesh, z, R=origin)
    t_plain, _ = _best(lambda: own.green_function(mesh, z, R=origin), reps)
    own.timing(reset=True)
    own.set_option(_lib.TBK_OPT_TIMING, 1)
    own.green_function(mesh, z, R=origin)
    eig_ms = sum(value[0] for value in own.timing(reset=True).values())
    own.set_option(_lib.TBK_OPT_TIMING, 0)
    # the library route on request
    forced = tbmodels_amd.Model.from_packed(r_vec, hop)
    forced.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    dressed(forced)()
    t_lib, by_library = _best(dressed(forced), reps)
    _, st_lib = _stages(forced, dressed(forced), reps)
    diff = np.abs(by_library.G - result.G).max()
    print("| %d | %s | %d | %s | %.1f | %.2f | %.3f | %.2f | %.3f | %.3f | %.1f | %.2f | %.1f | %.1f | %.1e |"
          % (n, "x".join(str(x) for x in mesh), n_z, "library" if n > 64 else "own kernel", t_own * 1e3, hk_ms, st[0], st[1], st[2], share, t_lib * 1e3,
             st_lib[1], t_plain * 1e3, eig_ms, diff))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a small mesh (a smoke run of the tool)")
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 32, 64, 80])
    args = ap.parse_args()
    tf = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
    print("library: %s" % _lib.LIB_PATH)
    print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
    print("| orbitals | mesh | NZ | inversion route | dressed call ms | H(k) ms | phase tables ms | inversions ms | contraction + reduce ms "
          "| inversions / MFMA peak (8 n^3 flops) | dressed call, library route ms | its inversions ms | green_function without Sigma ms "
          "| its H(k) + eigensolver ms | max|own - library| |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    mesh = (6,) * 3 if args.quick else (24,) * 3
    for n in args.sizes:
        measure(n, mesh, 16, args.reps, tf.value)


if __name__ == "__main__":
    main()
