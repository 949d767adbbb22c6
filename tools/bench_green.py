"""
Model.green_function measurements: prints one table.

For the silicon model on a 32^3 mesh with its own hopping vectors and 64 energies, and a synthetic dense model of 64 orbitals on a
24^3 mesh with NR = 1 and NR = 64, each at 16 and 64 energies, best of --reps after a warm-up:

1. wall time of Model.green_function;
2. the three stages of tbk_green_timing per call: the phase tables, the projectors, the contractions over k + the sums of their
   slices; and the eigensolver stages of the same calls (tbk_get_timing, summed);
3. the projector's executed flops, 8 n_pad^3 NK NZ (n_pad: n rounded up to its tile of 16), over its time, and the contraction's,
   8 NR_pad n^2 NK NZ, over its time, each as a fraction of tbk_mfma_f64_peak measured in the same run;
4. the only route to the same numbers without this call: Model.eigh of the mesh to the host and the einsums of
   tools/green_model.py.  Both are TIMED ON TWO PLANES AND SCALED to the mesh, and printed as such.

    python tools/bench_green.py [--reps 3] [--quick]
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
import dm_model  # noqa: E402  pylint: disable=wrong-import-position
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import green_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def energies(n_z, lo, hi, eta=0.1):
    """n_z points of the retarded line Im z = eta over [lo, hi]."""
    return np.linspace(lo, hi, n_z) + 1j * eta


def measure(name, model, mesh, z, vectors, reps, peak_tflops, host=True):
    lib = _lib.lib()
    n, n_k, n_z = model.size, int(np.prod(mesh)), len(z)
    model.green_function(mesh, z, R=vectors)  # warm-up
    t_call, result = _best(lambda: model.green_function(mesh, z, R=vectors), reps)
    n_r = len(result.R)

    handle = model._staged()
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 7)()
    _lib.check(lib.tbk_green_plan(n_k, n, n_r, n_z, 0, 0, plan))
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_green_timing(handle, ms, ctypes.byref(calls), 1))
    model.timing(reset=True)
    for _ in range(reps):
        model.green_function(mesh, z, R=vectors)
    _lib.check(lib.tbk_green_timing(handle, ms, ctypes.byref(calls), 1))
    eig_ms = sum(value[0] for value in model.timing(reset=True).values()) / max(1, calls.value)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    stages = [x / max(1, calls.value) for x in ms]
    n_pad = (n + 15) // 16 * 16
    share = lambda flops, t_ms: flops / (t_ms * 1e-3) / (peak_tflops * 1e12) if t_ms > 0 else float("nan")  # noqa: E731
    f_proj, f_four = share(8.0 * n_pad ** 3 * n_k * n_z, stages[1]), share(8.0 * plan[0] * n * n * n_k * n_z, stages[2])

    t_host = float("nan")
    if host:  # the host route: eigenvectors and einsums of two planes
        kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
        plane = int(np.prod(mesh[1:]))
        phase = dm_model.phases(mesh, result.R)

        def two_planes():
            total = np.zeros((n_r, n_z, n, n), dtype=complex)
            for p in range(2):
                rows = slice(p * plane, (p + 1) * plane)
                eig, vec = model.eigh(kpts[rows])
                P = green_model.projectors(np.array(eig), np.array(vec), z) * (plane / n_k)  # (projectors divides by its own point count)
                total += (phase[:, rows] @ P.reshape(plane, -1)).reshape(total.shape)
            return total

        t_planes, _ = _best(two_planes, 1)
        t_host = t_planes / 2 * mesh[0]
    print("| %s | %s | %d | %d | %d | %d | %d | %.1f | %.1f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f |"
          % (name, "x".join(str(x) for x in mesh), n, n_r, n_z, plan[1], plan[3], t_call * 1e3, eig_ms, stages[0], stages[1], stages[2], f_proj, f_four,
             t_host * 1e3))
    origin = np.all(result.R == 0, axis=1)
    if np.any(origin):
        dos = -np.trace(result.G[np.argmax(origin), n_z // 2]).imag / np.pi
        print("  (%s: -Im tr G(0, z[%d]) / pi = %.12g)" % (name, n_z // 2, dos))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    tf = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
    print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
    print("| model | mesh | orbitals | NR | NZ | k slices | z tile | Model.green_function ms | eigensolver stages ms | phase tables ms | projectors ms "
          "| contraction + reduce ms | projector / MFMA peak | contraction / MFMA peak | today: Model.eigh by planes + NumPy einsums ms (two planes, scaled) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, energies(64, -8.0, 12.0), None, args.reps, tf.value)
    r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    mesh = (6,) * 3 if args.quick else (24,) * 3
    for vectors, label in (([0, 0, 0], "dense 64, local"), (None, "dense 64")):
        for n_z in (16, 64):
            measure(label, dense, mesh, energies(n_z, -3.0, 3.0), vectors, args.reps, tf.value, host=(n_z == 16))


if __name__ == "__main__":
    main()
