"""
Model.density_matrix measurements: prints one table.

For the silicon model on a 32^3 mesh and a synthetic dense model of 64 orbitals and 64 lattice vectors on a 24^3 mesh, each with its
own hopping vectors as R, best of --reps after a warm-up:

1. wall time of Model.density_matrix and, for context, of Model.occupations of the same mesh;
2. the three stages of tbk_dm_timing per call: the phase tables, the projectors, the contraction over k + the sum of its slices;
3. the contraction's executed flops, 8 NR_pad n^2 NK, over its time, as a fraction of tbk_mfma_f64_peak;
4. the only route to the same numbers without this call: Model.eigh of the mesh to the host, Model.tetra_weights, and the einsums of
   tools/dm_model.py.  Model.eigh and the einsums are TIMED ON TWO PLANES AND SCALED to the mesh, and printed as such.

    python tools/bench_dm.py [--reps 3] [--filling 0.3] [--quick]
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


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(name, model, mesh, filling, reps, peak_tflops):
    lib = _lib.lib()
    n, n_k = filling * model.size, int(np.prod(mesh))
    model.occupations(mesh, n_electrons=n)  # warm-up of the eigenvalue and eigenvector paths
    t_occ, occ = _best(lambda: model.occupations(mesh, n_electrons=n), reps)
    model.density_matrix(mesh, n_electrons=n)
    t_dm, result = _best(lambda: model.density_matrix(mesh, n_electrons=n), reps)
    n_r = len(result.R)

    handle = model._staged()
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 3)()
    _lib.check(lib.tbk_dm_plan(n_k, model.size, n_r, plan))
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_dm_timing(handle, ms, ctypes.byref(calls), 1))
    for _ in range(reps):
        model.density_matrix(mesh, n_electrons=n)
    _lib.check(lib.tbk_dm_timing(handle, ms, ctypes.byref(calls), 1))
    model.timing(reset=True)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    stages = [x / max(1, calls.value) for x in ms]
    flops = 8.0 * plan[0] * model.size ** 2 * n_k
    fraction = flops / (stages[2] * 1e-3) / (peak_tflops * 1e12) if stages[2] > 0 else float("nan")

    # the host route: weights of the whole mesh, eigenvectors and einsums of two planes
    kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    t_w, w = _best(lambda: model.tetra_weights(mesh, result.mu.mu), reps)
    plane = int(np.prod(mesh[1:]))
    phase = dm_model.phases(mesh, result.R)

    def two_planes():
        total = np.zeros((n_r, model.size, model.size), dtype=complex)
        for p in range(2):
            rows = slice(p * plane, (p + 1) * plane)
            _, vec = model.eigh(kpts[rows])
            total += np.einsum("rk,kij->rij", phase[:, rows], dm_model.projectors(w.reshape(-1, model.size)[rows], vec))
        return total

    two_planes()
    t_planes, _ = _best(two_planes, max(1, reps - 1))
    t_host = t_w + t_planes / 2 * mesh[0]
    err_q = np.abs(np.diagonal(model.density_matrix(mesh, n_electrons=n, R=[0] * len(mesh)).rho[0]).real - occ.orbital_occ).max()
    print("| %s | %s | %d | %d | %d | %.4g | %.1f | %.1f | %.3f | %.3f | %.3f | %.3f | %.1f |"
          % (name, "x".join(str(x) for x in mesh), model.size, n_r, plan[1], n, t_dm * 1e3, t_occ * 1e3, stages[0], stages[1], stages[2], fraction,
             t_host * 1e3))
    print("  (%s: mu = %.12g, tr rho(0) - N = %.2e, max|diag rho(0) - orbital_occ| = %.2e)"
          % (name, result.mu.mu, float("nan") if not np.any(np.all(result.R == 0, axis=1)) else
             np.trace(result.rho[np.argmax(np.all(result.R == 0, axis=1))]).real - result.mu.nos, err_q))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--filling", type=float, default=0.3, help="electrons per orbital")
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    tf = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
    print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
    print("| model | mesh | orbitals | NR | k slices | n | Model.density_matrix ms | Model.occupations ms | phase tables ms | projectors ms "
          "| contraction + reduce ms | contraction / MFMA peak | today: tetra_weights + Model.eigh by planes + NumPy einsums ms (two planes, scaled) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, args.filling, args.reps, tf.value)
    r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    measure("dense 64", dense, (6,) * 3 if args.quick else (24,) * 3, args.filling, args.reps, tf.value)


if __name__ == "__main__":
    main()
