"""
Model.tetra_weights / Model.occupations measurements: prints one table.

For the silicon model on a 60^3 mesh and at the BASELINE config-4 shape (64 orbitals, 4096 lattice vectors, the 100^3 mesh), best
of --reps after a warm-up:

1. wall time of Model.tetra_weights (NK n doubles come back) and of Model.occupations (3 n + 4 doubles come back);
2. the three stages of tbk_occ_timing per occupations call: the weights kernel, the band sums, the contraction + its reduction;
3. Model.fermi_level and Model.pdos (one group, 201 energies) of the same mesh, for context;
4. what a user does today.  Weights: eigenval_array of the mesh to the host plus occ_model.point_weights (NumPy; timed up to
   --host-limit mesh points x orbitals, "not run" above: 24 passes over 64 M doubles at config 4).  Occupations:
   that, plus Model.eigh in plane-sized calls and a NumPy contraction -- TIMED ON TWO PLANES AND SCALED to the mesh, and printed as
   such (all eigenvectors of the config-4 mesh are 65 GB).

    python tools/bench_occ.py [--reps 3] [--filling 0.3] [--host-limit N] [--quick]
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
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import occ_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(name, model, mesh, filling, reps, host_weights):
    lib = _lib.lib()
    n = filling * model.size
    level = model.fermi_level(mesh, n)  # warm-up of the eigenvalue path
    t_fermi, level = _best(lambda: model.fermi_level(mesh, n), reps)
    model.tetra_weights(mesh, level.mu)
    t_w, w = _best(lambda: model.tetra_weights(mesh, level.mu), reps)
    model.occupations(mesh, n_electrons=n)
    t_occ, occ = _best(lambda: model.occupations(mesh, n_electrons=n), reps)

    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_occ_timing(handle, ms, ctypes.byref(calls), 1))
    for _ in range(reps):
        model.occupations(mesh, n_electrons=n)
    _lib.check(lib.tbk_occ_timing(handle, ms, ctypes.byref(calls), 1))
    model.timing(reset=True)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    stages = [x / max(1, calls.value) for x in ms]

    edges = model.band_edges(mesh)
    grid = np.linspace(edges.emin[0], edges.emax[-1], 201)
    model.pdos(mesh, grid, [[0]])
    t_pdos, _ = _best(lambda: model.pdos(mesh, grid, [[0]]), reps)

    kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    t_eig, eig = _best(lambda: np.ascontiguousarray(model.eigenval_array(kpts)).reshape(tuple(mesh) + (model.size,)), reps)
    t_model = float("nan")
    if host_weights:
        t_model, w_host = _best(lambda: occ_model.point_weights(eig, level.mu), 1)
        print("  (%s: NK max|w - NumPy model on eigenval_array| = %.2e)" % (name, w.size // model.size * np.abs(w - w_host).max()))
    plane = int(np.prod(mesh[1:]))

    def two_planes():
        total = np.zeros(model.size)
        for p in range(2):
            _, vec = model.eigh(kpts[p * plane:(p + 1) * plane])
            total += np.einsum("kb,kib->i", w.reshape(-1, model.size)[p * plane:(p + 1) * plane], np.abs(vec) ** 2)
        return total

    two_planes()
    t_planes, _ = _best(two_planes, reps)
    t_eigh_scaled = t_planes / 2 * mesh[0]
    print("| %s | %s | %d | %.4g | %.1f | %.1f | %.3f | %.3f | %.3f | %.1f | %.1f | %.1f | %s | %.1f |"
          % (name, "x".join(str(x) for x in mesh), model.size, n, t_w * 1e3, t_occ * 1e3, stages[0], stages[1], stages[2], t_fermi * 1e3,
             t_pdos * 1e3, t_eig * 1e3, "%.1f" % (t_model * 1e3) if host_weights else "not run", t_eigh_scaled * 1e3))
    print("  (%s: mu = %.12g, sum f = %.12g, sum q = %.12g, band energy = %.12g)" % (name, occ.mu.mu, occ.band_occ.sum(), occ.orbital_occ.sum(),
                                                                                  occ.band_energy.sum()))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--filling", type=float, default=0.3, help="electrons per orbital")
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    ap.add_argument("--host-limit", type=int, default=2 ** 25, help="largest NK * orbitals for which the NumPy weights of the whole mesh are timed")
    args = ap.parse_args()
    print("| model | mesh | orbitals | n | Model.tetra_weights ms | Model.occupations ms | weights kernel ms | band sums ms | contraction + reduce ms "
          "| Model.fermi_level ms | Model.pdos (1 group, 201 E) ms | today: eigenval_array ms | + occ_model.point_weights ms "
          "| + Model.eigh by planes and NumPy ms (two planes, scaled) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    mesh = (12,) * 3 if args.quick else (60,) * 3
    measure("silicon", silicon, mesh, args.filling, args.reps, int(np.prod(mesh)) * silicon.size <= args.host_limit)
    n_r = 64 if args.quick else 4096
    r_vec, hop, _ = synthetic.dense_model_arrays(64, n_r, synthetic.MODEL_SEED + 2)  # bench.py cfg2 / cfg4
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    mesh = (16,) * 3 if args.quick else (100,) * 3
    measure("config 4", dense, mesh, args.filling, args.reps, int(np.prod(mesh)) * dense.size <= args.host_limit)


if __name__ == "__main__":
    main()
