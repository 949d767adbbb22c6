"""
Model.fermi_level measurements: prints one table.

For the silicon model on a 60^3 mesh and at the BASELINE config-4 shape (64 orbitals, 4096 lattice vectors, the 100^3 mesh), at
half filling:

1. wall time of Model.fermi_level (eigenvalues of the mesh, band edges, the search; four doubles come back);
2. the time of its probe and band-edge kernels alone, from HIP events, and the passes of the search (tbk_fermi_timing);
3. what a user runs today: Model.dos of the same mesh with NE points between the band extremes and np.interp to invert nos;
4. the residual |N(mu) - n| of both answers, N from the probe kernel on the same eigenvalues (tbk_nos_at_from_eigenvalues on
   eigenval_array of the mesh): how well each mu solves N(mu) = n.  With a gap at the filling the residual is 0 for any mu inside
   it; a filling inside a band (--filling) shows the inversion error of the grid.

    python tools/bench_fermi.py [--reps 3] [--ne 2001] [--filling 0.5] [--quick]
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


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(name, model, mesh, n_e, filling, reps):
    lib = _lib.lib()
    n = filling * model.size
    model.fermi_level(mesh, n)  # warm-up
    t_fermi, level = _best(lambda: model.fermi_level(mesh, n), reps)

    handle = model._staged()
    ms, calls, passes = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_fermi_timing(handle, ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(passes), 1))
    for _ in range(reps):
        model.fermi_level(mesh, n)
    _lib.check(lib.tbk_fermi_timing(handle, ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(passes), 1))
    model.timing(reset=True)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    kernel_ms, n_passes = ms.value / max(1, calls.value), passes.value // max(1, calls.value)

    edges = model.band_edges(mesh)
    grid = np.linspace(edges.emin[0], edges.emax[-1], n_e)

    def by_grid():
        result = model.dos(mesh, grid)
        return float(np.interp(n, result.nos, result.energies))

    by_grid()  # warm-up
    t_grid, mu_grid = _best(by_grid, reps)

    eig = np.ascontiguousarray(model.eigenval_array(np.ascontiguousarray(dos_model.mesh_kpoints(mesh))))
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    probes, nos = np.array([level.mu, mu_grid]), np.zeros(2)
    _lib.check(lib.tbk_nos_at_from_eigenvalues(model.device or 0, len(mesh), _lib.ptr(mesh32), model.size, _lib.ptr(eig), _lib.ptr(probes), 2,
                                               _lib.ptr(nos)))
    print("| %s | %s | %d | %.4g | %.1f | %.3f | %d | %.1f | %.17g | %.17g | %.2e | %.2e |"
          % (name, "x".join(str(x) for x in mesh), model.size, n, t_fermi * 1e3, kernel_ms, n_passes, t_grid * 1e3, level.mu, mu_grid,
             abs(nos[0] - n), abs(nos[1] - n)))
    if level.lower < level.upper:
        print("  (%s: gap case, [%.12g, %.12g])" % (name, level.lower, level.upper))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ne", type=int, default=2001)
    ap.add_argument("--filling", type=float, default=0.5, help="electrons per orbital")
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    print("| model | mesh | orbitals | n | Model.fermi_level ms | probe + edge kernels ms | passes | Model.dos(NE = %d) + np.interp ms "
          "| mu | mu (grid) | residual | residual (grid) |" % args.ne)
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (12,) * 3 if args.quick else (60,) * 3, args.ne, args.filling, args.reps)
    measure("silicon", silicon, (12,) * 3 if args.quick else (60,) * 3, args.ne, 0.3, args.reps)
    n_r = 64 if args.quick else 4096
    r_vec, hop, _ = synthetic.dense_model_arrays(64, n_r, synthetic.MODEL_SEED + 2)  # bench.py cfg2 / cfg4
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    measure("config 4", dense, (16,) * 3 if args.quick else (100,) * 3, args.ne, args.filling, args.reps)


if __name__ == "__main__":
    main()
