"""
Model.pdos measurements: prints one table and the derived figures below it.

At the BASELINE config-4 shape (64 orbitals, 4096 lattice vectors, the 100^3 mesh) and for the silicon model on a 60^3 mesh, with
G = 4 groups:

1. wall time of Model.pdos (eigenvalues, eigenvectors and weights stay on the device, G x NE doubles come back);
2. the HIP-event time of its own kernels (tbk_pdos_timing): the weights kernel over all chunks, the accumulate kernel, the
   reduction + prefix sum -- and the achieved bandwidth of the weights kernel (it reads the chunk's U once and writes W);
3. for context, Model.dos of the same mesh and grid;
4. the baseline, what a user did before: Model.eigh in plane-sized calls (every eigenvector crosses PCIe), the weights in NumPy,
   and one weighted np.histogram per group.  It is timed on the first `--baseline-planes` planes of the mesh and scaled to the
   whole mesh (stated in the output); the full eigenvector array of config 4 is 65 GB.

    python tools/bench_pdos.py [--reps 3] [--ne 2001] [--baseline-planes 2] [--quick] [--only silicon|config4]
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
import pdos_model  # noqa: E402  pylint: disable=wrong-import-position

HBM_TBS = 8.0  # MI355X peak HBM bandwidth, TB/s


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def _baseline(model, mesh, groups, grid, planes):
    """eigh per mesh plane to the host + NumPy weights + one weighted histogram per group, on the first `planes` planes."""
    plane = int(np.prod(mesh[1:]))
    k = np.ascontiguousarray(dos_model.mesh_kpoints(mesh)[:planes * plane])
    t0 = time.perf_counter()
    hist = np.zeros((len(groups), len(grid) - 1))
    for p in range(planes):
        eig, vec = model.eigh(k[p * plane:(p + 1) * plane])
        weights = pdos_model.band_weights(vec, groups)
        for g in range(len(groups)):
            hist[g] += np.histogram(eig, bins=len(grid) - 1, range=(grid[0], grid[-1]), weights=weights[:, g, :])[0]
    return (time.perf_counter() - t0) * mesh[0] / planes


def measure(name, model, mesh, groups, n_e, reps, baseline_planes):
    lib = _lib.lib()
    nk = int(np.prod(mesh))
    plane = np.ascontiguousarray(dos_model.mesh_kpoints(mesh)[:nk // mesh[0]])
    eig = model.eigenval_array(plane)  # the window: one plane's spectrum with a wide margin
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.25 * span, eig.max() + 0.25 * span, n_e)
    model.pdos(mesh, grid, groups)  # warm-up
    model.dos(mesh, grid)
    t_pdos, result = _best(lambda: model.pdos(mesh, grid, groups), reps)
    t_dos, total = _best(lambda: model.dos(mesh, grid), reps)

    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_pdos_timing(handle, ms, ctypes.byref(calls), 1))
    model.pdos(mesh, grid, groups)
    _lib.check(lib.tbk_pdos_timing(handle, ms, ctypes.byref(calls), 1))
    stages = model.timing(reset=True)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    weights_ms, accumulate_ms, finish_ms = (value / max(1, calls.value) for value in ms)

    t_base = _baseline(model, mesh, groups, grid, min(baseline_planes, mesh[0]))
    assert np.all(result.nos[:, 0] == 0.0), result.nos[:, 0]
    n = model.size
    simplices = (6 if len(mesh) == 3 else 2) * nk * n
    traffic = nk * n * (n * 16 + len(groups) * 8)  # U read once, W written
    print("| %s | %s | %d | %d | %d | %.1f | %.3f / %.3f / %.3f | %.1f | %.0f | %.1f |"
          % (name, "x".join(str(m) for m in mesh), n, len(groups), n_e, t_pdos * 1e3, weights_ms, accumulate_ms, finish_ms, t_dos * 1e3,
             t_base * 1e3, t_base / t_pdos))
    print("  (%s: baseline timed on %d of %d planes and scaled; sum over the groups against Model.dos: %.2e)"
          % (name, min(baseline_planes, mesh[0]), mesh[0], np.abs(result.nos.sum(axis=0) - total.nos).max()))
    print("  (%s: weights kernel %.2f TB/s = %.0f %% of %.0f TB/s; accumulate %.2f ns per simplex, %.2f G simplices/s; stage timers %s)"
          % (name, traffic / (weights_ms * 1e-3) / 1e12, 100.0 * traffic / (weights_ms * 1e-3) / 1e12 / HBM_TBS, HBM_TBS,
             accumulate_ms * 1e6 / simplices, simplices / (accumulate_ms * 1e-3) / 1e9,
             ", ".join("%s %.1f ms" % (key, value[0]) for key, value in stages.items())))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ne", type=int, default=2001)
    ap.add_argument("--baseline-planes", type=int, default=2)
    ap.add_argument("--only", choices=("silicon", "config4"), default=None)
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    print("| model | mesh | orbitals | G | NE | Model.pdos ms | weights / accumulate / reduce+scan kernels ms | Model.dos ms "
          "| eigh + NumPy + np.histogram ms | baseline / Model.pdos |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    if args.only in (None, "silicon"):
        data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
        silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
        # s and p orbitals of the two atoms
        measure("silicon", silicon, (12,) * 3 if args.quick else (60,) * 3, [[0], [1, 2, 3], [4], [5, 6, 7]], args.ne, args.reps,
                args.baseline_planes)
    if args.only in (None, "config4"):
        n_r = 64 if args.quick else 4096
        r_vec, hop, _ = synthetic.dense_model_arrays(64, n_r, synthetic.MODEL_SEED + 2)  # bench.py cfg2 / cfg4
        dense = tbmodels_amd.Model.from_packed(r_vec, hop)
        groups = [list(range(16 * g, 16 * g + 16)) for g in range(4)]
        measure("config 4", dense, (16,) * 3 if args.quick else (100,) * 3, groups, args.ne, args.reps, args.baseline_planes)


if __name__ == "__main__":
    main()
