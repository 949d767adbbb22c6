"""
Model.transport_distribution measurements: prints one table and the derived figures below it.

For the silicon model on a 60^3 mesh and a synthetic 64-orbital model (64 lattice vectors) on 32^3:

1. wall time of Model.transport_distribution (eigenvalues, eigenvectors, derivatives and velocity matrices stay on the device,
   dim (dim + 1) / 2 x NE doubles come back);
2. the HIP-event time of its own kernels (tbk_tdf_timing): the derivative H(k) contractions, the weights kernel (rotation into the
   band basis and epilogue), accumulate + reduction + scan -- and the eigensolver stages beside them (Model.timing);
3. for context, Model.pdos of the same mesh and grid with as many groups as there are channels;
4. the host route a user runs today: Model.eigh in plane-sized calls (every eigenvector crosses PCIe), dH/dk and the weights in NumPy
   (tools/tdf_model.py), one weighted np.histogram per channel.  It is timed on the first `--baseline-planes` planes of the mesh and
   SCALED to the whole mesh, not measured on it (stated in the output).

    python tools/bench_tdf.py [--reps 3] [--ne 2001] [--baseline-planes 2] [--quick] [--only silicon|dense64]
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
import optics_model  # noqa: E402  pylint: disable=wrong-import-position
import tdf_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def _baseline(model, r_vec, hop, mesh, grid, planes):
    """eigh per mesh plane to the host + NumPy dH/dk and weights + one weighted histogram per channel, on the first `planes` planes."""
    plane = int(np.prod(mesh[1:]))
    k = np.ascontiguousarray(dos_model.mesh_kpoints(mesh)[:planes * plane])
    t0 = time.perf_counter()
    hist = None
    for p in range(planes):
        kp = k[p * plane:(p + 1) * plane]
        eig, vec = model.eigh(kp)
        ch = tdf_model.channels(eig, vec, optics_model.derivatives(r_vec, hop, kp))
        if hist is None:
            hist = np.zeros((ch.shape[1], len(grid) - 1))
        for g in range(ch.shape[1]):
            hist[g] += np.histogram(eig, bins=len(grid) - 1, range=(grid[0], grid[-1]), weights=ch[:, g, :])[0]
    return (time.perf_counter() - t0) * mesh[0] / planes


def measure(name, model, mesh, n_e, reps, baseline_planes):
    lib = _lib.lib()
    nk = int(np.prod(mesh))
    r_vec, hop = model.packed_hop()
    r_vec = r_vec.astype(np.int64)
    plane = np.ascontiguousarray(dos_model.mesh_kpoints(mesh)[:nk // mesh[0]])
    eig = model.eigenval_array(plane)  # the window: one plane's spectrum with a wide margin
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.25 * span, eig.max() + 0.25 * span, n_e)
    channels = len(mesh) * (len(mesh) + 1) // 2
    groups = [[g % model.size] for g in range(channels)]
    model.transport_distribution(mesh, grid)  # warm-up
    model.pdos(mesh, grid, groups)
    t_tdf, result = _best(lambda: model.transport_distribution(mesh, grid), reps)
    t_pdos, _ = _best(lambda: model.pdos(mesh, grid, groups), reps)

    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_tdf_timing(handle, ms, ctypes.byref(calls), 1))
    model.timing(reset=True)
    model.transport_distribution(mesh, grid)
    _lib.check(lib.tbk_tdf_timing(handle, ms, ctypes.byref(calls), 1))
    stages = model.timing(reset=True)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    dh_ms, weights_ms, tail_ms = (value / max(1, calls.value) for value in ms)

    t_base = _baseline(model, r_vec, hop, mesh, grid, min(baseline_planes, mesh[0]))
    n = model.size
    print("| %s | %s | %d | %d | %d | %.1f | %.3f / %.3f / %.3f | %.1f | %.0f | %.1f |"
          % (name, "x".join(str(m) for m in mesh), n, channels, n_e, t_tdf * 1e3, dh_ms, weights_ms, tail_ms, t_pdos * 1e3, t_base * 1e3, t_base / t_tdf))
    print("  (%s: the host route was timed on %d of %d planes and SCALED, not measured on the whole mesh; trace of N at the top of the grid %.6f)"
          % (name, min(baseline_planes, mesh[0]), mesh[0], float(np.trace(result.cumulative[:, :, -1]))))
    print("  (%s: eigensolver and H(k) stage timers of the timed call: %s)" % (name, ", ".join("%s %.1f ms" % (key, value[0]) for key, value in stages.items())))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ne", type=int, default=2001)
    ap.add_argument("--baseline-planes", type=int, default=2)
    ap.add_argument("--only", choices=("silicon", "dense64"), default=None)
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    print("| model | mesh | orbitals | G | NE | Model.transport_distribution ms | dH/dk / weights / accumulate+reduce+scan kernels ms | Model.pdos (G groups) ms "
          "| eigh + NumPy + np.histogram ms (scaled) | host route / Model.transport_distribution |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    if args.only in (None, "silicon"):
        data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
        silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
        measure("silicon", silicon, (12,) * 3 if args.quick else (60,) * 3, args.ne, args.reps, args.baseline_planes)
    if args.only in (None, "dense64"):
        r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
        dense = tbmodels_amd.Model.from_packed(r_vec, hop)
        measure("dense 64", dense, (8,) * 3 if args.quick else (32,) * 3, args.ne, args.reps, args.baseline_planes)


if __name__ == "__main__":
    main()
