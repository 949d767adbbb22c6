"""
Model.berry_flux measurements: prints one table.

For the silicon model on a 32^3 mesh (the valence set) and a synthetic dense model of 64 orbitals and 64 lattice vectors on a 24^3
mesh (sets of 16, 32 and 64 bands, each alone, and the three together), best of --reps after a warm-up:

1. wall time of Model.berry_flux;
2. the three stages of tbk_berry_timing per call: the link kernels, the library's LU (sets above 64 bands; none here) and the
   plaquette kernel;
3. the eigensolver stages of the same calls from tbk_get_timing (phase rows, H(k), the eigenvector solver), per call;
4. the only route to the same numbers without this call: Model.eigh of the mesh to the host and tools/berry_model.py.  Both are
   TIMED ON THE FIRST TWO PLANES of the mesh (the model on those planes as a periodic mesh of their own) AND SCALED to the mesh, and
   printed as such.

    python tools/bench_berry.py [--reps 3] [--quick]
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
import berry_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(name, model, mesh, band_lists, reps):
    lib = _lib.lib()
    n = model.size
    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)

    # the host route on two planes: their eigenvectors, then the model on them as a mesh of their own
    kpts = np.ascontiguousarray(berry_model.mesh_points(mesh))
    plane = int(np.prod(mesh[1:]))
    sub_mesh = (2,) + tuple(mesh[1:])
    model.eigh(kpts[:plane])
    t_eigh, (_, vec2) = _best(lambda: model.eigh(kpts[:2 * plane]), max(1, reps - 1))

    for bands in band_lists:
        model.berry_flux(mesh, bands)  # warm-up
        t_call, result = _best(lambda: model.berry_flux(mesh, bands), reps)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
        _lib.check(lib.tbk_berry_timing(handle, ms, ctypes.byref(calls), 1))
        model.timing(reset=True)
        for _ in range(reps):
            model.berry_flux(mesh, bands)
        _lib.check(lib.tbk_berry_timing(handle, ms, ctypes.byref(calls), 1))
        solver = model.timing(reset=True)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
        stages = [x / max(1, calls.value) for x in ms]
        eig_ms = sum(v[0] for v in solver.values()) / max(1, calls.value)
        t_model, _ = _best(lambda: berry_model.berry_flux(vec2, sub_mesh, bands), 1)
        t_host = (t_eigh + t_model) / 2 * mesh[0]
        print("| %s | %s | %d | %s | %.1f | %.1f | %.3f | %.3f | %.3f | %.1f |"
              % (name, "x".join(str(x) for x in mesh), n, " ".join("[%d,%d)" % tuple(p) for p in result.bands), t_call * 1e3, eig_ms, stages[0],
                 stages[1], stages[2], t_host * 1e3))
        print("  (%s: Chern numbers of plane (0, 1) %s, link_min %s, max |flux| %.4f turn)"
              % (name, result.chern[0].tolist() if result.chern[0].size <= 16 else "all zero: %s" % (not result.chern[0].any()),
                 np.array2string(result.link_min, precision=4), np.abs(result.flux).max() / berry_model.TWO_PI))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    print("| model | mesh | orbitals | band sets | Model.berry_flux ms | eigensolver stages of the call (tbk_get_timing) ms | links ms | library LU ms "
          "| fluxes ms | today: Model.eigh to the host + tools/berry_model.py ms (two planes, scaled) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, [4], args.reps)
    r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    measure("dense 64", dense, (6,) * 3 if args.quick else (24,) * 3, [16, 32, 64, [(0, 16), (0, 32), (0, 64)]], args.reps)


if __name__ == "__main__":
    main()
