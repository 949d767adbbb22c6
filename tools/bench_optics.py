"""
Model.optical_conductivity measurements: prints one table.

For the silicon model on a 32^3 mesh, a synthetic dense model of 64 orbitals and 64 lattice vectors on a 24^3 mesh and one of 80
orbitals on an 8^3 mesh (the library route), NW in {1, 64, 512} frequencies and both conventions, best of --reps after a warm-up:

1. wall time of Model.optical_conductivity, and how many passes over the mesh the frequencies took (tbk_optics_plan);
2. the three stages of tbk_optics_timing per call: the derivative H(k) contractions, the rotation into the band basis with its
   epilogue, the reductions;
3. the eigensolver stages of the same calls from tbk_get_timing (phase rows -- the derivative rows among them --, H(k), the
   eigenvector solver), per call;
4. the only route to the same numbers without this call: Model.eigh of the mesh to the host and tools/optics_model.py.  Both are
   TIMED ON THE FIRST TWO PLANES of the mesh (the model on at most four of the frequencies) AND SCALED to the mesh and the list,
   and printed as such.

    python tools/bench_optics.py [--reps 3] [--quick]
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
import optics_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(name, model, mesh, n_el, counts, reps, host=True):
    lib = _lib.lib()
    n, n_k = model.size, int(np.prod(mesh))
    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    plan = (ctypes.c_int64 * 5)()
    r_vec, hop = model.packed_hop()
    kpts = np.ascontiguousarray(optics_model.mesh_kpoints(mesh))
    two = 2 * int(np.prod(mesh[1:]))
    if host:
        model.eigh(kpts[:two // 2])
        t_eigh, (eig2, vec2) = _best(lambda: model.eigh(kpts[:two]), max(1, reps - 1))
    for n_w in counts:
        omega = np.linspace(0.0, 8.0, n_w) if n_w > 1 else np.array([0.5])
        _lib.check(lib.tbk_optics_plan(n_k, n, len(mesh), n_w, 0, plan))
        for convention in (2, 1):
            args = dict(eta=0.05, temperature=0.05, n_electrons=n_el, convention=convention)
            model.optical_conductivity(mesh, omega, **args)  # warm-up
            t_call, result = _best(lambda: model.optical_conductivity(mesh, omega, **args), reps)
            _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
            _lib.check(lib.tbk_optics_timing(handle, ms, ctypes.byref(calls), 1))
            model.timing(reset=True)
            for _ in range(reps):
                model.optical_conductivity(mesh, omega, **args)
            _lib.check(lib.tbk_optics_timing(handle, ms, ctypes.byref(calls), 1))
            solver = model.timing(reset=True)
            _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
            stages = [x / max(1, calls.value) for x in ms]
            eig_ms = {key: value[0] / max(1, calls.value) for key, value in solver.items()}
            t_host = float("nan")
            if host:
                pos = np.asarray(model.pos, dtype=float) if convention == 1 else None
                few = omega[:min(n_w, 4)]  # (the model's loop over the frequencies is timed on four of them and scaled)
                t_model, _ = _best(lambda: optics_model.conductivity(eig2, vec2, optics_model.derivatives(r_vec.astype(np.int64), hop, kpts[:two]),
                                                                     result.mu.mu, 0.05, few, 0.05, pos), 1)
                t_host = (t_eigh + t_model * n_w / len(few)) / two * n_k
            print("| %s | %s | %d | %d | %d | %d | %.1f | %s | %.3f | %.3f | %.3f | %.1f |"
                  % (name, "x".join(str(x) for x in mesh), n, n_w, convention, plan[3], t_call * 1e3,
                     " / ".join("%s %.2f" % (key, eig_ms[key]) for key in sorted(eig_ms)), stages[0], stages[1], stages[2], t_host * 1e3))
            sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    print("| model | mesh | orbitals | NW | convention | passes | Model.optical_conductivity ms | eigensolver stages of the call (tbk_get_timing) ms | "
          "derivative H(k) ms | rotation + epilogue ms | reductions ms | today: Model.eigh to the host + tools/optics_model.py ms (two planes, scaled) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    counts = (1, 8) if args.quick else (1, 64, 512)
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (6,) * 3 if args.quick else (32,) * 3, 4.0, counts, args.reps)
    r_vec, hop, pos = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
    dense = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    measure("dense 64", dense, (4,) * 3 if args.quick else (24,) * 3, 32.0, counts, args.reps)
    r_vec, hop, pos = synthetic.dense_model_arrays(80, 16, synthetic.MODEL_SEED + 902)
    wide = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    measure("dense 80 (library route)", wide, (3,) * 3 if args.quick else (8,) * 3, 40.0, counts, args.reps)


if __name__ == "__main__":
    main()
