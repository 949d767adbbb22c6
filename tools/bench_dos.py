"""
Model.dos measurements: prints one table.

At the BASELINE config-4 shape (64 orbitals, 4096 lattice vectors, the 100^3 mesh) and for the silicon model on a 60^3 mesh:

1. wall time of Model.dos (the eigenvalues stay on the device, NE doubles come back);
2. wall time of what a user did before it existed, on the same mesh: eigenval_array (every eigenvalue crosses PCIe) followed by
   np.histogram with the same number of bins -- the baseline; its two parts are printed apart;
3. the time of the density-of-states kernels alone, from HIP events (tbk_dos_timing).

    python tools/bench_dos.py [--reps 3] [--ne 2001] [--quick]
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


def measure(name, model, mesh, n_e, reps):
    lib = _lib.lib()
    k = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    eig = model.eigenval_array(k)  # warm-up of the eigenvalue path; the window comes from its result
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.05 * span, eig.max() + 0.05 * span, n_e)
    model.dos(mesh, grid)  # warm-up of the density-of-states path
    t_dos, result = _best(lambda: model.dos(mesh, grid), reps)
    t_eig, eig = _best(lambda: model.eigenval_array(k), reps)
    t_hist, _ = _best(lambda: np.histogram(eig, bins=n_e - 1, range=(grid[0], grid[-1])), 1)

    handle = model._staged()
    ms, calls = ctypes.c_double(0.0), ctypes.c_int64(0)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
    _lib.check(lib.tbk_dos_timing(handle, ctypes.byref(ms), ctypes.byref(calls), 1))
    for _ in range(reps):
        model.dos(mesh, grid)
    _lib.check(lib.tbk_dos_timing(handle, ctypes.byref(ms), ctypes.byref(calls), 1))
    model.timing(reset=True)
    _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
    kernel_ms = ms.value / max(1, calls.value)

    assert result.nos[0] == 0.0 and result.nos[-1] == float(model.size), (result.nos[0], result.nos[-1])
    nk = len(k)
    print("| %s | %s | %d | %d | %.1f | %.1f (%.1f + %.1f) | %.3f | %.1f |"
          % (name, "x".join(str(n) for n in mesh), model.size, n_e, t_dos * 1e3, (t_eig + t_hist) * 1e3, t_eig * 1e3, t_hist * 1e3,
             kernel_ms, (t_eig + t_hist) / t_dos))
    print("  (%s: %.2f M k-points/s through Model.dos; kernels alone %.2f G simplices/s)"
          % (name, nk / t_dos / 1e6, (6 if len(mesh) == 3 else 2) * nk * model.size / (kernel_ms * 1e-3) / 1e9))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ne", type=int, default=2001)
    ap.add_argument("--quick", action="store_true", help="small meshes (a smoke run of the tool)")
    args = ap.parse_args()
    print("| model | mesh | orbitals | NE | Model.dos ms | eigenval_array + np.histogram ms (parts) | DOS kernels ms | baseline / Model.dos |")
    print("|---|---|---|---|---|---|---|---|")
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (12,) * 3 if args.quick else (60,) * 3, args.ne, args.reps)
    n_r = 64 if args.quick else 4096
    r_vec, hop, _ = synthetic.dense_model_arrays(64, n_r, synthetic.MODEL_SEED + 2)  # bench.py cfg2 / cfg4
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    measure("config 4", dense, (16,) * 3 if args.quick else (100,) * 3, args.ne, args.reps)


if __name__ == "__main__":
    main()
