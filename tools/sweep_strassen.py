#!/usr/bin/env python3
"""H(k) stage time of one chunk on the classical product, one Strassen level and two, over the chunk length.

    python tools/sweep_strassen.py [--orbitals 64] [--vectors 4096] NK [NK ...]

One line per length: HIP-event times (TBK_OPT_TIMING) of the phase-row stage and the H(k) stage (contraction + combine) of
tbk_hamilton_device into a device buffer, the best of three calls after a warm-up, and the counters that show which path ran.
The thresholds TBK_STRASSEN_MIN_NK / TBK_STRASSEN2_MIN_NK (csrc/tbk_internal.h) are set where the faster path changes; to see
a path below its threshold, build with the threshold lowered.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tbmodels_amd  # noqa: E402
from tbmodels_amd import _lib, synthetic as syn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--orbitals", type=int, default=64)
ap.add_argument("--vectors", type=int, default=4096)
ap.add_argument("nk", type=int, nargs="+")
args = ap.parse_args()

lib = _lib.lib()
r_vec, hop, pos = syn.dense_model_arrays(args.orbitals, args.vectors, syn.MODEL_SEED)
model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
handle = model._staged()
n = args.orbitals
nk_max = max(args.nk)
k = np.ascontiguousarray(np.random.default_rng(1).random((nk_max, r_vec.shape[1])) * 2.0 - 1.0)
d_k, d_h = ctypes.c_void_p(), ctypes.c_void_p()
_lib.check(lib.tbk_device_malloc(model.device, k.nbytes, ctypes.byref(d_k)))
_lib.check(lib.tbk_device_malloc(model.device, nk_max * n * n * 16, ctypes.byref(d_h)))
_lib.check(lib.tbk_memcpy_h2d(model.device, d_k, _lib.ptr(k), k.nbytes))


def counter(which):
    value = ctypes.c_int64(-1)
    _lib.check(lib.tbk_model_counter(handle, which, ctypes.byref(value)))
    return value.value


def stage_ms(nk):
    best = None
    for rep in range(4):
        model.timing()
        _lib.check(lib.tbk_hamilton_device(handle, d_k, nk, 2, None, d_h))
        _lib.check(lib.tbk_synchronize(handle))
        t = model.timing()
        got = (t["hk"][0], t["phase"][0])
        if rep > 0 and (best is None or got[0] < best[0]):
            best = got
    return best


model.set_option(_lib.TBK_OPT_TIMING, 1)
try:
    for nk in args.nk:
        row = []
        for name, on, levels in (("classical", 0, 1), ("one level", 1, 1), ("two levels", 1, 2)):
            model.set_option(_lib.TBK_OPT_STRASSEN, on)
            model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, levels)
            c0 = counter(_lib.TBK_CNT_STRASSEN_LAUNCHES), counter(_lib.TBK_CNT_STRASSEN2_LAUNCHES)
            hk, phase = stage_ms(nk)
            took = 2 if counter(_lib.TBK_CNT_STRASSEN2_LAUNCHES) > c0[1] else 1 if counter(_lib.TBK_CNT_STRASSEN_LAUNCHES) > c0[0] else 0
            row.append("%s: hk %.3f ms, rows %.3f ms, levels run %d" % (name, hk, phase, took))
        print("nk=%6d  %s" % (nk, " | ".join(row)), flush=True)
finally:
    model.set_option(_lib.TBK_OPT_STRASSEN, 1)
    model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, 2)
    _lib.check(lib.tbk_device_free(model.device, d_k))
    _lib.check(lib.tbk_device_free(model.device, d_h))
