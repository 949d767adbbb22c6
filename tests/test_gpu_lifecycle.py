"""
Device memory comes back when a handle is dropped.

Every cycle stages a model, runs each family of entry points once (so that every workspace of the handle, its fold plans and
its timers exist), drops the handle and, on alternate cycles, does the same with a CSR model or a k.p model.  The free device
memory after the warm-up cycles is compared with the free memory after the measured ones.

What the bound can see: ``DevBuf::reserve`` rounds to 1 MiB, so one workspace leaked per cycle costs at least 16 MiB over the
16 measured cycles; the slack is 8 MiB (0.5 MiB per cycle), half of that.  What it cannot see: a leaked ``hipMalloc`` below the
page size (the small staged arrays of a model), which the runtime serves from memory it already holds.
"""

import ctypes
import gc

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn

pytestmark = pytest.mark.gpu

WARM_UP, MEASURED = 2, 16
SLACK_PER_CYCLE = 1 << 19  # 0.5 MiB
MESH = (2, 3, 2)


def _free_bytes():
    free_b, total_b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().tbk_device_mem_info(0, ctypes.byref(free_b), ctypes.byref(total_b)))
    return free_b.value


def _cycle(index):
    seed = syn.MODEL_SEED + 1500 + index
    r_vec, hop, pos = syn.dense_model_arrays(8, 64, seed)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k = syn.uniform_grid(4)
    eig = np.array(model.eigenval_array(k))  # a mesh in meshgrid order: the folded path and its plans
    model.hamilton(k[:2], convention=1)
    model.eigh(k[:4])
    grid = np.linspace(eig.min() - 1.0, eig.max() + 1.0, 65)
    model.dos(MESH, grid)
    model.pdos(MESH, grid, [[0, 1], [2, 3, 4], [5, 6, 7]])
    model.fermi_level(MESH, 3.5)
    model.occupations(MESH, n_electrons=3.5)
    if index % 2 == 0:
        r_vec, r_ptr, row, col, val, pos = syn.csr_model_arrays(8, 64, seed)
        other = tbmodels_amd.Model.from_packed(r_vec, syn.csr_to_dense(8, r_ptr, row, col, val), pos=pos, sparse=True)
    else:
        other = model.construct_kdotp(np.array([0.1, -0.3, 0.25]), 2)
    other.eigenval(k[1])
    del model, other
    gc.collect()


def test_dropped_handles_give_their_device_memory_back():
    for index in range(WARM_UP):
        _cycle(index)
    before = _free_bytes()
    for index in range(WARM_UP, WARM_UP + MEASURED):
        _cycle(index)
    after = _free_bytes()
    print("free device memory: %d bytes after cycle %d, %d after cycle %d: dropped by %.3f MiB"
          % (before, WARM_UP, after, WARM_UP + MEASURED, (before - after) / 2.0 ** 20))
    assert before - after <= MEASURED * SLACK_PER_CYCLE
