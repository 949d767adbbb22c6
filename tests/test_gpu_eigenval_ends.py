"""
The last chunk of a multi-chunk eigenvalue call (csrc/tbk_api.hip chunk_schedule).

A call ends on a short chunk of one 4096-point unit plus the ragged remainder -- or of two units plus the remainder where
tbk_hk_plan puts that length on two Strassen levels and the shorter one on a slower path.  The schedule is seen through
tbk_eigenval_schedule; models whose chunks never take two levels keep the schedule they had before the rule existed, written
down below.  Eigenvalues of a call that ends on the longer chunk are checked against the oracle on rows of both chunks.

The model is the smallest shape that reaches two levels: 32 orbitals (512 packed slots: four quarters of two element tiles,
and 8192 k-points make the 512 tiles the Strassen paths ask for; 8 and 16 orbitals pad to 128 slots, which do not divide) and
1024 lattice vectors (TBK_STRASSEN_MIN_NR).
"""

import ctypes

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib, synthetic as syn
from oracle import tbk_oracle as oracle

pytestmark = pytest.mark.gpu

UNIT = 4096
N_ORB, N_R = 32, 1024
NK = 3 * UNIT + 1696  # runs as 4096 + 9888


def _counter(model, which):
    value = ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), which, ctypes.byref(value)))
    return value.value


def _schedule(model, nk):
    lengths = (ctypes.c_int64 * 64)()
    count = ctypes.c_int(0)
    _lib.check(_lib.lib().tbk_eigenval_schedule(model._staged(), nk, lengths, 64, ctypes.byref(count)))
    assert 1 <= count.value <= 64
    return list(lengths[:count.value])


class _Device:
    """Device buffers of one test, freed at its end."""

    def __init__(self, device):
        self.device, self.ptrs = device, []

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        _lib.check(_lib.lib().tbk_device_malloc(self.device, nbytes, ctypes.byref(p)))
        self.ptrs.append(p)
        return p

    def upload(self, array):
        array = np.ascontiguousarray(array, dtype=np.float64)
        p = self.malloc(array.nbytes)
        _lib.check(_lib.lib().tbk_memcpy_h2d(self.device, p, _lib.ptr(array), array.nbytes))
        return p

    def download(self, p, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        _lib.check(_lib.lib().tbk_memcpy_d2h(self.device, _lib.ptr(out), p, out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            _lib.check(_lib.lib().tbk_device_free(self.device, p))
        return False


@pytest.fixture(scope="module")
def arrays():
    return syn.dense_model_arrays(N_ORB, N_R, syn.MODEL_SEED + 31)


@pytest.fixture(scope="module")
def model(arrays):
    r_vec, hop, pos = arrays
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def _eigenval_device(model, k):
    lib, handle = _lib.lib(), model._staged()
    with _Device(model.device) as dev:
        d_k, d_e = dev.upload(k), dev.malloc(len(k) * N_ORB * 8)
        _lib.check(lib.tbk_eigenval_device(handle, d_k, len(k), d_e))
        _lib.check(lib.tbk_synchronize(handle))
        out = dev.download(d_e, (len(k), N_ORB))
    _lib.check(lib.tbk_eigenval_check(handle))
    return out


# ---- the schedule -------------------------------------------------------------------------------------------------------

CASES = (3 * UNIT - 1, 3 * UNIT, 3 * UNIT + 1, 5 * UNIT + 1696, 100000)

# The schedules of a model that cannot take two levels, from the rule as it was before the last chunk had a choice (one unit
# plus the remainder; below three units the plain loop over the chunk).  At 32 orbitals one chunk holds the whole call.
BEFORE = {
    3 * UNIT - 1: [12287],
    3 * UNIT: [8192, 4096],
    3 * UNIT + 1: [8192, 4097],
    5 * UNIT + 1696: [16384, 5792],
    100000: [94208, 5792],
}


def _check_schedule(lengths, nk, long_last):
    assert sum(lengths) == nk
    assert all(length > 0 for length in lengths)
    if nk < 3 * UNIT:  # the plain loop: every chunk but the last is the chunk length
        assert all(length == lengths[0] for length in lengths[:-1]) and lengths[-1] <= lengths[0]
        return
    chunk = max(lengths[:-1])
    assert all(length % UNIT == 0 and length <= chunk for length in lengths[:-1])
    assert lengths[:-1] == sorted(lengths[:-1], reverse=True) and lengths[0] - lengths[-2] <= UNIT  # even shares, larger first
    lo = 2 * UNIT if long_last else UNIT
    assert lo <= lengths[-1] < lo + UNIT
    assert lengths[-1] % UNIT == nk % UNIT


@pytest.mark.parametrize("nk", CASES)
def test_schedule_of_a_two_level_model(model, nk):
    lengths = _schedule(model, nk)
    print("nk=%d: %s" % (nk, lengths))
    _check_schedule(lengths, nk, long_last=True)
    # with one level only the plan never answers "two levels": the schedule from before
    model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, 1)
    try:
        assert _schedule(model, nk) == BEFORE[nk]
    finally:
        model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, 2)
    # a fixed chunk length keeps the plain loop
    model.set_option(_lib.TBK_OPT_K_CHUNK, 2 * UNIT)
    try:
        want = [2 * UNIT] * (nk // (2 * UNIT)) + ([nk % (2 * UNIT)] if nk % (2 * UNIT) else [])
        assert _schedule(model, nk) == want
    finally:
        model.set_option(_lib.TBK_OPT_K_CHUNK, 0)


@pytest.mark.parametrize("nk", CASES)
def test_schedule_of_a_model_without_strassen_blocks(nk):
    """512 lattice vectors: fewer than the Strassen blocks need."""
    r_vec, hop, pos = syn.dense_model_arrays(N_ORB, 512, syn.MODEL_SEED + 32)
    small = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    lengths = _schedule(small, nk)
    _check_schedule(lengths, nk, long_last=False)
    assert lengths == BEFORE[nk]


def test_schedule_of_a_ragged_model_is_unchanged():
    """33 orbitals pad to 640 slots, which do not divide into quarters of whole element tiles: one level, the schedule from before."""
    r_vec, hop, pos = syn.dense_model_arrays(33, 1100, syn.MODEL_SEED + 33)
    ragged = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    # (from 33 orbitals a chunk holds 32768 k-points: the largest case runs as the headline shape used to)
    before = dict(BEFORE)
    before[100000] = [32768, 32768, 28672, 5792]
    for nk in CASES:
        assert _schedule(ragged, nk) == before[nk]


# ---- parity on the longer last chunk -------------------------------------------------------------------------------------

def test_parity_on_the_two_level_last_chunk(arrays, model):
    r_vec, hop, _ = arrays
    k = np.random.default_rng(91).random((NK, 3)) * 2.0 - 1.0
    assert _schedule(model, NK) == [UNIT, NK - UNIT]
    any0, two0 = _counter(model, _lib.TBK_CNT_STRASSEN_LAUNCHES), _counter(model, _lib.TBK_CNT_STRASSEN2_LAUNCHES)
    got = _eigenval_device(model, k)
    # the last chunk, and it alone, took two levels
    assert _counter(model, _lib.TBK_CNT_STRASSEN2_LAUNCHES) == two0 + 1
    assert _counter(model, _lib.TBK_CNT_STRASSEN_LAUNCHES) == any0 + 1
    assert np.array_equal(got, _eigenval_device(model, k))  # the same call gives the same bits
    # 64 seeded rows: the edges of both chunks and of the quarters of the last one, 24 more of the first chunk, 32 of the last
    rng = np.random.default_rng(92)
    fixed = [0, UNIT - 1, UNIT, UNIT + 1, UNIT + (NK - UNIT) // 4, UNIT + (NK - UNIT) // 2, NK - 2, NK - 1]
    head = rng.choice(np.setdiff1d(np.arange(UNIT), fixed), 24, replace=False)
    tail = rng.choice(np.setdiff1d(np.arange(UNIT, NK), fixed), 32, replace=False)
    rows = np.sort(np.r_[fixed, head, tail])
    assert len(np.unique(rows)) == 64
    want = np.array(oracle.eigenval(r_vec, hop, k[rows]))
    err = float(np.abs(got[rows] - want).max())
    print("max|dE| vs oracle on %d rows of both chunks: %.3e" % (len(rows), err))
    assert err < 1e-10
