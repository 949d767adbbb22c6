"""
One Strassen level in the dense H(k) contraction (csrc/tbk_hk_dense.hip launch_strassen): long k chunks
of dense models with at least 1024 lattice vectors take seven half-size products instead of eight.  Checked against the
classical product of the same handle (TBK_OPT_STRASSEN = 0), against the oracle, and for bitwise repeatability; the counter
TBK_CNT_STRASSEN_LAUNCHES shows which path ran.
"""

import ctypes

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib, synthetic as syn
from oracle import tbk_oracle as oracle

pytestmark = pytest.mark.gpu


def _counter(model, which):
    value = ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), which, ctypes.byref(value)))
    return value.value


def _strassen_launches(model):
    return _counter(model, _lib.TBK_CNT_STRASSEN_LAUNCHES)


def _hamilton_device(model, k, convention, pos):
    """FULL H(k) through tbk_hamilton_device (the host entry downloads in chunks of at most 128 MiB, too short for the path)."""
    lib = _lib.lib()
    k = np.ascontiguousarray(k, dtype=np.float64)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = pos.shape[0]
    out = np.empty((len(k), n, n), dtype=np.complex128)
    ptrs = []
    try:
        for nbytes in (k.nbytes, pos.nbytes, out.nbytes):
            p = ctypes.c_void_p()
            _lib.check(lib.tbk_device_malloc(model.device, nbytes, ctypes.byref(p)))
            ptrs.append(p)
        d_k, d_pos, d_h = ptrs
        _lib.check(lib.tbk_memcpy_h2d(model.device, d_k, _lib.ptr(k), k.nbytes))
        _lib.check(lib.tbk_memcpy_h2d(model.device, d_pos, _lib.ptr(pos), pos.nbytes))
        _lib.check(lib.tbk_hamilton_device(model._staged(), d_k, len(k), convention, d_pos if convention == 1 else None, d_h))
        _lib.check(lib.tbk_synchronize(model._staged()))
        _lib.check(lib.tbk_memcpy_d2h(model.device, _lib.ptr(out), d_h, out.nbytes))
    finally:
        for p in ptrs:
            _lib.check(lib.tbk_device_free(model.device, p))
    return out


def _max_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def _both_paths(model, fn):
    """fn() with the Strassen path on (asserting that it ran), then with TBK_OPT_STRASSEN = 0 (asserting that it did not)."""
    before = _strassen_launches(model)
    fast = fn()
    assert _strassen_launches(model) > before
    model.set_option(_lib.TBK_OPT_STRASSEN, 0)
    try:
        before = _strassen_launches(model)
        slow = fn()
        assert _strassen_launches(model) == before
    finally:
        model.set_option(_lib.TBK_OPT_STRASSEN, 1)
    return fast, slow


@pytest.fixture(scope="module")
def headline():
    r_vec, hop, pos = syn.dense_model_arrays(64, 4096, syn.MODEL_SEED)
    return r_vec, hop, pos, tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def test_headline_hamilton_both_conventions(headline):
    r_vec, hop, pos, model = headline
    k = np.random.default_rng(31).random((20000, 3)) * 2.0 - 1.0
    for convention in (1, 2):
        fast, slow = _both_paths(model, lambda: _hamilton_device(model, k, convention, pos))
        assert np.array_equal(fast, np.conj(np.swapaxes(fast, -1, -2)))  # exactly Hermitian
        assert not np.diagonal(fast, axis1=-2, axis2=-1).imag.any()
        assert _max_err(fast, slow) <= 1e-12
        # k-points of both halves of the chunk, against the oracle
        sub = np.r_[0:4, 9998:10004, 19996:20000]
        assert _max_err(fast[sub], oracle.hamilton(r_vec, hop, k[sub], convention, pos=pos)) <= 1e-10
        del fast, slow


def test_headline_eigenvalues_repeat_and_windows(headline):
    r_vec, hop, pos, model = headline
    k = np.random.default_rng(32).random((20000, 3)) * 2.0 - 1.0
    fast, slow = _both_paths(model, lambda: np.array(model.eigenval(k)))
    assert _max_err(fast, slow) <= 1e-12
    again = np.array(model.eigenval(k))
    assert np.array_equal(fast, again)  # the same call gives the same bits
    for lo in (0, 10000, 19980):  # 20-point windows take the matrix-vector path: classical sums
        assert _max_err(np.array(model.eigenval(k[lo:lo + 20])), fast[lo:lo + 20]) <= 1e-12


def test_ragged_shapes():
    """Odd orbital count (a single diagonal in the last slot), n_r not a multiple of 16, nk not a multiple of 256."""
    n_orb, n_r, n_k = 33, 1100, 9001
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 7)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k = np.random.default_rng(33).random((n_k, 3)) * 4.0 - 2.0
    for convention in (1, 2):
        fast, slow = _both_paths(model, lambda: _hamilton_device(model, k, convention, pos))
        assert _max_err(fast, slow) <= 1e-12
        sub = np.r_[0:3, 4499:4503, n_k - 3:n_k]
        assert _max_err(fast[sub], oracle.hamilton(r_vec, hop, k[sub], convention, pos=pos)) <= 1e-10
    fast, slow = _both_paths(model, lambda: np.array(model.eigenval(k)))
    assert _max_err(fast, slow) <= 1e-12


def test_structural_zeros_and_decoupled_scales():
    """Two decoupled blocks whose scales differ by 1e6 and structural zeros: Strassen mixes slot halves and k halves, so
    the small block sees rounding of the large one at the level of max|H|, not more."""
    n_orb, n_r, n_k = 32, 1024, 12000
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 8)
    hop = hop.copy()
    hop[:, :16, 16:] = 0.0
    hop[:, 16:, :16] = 0.0
    hop[:, :16, :16] *= 1e3
    hop[:, 16:, 16:] *= 1e-3
    hop[:, 3, :] = 0.0  # an orbital coupled to nothing but itself
    hop[:, :, 3] = 0.0
    hop[0, 3, 3] = 0.25
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k = np.random.default_rng(34).random((n_k, 3)) * 2.0 - 1.0
    fast, slow = _both_paths(model, lambda: _hamilton_device(model, k, 2, pos))
    scale = float(np.abs(slow).max())
    assert _max_err(fast, slow) <= 1e-13 * scale
    fast = slow = None
    sub = np.r_[0:8, 5996:6004]
    want = np.array(oracle.eigenval(r_vec, np.ascontiguousarray(hop[:, 16:, 16:]), k[sub]))
    got = np.array(model.eigenval(k))[sub]
    # every eigenvalue of the small block (|E| ~ 1e-3) is one of the full H's, whose others are ~1e3 away or the 0.5 of orbital 3
    err = np.abs(got[:, None, :] - want[:, :, None]).min(axis=2)
    assert float(err.max()) <= 1e-10
