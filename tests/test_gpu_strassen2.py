"""
Two Strassen levels in the dense H(k) contraction (csrc/tbk_hk_dense.hip launch_strassen2): k chunks of at
least TBK_STRASSEN2_MIN_NK k-points of models whose padding divides into quarters take 49 quarter-size products instead of 64.
Checked against one level (TBK_OPT_STRASSEN_LEVELS = 1) and the classical product (TBK_OPT_STRASSEN = 0) of the same handle,
against the oracle, and for bitwise repeatability; the counters show which path ran.  The bars are those of the one-level path.
"""

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib, synthetic as syn
from oracle import tbk_oracle as oracle

from test_gpu_strassen import _counter, _hamilton_device, _max_err

pytestmark = pytest.mark.gpu

MIN_NK2 = 8192  # TBK_STRASSEN2_MIN_NK of csrc/tbk_internal.h


def _launches(model):
    return _counter(model, _lib.TBK_CNT_STRASSEN_LAUNCHES), _counter(model, _lib.TBK_CNT_STRASSEN2_LAUNCHES)


def _three_paths(model, fn):
    """fn() on two levels, on one level and on the classical product, each shown by the counters to have run as asked."""
    any0, two0 = _launches(model)
    two = fn()
    any1, two1 = _launches(model)
    assert two1 > two0 and any1 - any0 >= two1 - two0  # (a call may end on a short chunk of one level)
    model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, 1)
    try:
        one = fn()
        any2, two2 = _launches(model)
        assert two2 == two1 and any2 > any1
        model.set_option(_lib.TBK_OPT_STRASSEN, 0)
        try:
            classical = fn()
            assert _launches(model) == (any2, two2)
        finally:
            model.set_option(_lib.TBK_OPT_STRASSEN, 1)
    finally:
        model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, 2)
    return two, one, classical


@pytest.fixture(scope="module")
def headline():
    r_vec, hop, pos = syn.dense_model_arrays(64, 4096, syn.MODEL_SEED)
    return r_vec, hop, pos, tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def test_levels_option_takes_one_or_two(headline):
    model = headline[3]
    lib = _lib.lib()
    for bad in (0, 3, -1):
        assert lib.tbk_model_set_option(model._staged(), _lib.TBK_OPT_STRASSEN_LEVELS, bad) == _lib.TBK_ERR_ARGUMENT
    model.set_option(_lib.TBK_OPT_STRASSEN_LEVELS, 2)


def test_headline_hamilton_both_conventions(headline):
    r_vec, hop, pos, model = headline
    n_k = 20000  # quarters of 5120 k-points (the last one holds 4640)
    k = np.random.default_rng(41).random((n_k, 3)) * 2.0 - 1.0
    for convention in (1, 2):
        two, one, classical = _three_paths(model, lambda: _hamilton_device(model, k, convention, pos))
        assert np.array_equal(two, np.conj(np.swapaxes(two, -1, -2)))  # exactly Hermitian
        assert not np.diagonal(two, axis1=-2, axis2=-1).imag.any()
        d_one, d_classical = _max_err(two, one), _max_err(two, classical)
        print("convention %d: max|dH| two levels vs one %.3e, vs classical %.3e" % (convention, d_one, d_classical))
        assert d_one <= 1e-12
        assert d_classical <= 1e-12
        del one, classical
        # k-points of all four quarters of the chunk, against the oracle
        sub = np.r_[0:3, 5118:5122, 10238:10242, 15358:15362, n_k - 3:n_k]
        d_oracle = _max_err(two[sub], oracle.hamilton(r_vec, hop, k[sub], convention, pos=pos))
        print("convention %d: max|dH| vs oracle %.3e" % (convention, d_oracle))
        assert d_oracle <= 1e-10
        del two


def test_headline_eigenvalues_and_repeat(headline):
    r_vec, hop, pos, model = headline
    # (the eigenvalue pipeline ends every call on a short chunk: 24000 k-points run as 16384, two levels, and 7616, one level)
    k = np.random.default_rng(42).random((24000, 3)) * 2.0 - 1.0
    two, one, classical = _three_paths(model, lambda: np.array(model.eigenval(k)))
    d_one, d_classical = _max_err(two, one), _max_err(two, classical)
    print("max|dE| two levels vs one %.3e, vs classical %.3e" % (d_one, d_classical))
    assert d_one <= 1e-12
    assert d_classical <= 1e-12
    assert np.array_equal(two, np.array(model.eigenval(k)))  # the same call gives the same bits
    sub = np.r_[0:2, 4095:4097, 8191:8193, 12287:12289, 16382:16386, 23998:24000]
    assert _max_err(two[sub], np.array(oracle.eigenval(r_vec, hop, k[sub]))) <= 1e-10


def test_chunk_below_the_threshold_takes_one_level(headline):
    r_vec, hop, pos, model = headline
    k = np.random.default_rng(43).random((MIN_NK2, 3)) * 2.0 - 1.0
    any0, two0 = _launches(model)
    below = _hamilton_device(model, k[:-1], 2, pos)
    assert _launches(model) == (any0 + 1, two0)
    at = _hamilton_device(model, k, 2, pos)
    assert _launches(model) == (any0 + 2, two0 + 1)
    assert _max_err(below, at[:-1]) <= 1e-12


def test_ragged_model_stays_on_one_level():
    """33 orbitals: 545 slots padded to 640, which do not divide into quarters of whole element tiles (and padding them to 768
    would cost more than the second level saves): long chunks keep one level."""
    n_orb, n_r, n_k = 33, 1100, 9001
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 7)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k = np.random.default_rng(44).random((n_k, 3)) * 4.0 - 2.0
    any0, two0 = _launches(model)
    fast = _hamilton_device(model, k, 1, pos)
    assert _launches(model) == (any0 + 1, two0)
    sub = np.r_[0:3, 4499:4503, n_k - 3:n_k]
    assert _max_err(fast[sub], oracle.hamilton(r_vec, hop, k[sub], 1, pos=pos)) <= 1e-10


def test_structural_zeros_and_decoupled_scales():
    """The model of test_gpu_strassen.py at a two-level length: the small block sees rounding of the large one at the level
    of max|H|, not more."""
    n_orb, n_r, n_k = 32, 1024, 20000
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 8)
    hop = hop.copy()
    hop[:, :16, 16:] = 0.0
    hop[:, 16:, :16] = 0.0
    hop[:, :16, :16] *= 1e3
    hop[:, 16:, 16:] *= 1e-3
    hop[:, 3, :] = 0.0
    hop[:, :, 3] = 0.0
    hop[0, 3, 3] = 0.25
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k = np.random.default_rng(45).random((n_k, 3)) * 2.0 - 1.0
    two, one, classical = _three_paths(model, lambda: _hamilton_device(model, k, 2, pos))
    scale = float(np.abs(classical).max())
    d_one, d_classical = _max_err(two, one), _max_err(two, classical)
    print("decoupled scales: max|dH| / max|H| two levels vs one %.3e, vs classical %.3e" % (d_one / scale, d_classical / scale))
    assert d_classical <= 1e-13 * scale
    assert d_one <= 1e-13 * scale
    two = one = classical = None
    sub = np.r_[0:8, 9996:10004]
    want = np.array(oracle.eigenval(r_vec, np.ascontiguousarray(hop[:, 16:, 16:]), k[sub]))
    got = np.array(model.eigenval(k))[sub]
    err = np.abs(got[:, None, :] - want[:, :, None]).min(axis=2)
    assert float(err.max()) <= 1e-10
