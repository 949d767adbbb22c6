"""
The two-pass Strassen combine of the eigenvalue path (csrc/tbk_hk_dense.hip launch_strassen2): the
products of a two-level chunk go as two launches, hk_strassen2_first_kernel combines the outer products 0 .. 5 on the
reduction's stream beside the second launch, hk_strassen2_close_kernel adds M7 behind it.  TBK_OPT_STRASSEN_COMBINE = 0 keeps
the single launch and the single combine; both forms must give the same bits.  The counters show which form ran.

The model is the smallest the plan puts on two levels: dense synthetic, 32 orbitals (512 slots, 8 element tiles), 1024 lattice
vectors.
"""

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib, synthetic as syn
from oracle import tbk_oracle as oracle

from test_gpu_strassen import _counter, _max_err

pytestmark = pytest.mark.gpu

BM = 128


def _mq(nk):  # tbk_strassen_mq of csrc/tbk_internal.h
    return ((nk + 3) // 4 + BM - 1) // BM * BM


def _counts(model):
    return _counter(model, _lib.TBK_CNT_STRASSEN2_LAUNCHES), _counter(model, _lib.TBK_CNT_STRASSEN2_SPLIT)


def _eigenval(model, k, combine, k_chunk):
    """(eigenvalues, two-level launches, split combines) of one call with the option set as asked."""
    model.set_option(_lib.TBK_OPT_K_CHUNK, k_chunk)
    model.set_option(_lib.TBK_OPT_STRASSEN_COMBINE, combine)
    try:
        two0, split0 = _counts(model)
        eig = np.array(model.eigenval(k))
        two1, split1 = _counts(model)
    finally:
        model.set_option(_lib.TBK_OPT_STRASSEN_COMBINE, 1)
        model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    return eig, two1 - two0, split1 - split0


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _quarter_rows(nk, per_quarter=16):
    """Up to `per_quarter` k-points of every quarter of the chunk: the first and the last ones it holds."""
    mq, rows = _mq(nk), []
    for q in range(4):
        lo, hi = q * mq, min((q + 1) * mq, nk)
        if hi <= lo:
            continue
        idx = np.r_[lo:min(lo + per_quarter // 2, hi), max(hi - per_quarter // 2, lo):hi]
        rows.extend(np.unique(idx).tolist())
    return np.array(rows)


@pytest.fixture(scope="module")
def small():
    r_vec, hop, pos = syn.dense_model_arrays(32, 1024, syn.MODEL_SEED + 10)
    return r_vec, hop, tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def test_combine_option_takes_zero_or_one(small):
    model = small[2]
    lib = _lib.lib()
    for bad in (2, -1):
        assert lib.tbk_model_set_option(model._staged(), _lib.TBK_OPT_STRASSEN_COMBINE, bad) == _lib.TBK_ERR_ARGUMENT
    model.set_option(_lib.TBK_OPT_STRASSEN_COMBINE, 1)


# the two-level threshold, one k-point past it, a ragged last quarter, whole quarters with more tiles
@pytest.mark.parametrize("nk", [8192, 8193, 8709, 12288])
def test_one_chunk_both_forms_same_bits_and_oracle(small, nk):
    r_vec, hop, model = small
    k = np.random.default_rng(100 + nk).random((nk, 3)) * 2.0 - 1.0
    split, two1, split1 = _eigenval(model, k, 1, nk)
    assert (two1, split1) == (1, 1)  # one chunk, on two levels, combined in two passes
    single, two0, split0 = _eigenval(model, k, 0, nk)
    assert (two0, split0) == (1, 0)  # ... and with the single kernel
    assert _same_bits(split, single)
    rows = _quarter_rows(nk)
    assert len(rows) >= 16 * 3
    err = _max_err(split[rows], np.array(oracle.eigenval(r_vec, hop, k[rows])))
    print("nk = %d: max|dE| vs oracle on %d rows %.3e" % (nk, len(rows), err))
    assert err <= 1e-10


def test_chunks_in_the_pipeline_same_bits_and_repeat(small):
    """Three two-level chunks and a short one: the first pass of a chunk shares the reduction's stream with the reductions of
    its neighbours."""
    r_vec, hop, model = small
    nk = 3 * 8192 + 517
    k = np.random.default_rng(7).random((nk, 3)) * 2.0 - 1.0
    split, two1, split1 = _eigenval(model, k, 1, 8192)
    assert (two1, split1) == (3, 3)
    single, two0, split0 = _eigenval(model, k, 0, 8192)
    assert (two0, split0) == (3, 0)
    assert _same_bits(split, single)
    again, two2, split2 = _eigenval(model, k, 1, 8192)
    assert (two2, split2) == (3, 3)
    assert _same_bits(split, again)
    rows = np.r_[0:4, 8190:8194, 16382:16386, 24574:24578, nk - 4:nk]
    assert _max_err(split[rows], np.array(oracle.eigenval(r_vec, hop, k[rows]))) <= 1e-10


def test_rounding_that_leaves_no_second_launch_takes_the_single_form():
    """22 orbitals (256 slots, one element tile per quarter), 18944 k-points: 40 blocks per product, and 42 x 40 units rounded up
    to whole rounds of 512 workgroup slots passes 49 x 40 -- nothing would be left to run the first pass beside."""
    n_orb, n_r, nk = 22, 1024, 18944
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 11)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k = np.random.default_rng(8).random((nk, 3)) * 2.0 - 1.0
    on, two1, split1 = _eigenval(model, k, 1, nk)
    assert two1 == 1
    assert split1 == 0, "the split ran: this test assumes the 256 compute units of an MI355X"
    off, two0, split0 = _eigenval(model, k, 0, nk)
    assert (two0, split0) == (1, 0)
    assert _same_bits(on, off)
    rows = _quarter_rows(nk)
    assert _max_err(on[rows], np.array(oracle.eigenval(r_vec, hop, k[rows]))) <= 1e-10
