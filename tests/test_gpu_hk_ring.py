"""
The K loop of hk_dense_kernel (csrc/tbk_hk_dense.hip) walks K in half stages of 8 rows through a ring of four LDS buffers whose
LDS-DMA stays in flight across the loop's barriers.  A ring goes wrong at its ends -- K ranges shorter than, equal to and longer
than the ring, odd and even stage counts, ranges that start inside K (split-K) -- and by refilling or reading a buffer a barrier
early, which is a race: it shows as different bits between two evaluations, mostly when the memory system is busy.

Every case here is held to the oracle at the 1e-10 bar of the suite and evaluated twice for identical bits; one evaluation runs
while a second model handle keeps another stream of the process busy with a large hamilton().

Which kernel a case reaches is decided by tbk_hk_plan.  Models of at most 22 orbitals (256 packed slots) with fewer than 128
lattice vectors take the matrix-vector kernel up to 4096 k-points, so the 6- and 22-orbital cases pin that path beside the
ring; the 24-orbital models (320 slots) are there to put the same stage counts -- n_r = 1, 8, 9, 16, 24, 40, 72 pad to 1, 1, 2,
2, 3, 5 and 9 stages of 16 K rows -- through the MFMA tiles.
"""

import threading

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib, synthetic as syn
from oracle import tbk_oracle as oracle

from test_gpu_strassen import _counter, _hamilton_device, _max_err

pytestmark = pytest.mark.gpu

N_ORB = (6, 22, 24)
N_R = (1, 8, 9, 16, 24, 40, 72)
N_K = (33, 128, 129, 300)
BAR = 1e-10  # max|dH| against the oracle, as everywhere in the suite


def _model(n_orb, n_r, seed):
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + seed)
    return r_vec, hop, pos, tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


@pytest.fixture(scope="module")
def kpoints():
    return np.random.default_rng(1101).random((max(N_K), 3)) * 2.0 - 1.0


@pytest.fixture(scope="module")
def load():
    """A second model handle (its own stream) whose hamilton() of 2048 k-points moves 128 MiB of H(k) per call."""
    model = _model(64, 256, 1190)[3]
    k = np.random.default_rng(1102).random((2048, 3)) * 2.0 - 1.0
    model.hamilton(k)  # staged and warm before anything is timed against it
    return model, k


class _Busy:
    """Runs `load`'s hamilton() back to back on a thread for the length of a `with` block (ctypes calls release the GIL)."""

    def __init__(self, load):
        self.model, self.k = load
        self.stop = threading.Event()
        self.running = threading.Event()
        self.calls = 0
        self.thread = threading.Thread(target=self._run)

    def _run(self):
        while not self.stop.is_set():
            self.running.set()
            self.model.hamilton(self.k)
            self.calls += 1

    def __enter__(self):
        self.thread.start()
        self.running.wait()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()


@pytest.mark.parametrize("n_r", N_R)
@pytest.mark.parametrize("n_orb", N_ORB)
def test_short_k_ranges_against_oracle_and_twice(n_orb, n_r, kpoints, load):
    r_vec, hop, pos, model = _model(n_orb, n_r, 1100 + 100 * n_orb + n_r)
    first = {}
    for n_k in N_K:
        for convention in (1, 2):
            k = kpoints[:n_k]
            got = np.array(model.hamilton(k, convention=convention))
            err = _max_err(got, oracle.hamilton(r_vec, hop, k, convention, pos=pos))
            print("n_orb %d n_r %d n_k %d convention %d: max|dH| vs oracle %.3e" % (n_orb, n_r, n_k, convention, err))
            assert err <= BAR
            assert np.array_equal(got, np.array(model.hamilton(k, convention=convention)))
            first[n_k, convention] = got
    with _Busy(load) as busy:  # the same calls once more beside a busy stream
        for (n_k, convention), want in first.items():
            assert np.array_equal(want, np.array(model.hamilton(kpoints[:n_k], convention=convention)))
    assert busy.calls >= 1


def test_split_k_ranges(load):
    """Few k-points of a long K: 24 orbitals are 5 element tiles, 40 k-points one k tile, n_r = 1024 is 128 stages -> 32 K ranges of 4
    stages, all but the first starting inside K; 300 k-points the same with three k tiles."""
    r_vec, hop, pos, model = _model(24, 1024, 1180)
    k_all = np.random.default_rng(1103).random((300, 3)) * 2.0 - 1.0
    for n_k in (40, 300):
        k = k_all[:n_k]
        for convention in (1, 2):
            got = np.array(model.hamilton(k, convention=convention))
            err = _max_err(got, oracle.hamilton(r_vec, hop, k, convention, pos=pos))
            print("split-K n_k %d convention %d: max|dH| vs oracle %.3e" % (n_k, convention, err))
            assert err <= BAR
            assert np.array_equal(got, np.array(model.hamilton(k, convention=convention)))
            with _Busy(load):
                assert np.array_equal(got, np.array(model.hamilton(k, convention=convention)))


def test_split_k_with_a_sub_split_tail():
    """600 k-points of 24 orbitals and 4096 lattice vectors: 25 tiles x 51 K ranges of 11 stages are 2.5 rounds of workgroup slots,
    so the ragged round is cut along K once more (block_offset, sub_splits) -- ranges of a few, odd and even, stages."""
    r_vec, hop, pos, model = _model(24, 4096, 1181)
    k = np.random.default_rng(1104).random((600, 3)) * 2.0 - 1.0
    got = np.array(model.hamilton(k))
    sub = np.r_[0:3, 127:130, 383:386, 597:600]
    err = _max_err(got[sub], oracle.hamilton(r_vec, hop, k[sub], 2, pos=pos))
    print("sub-split tail: max|dH| vs oracle %.3e" % err)
    assert err <= BAR
    assert np.array_equal(got, np.array(model.hamilton(k)))


def test_one_and_two_strassen_levels(load):
    """64 orbitals, 1024 lattice vectors: 4096 k-points are a one-level chunk (K / 2 = 64 stages per product), 8192 k-points a
    two-level chunk (32 stages).  Bars of tests/test_gpu_strassen.py: 1e-12 against the classical product, 1e-10 against the oracle."""
    r_vec, hop, pos, model = _model(64, 1024, 1182)
    k_all = np.random.default_rng(1105).random((8192, 3)) * 2.0 - 1.0
    for n_k, which in ((4096, _lib.TBK_CNT_STRASSEN_LAUNCHES), (8192, _lib.TBK_CNT_STRASSEN2_LAUNCHES)):
        k = k_all[:n_k]
        before = _counter(model, which)
        fast = _hamilton_device(model, k, 2, pos)
        assert _counter(model, which) == before + 1
        with _Busy(load):
            assert np.array_equal(fast, _hamilton_device(model, k, 2, pos))
        model.set_option(_lib.TBK_OPT_STRASSEN, 0)
        try:
            before = _counter(model, _lib.TBK_CNT_STRASSEN_LAUNCHES)
            slow = _hamilton_device(model, k, 2, pos)
            assert _counter(model, _lib.TBK_CNT_STRASSEN_LAUNCHES) == before
        finally:
            model.set_option(_lib.TBK_OPT_STRASSEN, 1)
        d_classical = _max_err(fast, slow)
        del slow
        sub = np.r_[0:3, n_k // 4 - 2:n_k // 4 + 2, n_k // 2 - 2:n_k // 2 + 2, n_k - 3:n_k]
        d_oracle = _max_err(fast[sub], oracle.hamilton(r_vec, hop, k[sub], 2, pos=pos))
        print("%d k-points: max|dH| vs classical %.3e, vs oracle %.3e" % (n_k, d_classical, d_oracle))
        assert d_classical <= 1e-12
        assert d_oracle <= BAR
        del fast
