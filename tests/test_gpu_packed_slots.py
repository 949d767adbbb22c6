"""
The packed slots of dense models (csrc/tbk_internal.h, TBK_SLOT_PAIR): two diagonal elements share one slot of the staged
operand, plane 0 Re H[i][i] and plane 1 Re H[j][j], so N orbitals take ceil(N^2 / 2) slots.  Every consumer of a slot decodes
it: the MFMA epilogue, the split-K and tail-split partial tiles with their finish kernels, the matrix-vector kernel with its
finish kernels, the one-launch kernel of small models, the derivative kernel of construct_kdotp and the folded mesh path.
Odd orbital counts end on a slot that holds one diagonal element.  Checked against the oracle over orbital counts and call
shapes, with H exactly Hermitian and Im H[i][i] exactly 0.
"""

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib, synthetic as syn
from oracle import tbk_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _close(a, b, tol=TOL):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= tol, err


def _exact_structure(ham):
    ham = np.asarray(ham)
    assert np.array_equal(ham, np.conj(np.swapaxes(ham, -1, -2)))  # exactly Hermitian
    assert not np.diagonal(ham, axis1=-2, axis2=-1).imag.any()  # Im H[i][i] exactly 0


N_ORBS = [1, 2, 3, 7, 8, 15, 16, 17, 22, 23, 33, 63, 64, 65, 128, 185, 512]


@pytest.mark.parametrize("n_orb", N_ORBS)
def test_hamilton_over_orbital_counts_and_call_shapes(n_orb):
    """One k-point (the one-launch kernel up to 22 orbitals, the matrix-vector kernel above), a few k-points (matrix-vector
    kernel and its finish kernels), a split-K batch of the MFMA kernel and a batch past it; both conventions."""
    n_r = max(2, min(300, int(4e6 / (n_orb * n_orb * 40))))
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 1100 + n_orb)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    rng = np.random.default_rng(1100 + n_orb)
    for n_k in (1, 5, 33, 200, 1000):
        if n_k > 1 and n_k * n_orb * n_orb * 16 > (256 << 20):  # (host memory of the result)
            continue
        k = rng.random((n_k, 3)) * 4.0 - 2.0
        arg = k[0] if n_k == 1 else k
        sub = slice(0, min(n_k, 12 if n_orb <= 128 else 3))
        for convention in (1, 2):
            got = np.asarray(model.hamilton(arg, convention=convention)).reshape(n_k, n_orb, n_orb)
            _exact_structure(got)
            want = oracle.hamilton(r_vec, hop, k[sub], convention, pos=pos)
            _close(got[sub], want)
    k = rng.random((5, 3))
    _close(np.array(model.eigenval(k)), np.array(oracle.eigenval(r_vec, hop, k)))


@pytest.mark.parametrize("n_orb", [7, 64, 65])
def test_tail_split_launches_and_chunks(n_orb):
    """Split-K batches and batches whose last round of tiles is split along K once more (tbk_hk_dense.hip: launch), in both
    conventions, and eigenvalues in many chunks against one chunk."""
    n_r = 1000
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 1200 + n_orb)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    rng = np.random.default_rng(1200 + n_orb)
    idx = np.array([0, 1, 127, 128, 2047, 2048, 2099])
    for n_k in (1100, 2100, 4200):
        k = rng.random((n_k, 3)) * 2.0 - 1.0
        rows = idx[idx < n_k]
        for convention in (1, 2):
            got = model.hamilton(k, convention=convention)
            _exact_structure(got)
            _close(got[rows], oracle.hamilton(r_vec, hop, k[rows], convention, pos=pos))
    whole = model.eigenval_array(k)
    _close(whole[rows], np.array(oracle.eigenval(r_vec, hop, k[rows])))
    model.set_option(_lib.TBK_OPT_K_CHUNK, 512)  # (the split of K follows the chunk: the last bits may differ)
    assert np.abs(model.eigenval_array(k) - whole).max() < 1e-12


@pytest.mark.parametrize("n_orb", [7, 8, 17])
def test_folded_mesh(n_orb):
    """Mesh planes and lines are evaluated on the operand folded along a shared k component (tbk_fold.hip works on whole
    rows of the packed operand): same eigenvalues as the direct path and the oracle."""
    n_r = 300
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 1300 + n_orb)
    axes = [np.linspace(0, 1, n, endpoint=False) for n in (3, 40, 40)]
    k = np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    folded = model.eigenval_array(k)
    model.set_option(_lib.TBK_OPT_FOLD, 0)
    direct = model.eigenval_array(k)
    assert 0.0 < np.abs(folded - direct).max() < 1e-12  # (the folded path really ran)
    sample = np.random.default_rng(n_orb).choice(len(k), 24, replace=False)
    _close(folded[sample], np.array(oracle.eigenval(r_vec, hop, k[sample])))


@pytest.mark.parametrize("n_orb", [1, 7, 8, 17, 64])
def test_construct_kdotp_and_kdotp_models(n_orb):
    """construct_kdotp reads the packed operand of a dense model (pair slots included); the k.p model it returns keeps one
    slot per element.  Both against the oracle."""
    n_r = 40
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 1400 + n_orb)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k0 = np.array([0.1, -0.3, 0.25])
    kp = model.construct_kdotp(k0, 2)
    powers, coeffs = oracle.construct_kdotp(r_vec, hop, k0, 2)
    for p, c in zip(powers.tolist(), coeffs):
        _close(kp.taylor_coefficients[tuple(p)], c, 1e-9 * max(1.0, np.abs(c).max()))
    dk = np.random.default_rng(n_orb).random((40, 3)) * 0.2 - 0.1
    herm = {p: 0.5 * (c + c.conj().T) for p, c in kp.taylor_coefficients.items()}  # exactly Hermitian coefficients
    kp_h = tbmodels_amd.KdotpModel(herm)
    got = kp_h.hamilton(dk)
    _exact_structure(got)
    p_list = sorted(herm)
    _close(got, oracle.kdotp_hamilton(np.array(p_list), np.array([herm[p] for p in p_list]), dk), 1e-9)
