"""
Model.eigh / KdotpModel.eigh on the GPU: eigenvalues against eigenval and LAPACK, residuals and orthonormality of the
eigenvectors, spectral projectors of every eigenvalue cluster, a gauge-independent Wilson loop, call-shape independence of
the Jacobi kernel, errors, several devices and the rocSOLVER branch.
"""

import pickle

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn
from oracle import tbk_oracle as oracle

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _onsite_model(mat):
    """A model whose H(k) is the constant Hermitian matrix `mat` (R = 0 block stored halved)."""
    mat = np.asarray(mat, dtype=complex)
    return tbmodels_amd.Model(hop={(0, 0, 0): mat / 2}, size=len(mat), dim=3, contains_cc=False)


def _counter(model, which):
    import ctypes  # pylint: disable=import-outside-toplevel

    value = ctypes.c_int64(0)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), which, ctypes.byref(value)))
    return value.value


def _check_vectors(H, E, U, scale=None):
    """Residual max|H U - U diag(E)| <= 1e-12 n scale and max|U^H U - I| <= 1e-12 n, per k-point."""
    H, E, U = H.reshape((-1,) + H.shape[-2:]), E.reshape(-1, E.shape[-1]), U.reshape((-1,) + U.shape[-2:])
    n = E.shape[-1]
    if scale is None:
        scale = np.maximum(1.0, np.abs(E).max(axis=1))
    scale = np.broadcast_to(scale, E.shape[:1])
    assert np.all(np.diff(E, axis=1) >= 0), "eigenvalues not ascending"
    res = np.abs(H @ U - U * E[:, None, :]).max(axis=(1, 2))
    assert np.all(res <= 1e-12 * n * scale), res.max()
    orth = np.abs(np.conj(np.swapaxes(U, 1, 2)) @ U - np.eye(n)).max()
    assert orth <= 1e-12 * n, orth


def _cluster_projectors(mat, E, U, scale):
    """
    Spectral projector of every eigenvalue cluster (gaps > 1e-8 scale in eigvalsh) against numpy.linalg.eigh's: within
    1e-9, or within what the residual bound allows a cluster whose gap to the rest of the spectrum is narrow (Davis-Kahan:
    a backward error r moves the projector by up to ~r / gap -- LAPACK's own projectors of the graded family differ by
    1e-9 to 5e-9 from one solver to the next at 31 - 129 orbitals).
    """
    n = len(E)
    ref_e, ref_u = np.linalg.eigh(mat)
    cuts = np.flatnonzero(np.diff(ref_e) > 1e-8 * scale) + 1
    for idx in np.split(np.arange(n), cuts):
        below = ref_e[idx[0]] - ref_e[idx[0] - 1] if idx[0] > 0 else np.inf
        above = ref_e[idx[-1] + 1] - ref_e[idx[-1]] if idx[-1] + 1 < n else np.inf
        tol = max(1e-9, 2 * 1e-12 * n * scale / min(below, above))
        p_ref = ref_u[:, idx] @ ref_u[:, idx].conj().T
        p_got = U[:, idx] @ U[:, idx].conj().T
        assert np.abs(p_got - p_ref).max() <= tol, (idx, np.abs(p_got - p_ref).max(), tol)


@pytest.fixture(scope="module")
def silicon_model():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"]), g


# ---- 1. silicon --------------------------------------------------------------------------------------------------------
def test_silicon_known_kpoints_and_grid(silicon_model):
    model, g = silicon_model
    for k, known in ((g["known_kpoints"], g["known_eigenvals"]), (g["grid"], g["grid_eig"])):
        E, U = model.eigh(k)
        assert E.shape == (len(k), 8) and U.shape == (len(k), 8, 8) and U.dtype == np.complex128
        scale = np.maximum(1.0, np.abs(E).max(axis=1))
        assert np.all(np.abs(E - model.eigenval_array(k)).max(axis=1) <= 1e-12 * scale)
        assert np.abs(E - known).max() <= 1e-10
        _check_vectors(model.hamilton(k), E, U)
    e1, u1 = model.eigh(g["known_kpoints"][3])
    assert e1.shape == (8,) and u1.shape == (8, 8)
    _check_vectors(model.hamilton(g["known_kpoints"][3]), e1, u1)


# ---- 2. structured matrices --------------------------------------------------------------------------------------------
def _structured_cases(n):
    """The families of test_gpu_parity.test_eigensolver_structured_matrices, plus exact multiplicities."""
    rng = np.random.default_rng(100 + n)
    rand = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    rand = (rand + rand.conj().T) / 2
    cases = {
        "diagonal": np.diag(rng.standard_normal(n)).astype(complex),
        "identity": np.eye(n, dtype=complex) * 0.75,
        "random": rand,
        "graded": rand * np.outer(10.0 ** -np.arange(n) / max(1, n // 8), np.ones(n)),
        "imag_offdiag": np.diag(np.arange(n, dtype=float)) + 1j * (np.eye(n, k=1) - np.eye(n, k=-1)),
        "tiny": rand * 1e-30,
        "huge": rand * 1e30,
    }
    cases["graded"] = (cases["graded"] + cases["graded"].conj().T) / 2
    if n >= 4:
        blk = np.zeros((n, n), dtype=complex)
        h = n // 2
        blk[:h, :h] = rand[:h, :h]
        blk[h:, h:] = rand[:n - h, :n - h]
        cases["two_equal_blocks"] = blk
        cases["rank_one"] = np.outer(rand[:, 0], rand[:, 0].conj())
        dup = rand.copy()
        for q in range(1, n - 1, 4):
            dup[q + 1, :] = dup[q, :]
            dup[:, q + 1] = dup[:, q]
        cases["duplicate_columns"] = (dup + dup.conj().T) / 2
    # exact multiplicities: Q diag(lambda with repeats) Q^H
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    lam = np.array([(-1.5, 0.25, 0.25, 2.0)[i % 4] for i in range(n)]) * np.repeat([1.0, 3.0], [n - n // 3, n // 3])
    mult = (q * lam) @ q.conj().T
    cases["multiplicities"] = (mult + mult.conj().T) / 2
    return cases


@pytest.mark.parametrize(
    "solver, n",
    [("auto", n) for n in (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)]
    + [("rocsolver", n) for n in (8, 40, 64, 65, 100, 129)],
)
def test_structured_matrices(solver, n):
    code = {"auto": _lib.TBK_EIG_AUTO, "rocsolver": _lib.TBK_EIG_ROCSOLVER}[solver]
    k = [[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]]
    for name, mat in _structured_cases(n).items():
        model = _onsite_model(mat)
        if not model.hop:  # all-zero matrices are dropped, like the reference
            continue
        model.set_option(_lib.TBK_OPT_EIGENSOLVER, code)
        E, U = model.eigh(k)
        ref = np.linalg.eigvalsh(mat)
        scale = np.abs(ref).max() if name in ("tiny", "huge") else max(1.0, np.abs(ref).max())
        err = np.abs(E - ref[None]).max()
        assert err <= 1e-12 * scale * n, (name, err)
        H = model.hamilton(k)
        try:
            _check_vectors(H, E, U, scale)
            for row in range(2):
                _cluster_projectors(H[row], E[row], U[row], scale)
        except AssertionError as exc:
            raise AssertionError("{}: {}".format(name, exc)) from exc


# ---- 3. call-shape independence of the Jacobi kernel -------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 24, 64])
def test_jacobi_result_does_not_depend_on_the_call_shape(n):
    rng = np.random.default_rng(7 + n)
    mat = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    mat = (mat + mat.conj().T) / 2
    model = _onsite_model(mat)
    first_e, first_u = model.eigh([0.3, 0.1, 0.2])
    _check_vectors(mat, first_e, first_u)
    for nk in (1, 2, 65, 5000):
        k = np.random.default_rng(nk).uniform(-1, 1, size=(nk, 3))
        E, U = model.eigh(k)
        assert np.array_equal(E, np.broadcast_to(first_e, E.shape)), nk
        assert np.array_equal(U, np.broadcast_to(first_u, U.shape)), nk


# ---- 4. seeded synthetic models ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [24, 64])
def test_seeded_dense_models(n):
    r_vec, hop, pos = syn.dense_model_arrays(n, 64, syn.MODEL_SEED + 40 + n)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    k_all = syn.random_kpoints(300, seed=n)
    for nk in (1, 3, 300):
        k = k_all[:nk]
        for convention in (1, 2):
            E, U = model.eigh(k, convention=convention)
            _check_vectors(model.hamilton(k, convention=convention), E, U)
            assert np.abs(E - model.eigenval_array(k)).max() <= 1e-12 * n * max(1.0, np.abs(E).max())
    # a call forced into several chunks gives the rows of the one-chunk call
    whole = model.eigh(k_all, convention=1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 128)
    E, U = model.eigh(k_all, convention=1)
    _check_vectors(model.hamilton(k_all, convention=1), E, U)
    assert np.abs(E - whole[0]).max() <= 1e-12 * n * max(1.0, np.abs(E).max())
    assert np.abs(oracle.hamilton(r_vec, hop, k_all[:4], 1, pos=pos) @ U[:4] - U[:4] * E[:4, None, :]).max() <= 1e-10


def test_seeded_csr_model():
    r_vec, r_ptr, row, col, val, pos = syn.csr_model_arrays(48, 32, syn.MODEL_SEED + 41, fill=0.05)
    hop = syn.csr_to_dense(48, r_ptr, row, col, val)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos, sparse=True)
    k = syn.random_kpoints(300, seed=5)
    for convention in (1, 2):
        E, U = model.eigh(k, convention=convention)
        _check_vectors(model.hamilton(k, convention=convention), E, U)
    assert np.abs(E - np.array(oracle.eigenval(r_vec, hop, k))).max() <= 1e-10


# ---- 5. Wilson loop ----------------------------------------------------------------------------------------------------
def _wilson_phases(vectors_of, pos, start, axis, n_occ=4, steps=48):
    """Eigenphases of prod_i U_occ(k_i)^H U_occ(k_{i+1}) on the closed string start + [0, 1] b_axis; the string closes with
    U(k + G) = diag(exp(-2 pi i G.pos)) U(k), the boundary condition of convention-1 eigenvectors."""
    g_vec = np.eye(3)[axis]
    ks = np.array([start + g_vec * i / steps for i in range(steps)])
    occ = vectors_of(ks)[:, :, :n_occ]
    closing = np.exp(-2j * np.pi * (pos @ g_vec))[:, None] * occ[0]
    prod = np.eye(n_occ, dtype=complex)
    for i in range(steps):
        nxt = occ[i + 1] if i + 1 < steps else closing
        prod = prod @ (occ[i].conj().T @ nxt)
    return np.linalg.eigvals(prod)


def test_wilson_loop_of_the_silicon_valence_bands(silicon_model):
    model, g = silicon_model
    pos = np.asarray(g["pos"])
    gpu = lambda ks: model.eigh(ks, convention=1)[1]
    cpu = lambda ks: np.linalg.eigh(oracle.hamilton(g["R"], g["hop"], ks, 1, pos=pos))[1]
    for start in (np.zeros(3), np.array([0.1, 0.25, -0.3]), np.array([0.37, -0.12, 0.05])):
        for axis in range(3):
            got, ref = _wilson_phases(gpu, pos, start, axis), _wilson_phases(cpu, pos, start, axis)
            # (the eigenvalues matched as sets: their phases agree mod 2 pi)
            assert np.abs(got[:, None] - ref[None, :]).min(axis=1).max() <= 1e-8, (start, axis)
            assert np.abs(ref[:, None] - got[None, :]).min(axis=1).max() <= 1e-8, (start, axis)


# ---- 6. k.p ------------------------------------------------------------------------------------------------------------
def test_kdotp_eigh():
    g = load_golden("kdotp")
    powers, coeffs, dk = g["order2_powers"], g["order2_coeffs"], g["order2_dk"]
    kp = tbmodels_amd.KdotpModel({tuple(p): c for p, c in zip(powers.tolist(), coeffs)})
    E, U = kp.eigh(dk)
    assert E.shape == (len(dk), 6) and U.shape == (len(dk), 6, 6)
    _check_vectors(kp.hamilton(dk), E, U)
    assert np.abs(E - kp.eigenval_array(dk)).max() <= 1e-12 * 6 * max(1.0, np.abs(E).max())
    e1, u1 = kp.eigh(dk[0])
    assert e1.shape == (6,) and u1.shape == (6, 6)
    _check_vectors(kp.hamilton(dk[0]), e1, u1)


# ---- 7. errors and edge cases ------------------------------------------------------------------------------------------
def test_eigh_errors_and_empty_lists(silicon_model):
    model, g = silicon_model
    bad = np.array(g["grid"][:10])
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        model.eigh(bad)
    E, U = model.eigh(g["known_kpoints"])  # the model is usable afterwards
    assert np.abs(E - g["known_eigenvals"]).max() <= 1e-10
    with pytest.raises(ValueError):
        model.eigh([[0.0, 0.0]])
    for empty in ([], np.zeros((0, 3))):
        E, U = model.eigh(empty)
        assert E.shape == (0, 8) and U.shape == (0, 8, 8)
    wide = _onsite_model(np.diag(np.arange(65, dtype=float)))
    wide.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_WAVE)
    with pytest.raises(ValueError):
        wide.eigh([0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        model.eigh([0.0, 0.0, np.inf], convention=1)
    nan_model = _onsite_model(np.array([[1.0, np.nan], [np.nan, 2.0]]))
    with pytest.raises(ValueError):
        nan_model.eigh([0.0, 0.0, 0.0])


# ---- 8. several devices, counters --------------------------------------------------------------------------------------
def test_device_list_and_library_counter(silicon_model):
    model, g = silicon_model
    k = np.array(g["grid"][:301])
    single = model.eigh(k, convention=1)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    both = twin.eigh(k, convention=1)
    assert len(twin._handles) == 2
    assert np.array_equal(both[0], single[0]) and np.array_equal(both[1], single[1])

    before = _counter(model, _lib.TBK_CNT_LIBRARY_CALLS)
    model.eigh(k[:5])
    assert _counter(model, _lib.TBK_CNT_LIBRARY_CALLS) == before
    model.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    try:
        E, U = model.eigh(k[:5], convention=1)
        assert _counter(model, _lib.TBK_CNT_LIBRARY_CALLS) == before + 1
        _check_vectors(model.hamilton(k[:5], convention=1), E, U)
    finally:
        model.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_AUTO)


def test_device_entry_overwrites_h_in_place(silicon_model):
    """tbk_eigh_device: H(k) built into d_U and replaced there by the eigenvectors; flags through tbk_eigenval_check."""
    import ctypes  # pylint: disable=import-outside-toplevel

    model, g = silicon_model
    lib = _lib.lib()
    k = np.ascontiguousarray(g["grid"][:200])
    handle = model._staged()
    bufs = []
    try:
        for nbytes in (k.nbytes, 200 * 8 * 8, 200 * 8 * 8 * 16):
            ptr = ctypes.c_void_p()
            _lib.check(lib.tbk_device_malloc(0, nbytes, ctypes.byref(ptr)))
            bufs.append(ptr)
        d_k, d_e, d_u = bufs
        _lib.check(lib.tbk_memcpy_h2d(0, d_k, _lib.ptr(k), k.nbytes))
        _lib.check(lib.tbk_eigh_device(handle, d_k, 200, 2, None, d_e, d_u))
        _lib.check(lib.tbk_eigenval_check(handle))
        E = np.empty((200, 8))
        U = np.empty((200, 8, 8), dtype=complex)
        _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(E), d_e, E.nbytes))
        _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(U), d_u, U.nbytes))
        host = model.eigh(k)
        assert np.array_equal(E, host[0]) and np.array_equal(U, host[1])
    finally:
        for ptr in bufs:
            lib.tbk_device_free(0, ptr)
