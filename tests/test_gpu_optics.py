"""
The optical conductivity on the GPU (csrc/tbk_optics.hip): the kernels against tools/optics_model.py
`conductivity` on identical (E, U, D), the derivative phase rows against the model's D^a, and `Model.optical_conductivity` against the
model fed with the eigensystem `Model.eigh` returns, against its properties and against `Model.berry_flux`.

Bound: optics_model.tolerance, per frequency and in either component -- derived from the number formats, NK, n, the
Frobenius norm of the velocity matrices, the bandwidth, |omega| and eta; nothing measured on the kernels enters it.  Identities of bits
(property 4: the lists, the passes, TBK_OPT_K_CHUNK, two handles, a second call; mu against `fermi_level`) are asserted as such.  Every
case prints its measured maximum.
"""

import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import berry_model  # noqa: E402  pylint: disable=wrong-import-position
import optics_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

MU = 0.1
TEMPERATURES = (0.05, 0.5)
ETAS = (0.05, 1e-3)
MESHES = ((3, 4), (2, 3, 2))
MIRROR = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 2])  # omega -> -omega in the list of _frequencies
_CACHE = {}


def _inputs(mesh, n):
    """Random ascending bands with a flat band 0 and an exactly degenerate pair (1, 2) inside every k-point (the construction of
    tests/test_gpu_chi_dynamic.py), a random unitary U, a random Hermitian D^a per axis and positions in the cell; shared by the cases
    and never written."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k, dim = int(np.prod(mesh)), len(mesh)
        rng = np.random.default_rng(9300 + 41 * n_k + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
        eig[:, 0] = -1.25 if n > 1 else 0.125
        if n >= 3:
            eig[:, 2] = eig[:, 1]
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        D = rng.normal(size=(n_k, dim, n, n)) + 1j * rng.normal(size=(n_k, dim, n, n))
        D = (D + D.conj().transpose(0, 1, 3, 2)) / 2.0
        pos = rng.uniform(0.0, 1.0, (n, dim))
        arrays = tuple(np.ascontiguousarray(a) for a in (eig, U.astype(np.complex128), D, pos))
        for array in arrays:
            array.setflags(write=False)
        _CACHE[key] = arrays
    return _CACHE[key]


def _frequencies(level):
    """0, +-0.2, +-0.7, +-one exact level difference (x = 0 for that pair), +-1e6, a duplicate of 0.2: ten, more than one register chunk."""
    level = float(level)
    return np.array([0.0, 0.2, -0.2, 0.7, -0.7, level, -level, 1e6, -1e6, 0.2])


def _from_eigensystem(eig, U, D, pos, T, omega, eta, mu=MU, part_bytes=0):
    n_k, dim, n = D.shape[0], D.shape[1], D.shape[2]
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    out = np.full((len(omega), dim, dim), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_optics_from_eigensystem(0, dim, n, n_k, _lib.ptr(eig), _lib.ptr(U), _lib.ptr(D), _lib.ptr(pos), float(mu), float(T),
                                                      len(omega), _lib.ptr(omega), float(eta), int(part_bytes), _lib.ptr(out)))
    return out


def _plan(n_k, n_orb, dim, n_w, part_bytes=0):
    out = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().tbk_optics_plan(n_k, n_orb, dim, n_w, part_bytes, out))
    return {"template": out[0], "chunk": out[1], "w_pass": out[2], "passes": out[3], "groups": out[4]}


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _worst(got, want, tol):
    gap = got - want
    return float(np.maximum(np.abs(gap.real), np.abs(gap.imag)).max()), bool(np.all(np.abs(gap.real) <= tol) and np.all(np.abs(gap.imag) <= tol))


def _tolerance(n_k, eig, D, pos, T, eta, omega, extra=0.0):
    norm = optics_model.velocity_norm(D, eig, pos)
    spread = 2.0 * float(np.ptp(eig)) + np.abs(omega)
    return optics_model.tolerance(n_k, eig.shape[-1], T, eta, spread, norm, 2 if pos is None else 3, extra)[:, None, None]


def _properties(sigma, tol, where):
    """Properties 1 and 2 within the bound: sigma(-omega) = conj sigma(omega); the Hermitian part over (a, c) is positive semidefinite."""
    err, ok = _worst(sigma[MIRROR], np.conj(sigma), tol)
    assert ok, where + ("conjugation", err)
    lowest = min(float(np.linalg.eigvalsh((s + s.conj().T) / 2.0).min()) + 2.0 * float(t.max()) * s.shape[0] for s, t in zip(sigma, tol))
    assert lowest >= 0.0, where + ("the Hermitian part has a negative eigenvalue", lowest)
    return err


# ---- 1. the kernels against the model on the same (E, U, D) ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 33, 64, 65, 80])
def test_kernels_match_the_model(n):
    for mesh in MESHES:
        n_k, dim = int(np.prod(mesh)), len(mesh)
        plan = _plan(n_k, n, dim, 10)
        assert plan["template"] == (16 if n <= 16 else 32 if n <= 32 else 64 if n <= 64 else 0) and plan["groups"] == 1
        assert (plan["w_pass"], plan["passes"]) == (10, 1) and 2 <= plan["chunk"] < 10
        eig, U, D, positions = _inputs(mesh, n)
        omega = _frequencies(eig[0, n - 1] - eig[0, 0])
        order = np.random.default_rng(10).permutation(len(omega))
        for pos in (None, positions):
            for T in TEMPERATURES:
                for eta in ETAS:
                    where = (mesh, n, pos is not None, T, eta)
                    want = optics_model.conductivity(eig, U, D, MU, T, omega, eta, pos)
                    got = _from_eigensystem(eig, U, D, pos, T, omega, eta)
                    tol = _tolerance(n_k, eig, D, pos, T, eta, omega)
                    err, inside = _worst(got, want, tol)
                    print("mesh %s n = %d positions %s T = %g eta = %g: max|sigma - model| = %.3e (bound %.3e - %.3e), max|sigma| = %.3e"
                          % (mesh, n, pos is not None, T, eta, err, tol.min(), tol.max(), np.abs(got).max()))
                    assert np.all(np.isfinite(_bits(got))) and inside, where + (err,)
                    _properties(got, tol, where)
                    # property 4 on the kernels: a duplicate; at the sharper pair of (T, eta) a second call, a permuted and a thinned list
                    assert _same(got[1], got[9]), where + ("a duplicate differs",)
                    if (T, eta) != (TEMPERATURES[0], ETAS[1]):
                        continue
                    assert _same(got, _from_eigensystem(eig, U, D, pos, T, omega, eta)), where + ("two calls differ",)
                    assert _same(got[order], _from_eigensystem(eig, U, D, pos, T, omega[order], eta)), where + ("the order changed bits",)
                    assert _same(got[[5, 8]], _from_eigensystem(eig, U, D, pos, T, omega[[5, 8]], eta)), where + ("the rest of the list changed bits",)
        # (once per n: the partials of plan["chunk"] + 1 frequencies fit, so ten go in whole register chunks and more than one pass)
        room = (plan["chunk"] + 1) * 16 * dim * dim * n_k + 7
        forced = _plan(n_k, n, dim, 10, room)
        assert forced["w_pass"] == plan["chunk"] and forced["passes"] == -(-10 // plan["chunk"]) >= 2
        whole = _from_eigensystem(eig, U, D, positions, 0.05, omega, 1e-3)
        assert _same(whole, _from_eigensystem(eig, U, D, positions, 0.05, omega, 1e-3, part_bytes=room)), (mesh, n, "the passes changed bits")


def test_extreme_chemical_potentials_give_plus_zero():
    for mesh, n in (((2, 3, 2), 17), ((3, 4), 3), ((3, 4), 65)):
        eig, U, D, positions = _inputs(mesh, n)
        omega = _frequencies(eig[0, n - 1] - eig[0, 0])
        for T in TEMPERATURES:
            for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # property 3: every f (or every 1 - f) is 0
                for pos in (None, positions):
                    flat = _bits(_from_eigensystem(eig, U, D, pos, T, omega, 1e-3, mu=mu))
                    assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (mesh, n, T, mu)


# ---- 2. the derivative phase rows ------------------------------------------------------------------------------------------------------
def _derivative_device(model, k, axis):
    """D^a through tbk_hamilton_derivative_device."""
    lib = _lib.lib()
    k = np.ascontiguousarray(k, dtype=np.float64)
    n = model.size
    out = np.full((len(k), n, n), np.nan + 1j * np.nan, dtype=np.complex128)
    ptrs = []
    try:
        for nbytes in (k.nbytes, out.nbytes):
            p = ctypes.c_void_p()
            _lib.check(lib.tbk_device_malloc(model.device, nbytes, ctypes.byref(p)))
            ptrs.append(p)
        d_k, d_d = ptrs
        _lib.check(lib.tbk_memcpy_h2d(model.device, d_k, _lib.ptr(k), k.nbytes))
        _lib.check(lib.tbk_hamilton_derivative_device(model._staged(), d_k, len(k), axis, d_d))
        _lib.check(lib.tbk_synchronize(model._staged()))
        _lib.check(lib.tbk_memcpy_d2h(model.device, _lib.ptr(out), d_d, out.nbytes))
    finally:
        for p in ptrs:
            _lib.check(lib.tbk_device_free(model.device, p))
    return out


def _derivative_case(name, model, r_vec, hop, counts):
    dim = r_vec.shape[1]
    weights = np.sqrt((np.abs(hop) ** 2).sum(axis=(1, 2)))  # ||hop[R]||_F
    for nk in counts:
        k = syn.random_kpoints(nk, dim=dim, seed=77 + nk) * 3.0 - 1.0  # (outside [0, 1) too: the argument reduction)
        for axis in range(dim):
            bound = 1e-13 * float((np.abs(r_vec[:, axis]) * weights).sum())
            got = _derivative_device(model, k, axis)
            want = optics_model.derivative(r_vec, hop, k, axis)
            err = float(np.abs(got - want).max())
            print("%s nk = %d axis %d: max|D - model| = %.3e (bound %.3e)" % (name, nk, axis, err, bound))
            assert np.all(np.isfinite(_bits(got))) and err <= bound, (name, nk, axis, err)
            diagonal = np.einsum("kii->ki", got).imag
            assert np.all(diagonal == 0.0), (name, nk, axis, "a diagonal element has an imaginary part")
            assert np.array_equal(got, got.conj().transpose(0, 2, 1)), (name, nk, axis, "not Hermitian bit for bit")


def test_derivative_rows_silicon():
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    _derivative_case("silicon", model, np.asarray(g["R"]), np.asarray(g["hop"]), (1, 3, 33, 200))


def test_derivative_rows_dense_64_on_every_path():
    """The paths of tbk_hk_plan for 64 orbitals (2048 packed slots: 32 element tiles per tile of 128 k-points).  64 lattice vectors are
    8 K stages of 16 rows: 1 and 3 points take the matrix-vector kernel, 33 and 200 the tiles unsplit (splitting needs 16 stages).  256
    lattice vectors are 32 stages: 33 and 200 points are 32 and 64 tiles, fewer than two per compute unit, so the tiles are split along K
    (8 ways) and the partial tiles are added by the finishing kernel."""
    r_vec, hop, pos = syn.dense_model_arrays(64, 64, syn.MODEL_SEED + 1900)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    _derivative_case("dense 64 x 64", model, r_vec, hop, (1, 3, 33, 200))
    r_vec, hop, pos = syn.dense_model_arrays(64, 256, syn.MODEL_SEED + 1901)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    _derivative_case("dense 64 x 256 (split-K)", model, r_vec, hop, (33, 200))


def test_derivative_rows_sparse_40():
    r_vec, r_ptr, row, col, val, pos = syn.csr_model_arrays(40, 64, syn.MODEL_SEED + 1903)
    hop = syn.csr_to_dense(40, r_ptr, row, col, val)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos, sparse=True)
    _derivative_case("CSR 40", model, r_vec, hop, (1, 3, 33, 200))


def test_derivative_rows_argument_errors():
    lib = _lib.lib()
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"])
    handle = model._staged()
    p = ctypes.c_void_p()
    _lib.check(lib.tbk_device_malloc(0, 4096, ctypes.byref(p)))
    try:
        bad = [lib.tbk_hamilton_derivative_device(None, p, 1, 0, p), lib.tbk_hamilton_derivative_device(handle, p, 1, -1, p),
               lib.tbk_hamilton_derivative_device(handle, p, 1, 3, p), lib.tbk_hamilton_derivative_device(handle, p, -1, 0, p),
               lib.tbk_hamilton_derivative_device(handle, None, 1, 0, p), lib.tbk_hamilton_derivative_device(handle, p, 1, 0, None)]
        assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
        assert lib.tbk_hamilton_derivative_device(handle, p, 0, 0, p) == _lib.TBK_OK
    finally:
        _lib.check(lib.tbk_device_free(0, p))


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------
def _silicon(sparse=False):
    """The model and the hoppings it holds (the constructor folds positions into the home cell, which moves lattice vectors: the
    reference takes the model's own, read before a sparse twin stores them as CSR)."""
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    r_vec, hop = model.packed_hop()
    if sparse:
        model.set_sparse()
    return model, r_vec.astype(np.int64), hop


def _qwz(u):
    pos = [[0.1, 0.2], [0.3, 0.85]]
    model = tbmodels_amd.Model(hop=berry_model.qwz_hoppings(u), size=2, dim=2, pos=pos, uc=[[1.5, 0.0], [0.5, 2.0]], contains_cc=False)
    r_vec, hop = model.packed_hop()
    return model, r_vec.astype(np.int64), hop


def _derivative_rounding(r_vec, hop, norm):
    """`extra` of the bound: the derivative rows' own rounding, 1e-13 sum_R |R_a| ||hop[R]|| per element at most (the bound of section 2
    of this file), as a Frobenius norm over G in units of u."""
    weights = np.sqrt((np.abs(hop) ** 2).sum(axis=(1, 2)))
    worst = max(float((np.abs(r_vec[:, a]) * weights).sum()) for a in range(r_vec.shape[1]))
    return 1e-13 * worst * hop.shape[1] / norm / 2.0 ** -53


CALLS = {"silicon": (lambda: _silicon(), (3, 4, 2), 4.5), "QWZ": (lambda: _qwz(1.0), (5, 7), 1.2)}


@pytest.mark.parametrize("name", list(CALLS))
def test_properties_of_a_whole_call(name):
    make, mesh, n_el = CALLS[name]
    model, r_vec, hop = make()
    n, n_k = model.size, int(np.prod(mesh))
    kpts = optics_model.mesh_kpoints(mesh)
    eig, vec = model.eigh(kpts)
    D = optics_model.derivatives(r_vec, hop, kpts)
    level = model.fermi_level(mesh, n_el)
    omega = _frequencies(eig[0, n - 1] - eig[0, 0])
    positions = np.asarray(model.pos, dtype=float)
    for T in TEMPERATURES:
        for eta in ETAS:
            for convention, pos in ((2, None), (1, positions)):
                where = (name, T, eta, convention)
                result = model.optical_conductivity(mesh, omega, eta=eta, temperature=T, n_electrons=n_el, convention=convention)
                assert isinstance(result, tbmodels_amd.OpticalConductivity) and result.mu == level  # bit for bit
                assert result.omega.dtype == np.float64 and np.array_equal(result.omega, omega)
                sigma = result.sigma
                assert sigma.shape == (len(omega), len(mesh), len(mesh)) and sigma.dtype == np.complex128 and np.all(np.isfinite(_bits(sigma)))
                norm = optics_model.velocity_norm(D, eig, pos)
                tol = _tolerance(n_k, eig, D, pos, T, eta, omega, _derivative_rounding(r_vec, hop, norm))
                err, inside = _worst(sigma, optics_model.conductivity(eig, vec, D, level.mu, T, omega, eta, pos), tol)
                mirror = _properties(sigma, tol, where)
                assert _same(sigma[1], sigma[9]), where + ("a duplicate differs",)
                print("%s %s convention %d T = %g eta = %g: max|sigma - model| = %.3e (bound %.3e - %.3e), conjugation %.3e, min Re sigma_aa = %.3e"
                      % (name, mesh, convention, T, eta, err, tol.min(), tol.max(), mirror, min(sigma[:, a, a].real.min() for a in range(len(mesh)))))
                assert inside, where + (err,)
    edges = model.band_edges(mesh)
    for mu in (float(edges.emin.min()) - 746.0 * 0.05, float(edges.emax.max()) + 746.0 * 0.05):  # property 3
        for convention in (1, 2):
            far = model.optical_conductivity(mesh, omega, eta=1e-3, temperature=0.05, energy=mu, convention=convention)
            assert far.mu.mu == mu and np.all(_bits(far.sigma) == 0.0) and not np.any(np.signbit(_bits(far.sigma)))
    one = model.optical_conductivity(mesh, 0.2, eta=0.05, temperature=0.05, n_electrons=n_el)  # one number
    assert one.sigma.shape == (1, len(mesh), len(mesh)) and one.omega.shape == (1,)
    assert _same(one.sigma[0], model.optical_conductivity(mesh, omega, eta=0.05, temperature=0.05, n_electrons=n_el).sigma[1])
    # cartesian=True is the host transform of the reduced result
    reduced = model.optical_conductivity(mesh, omega, eta=0.05, temperature=0.05, n_electrons=n_el, convention=1)
    moved = model.optical_conductivity(mesh, omega, eta=0.05, temperature=0.05, n_electrons=n_el, convention=1, cartesian=True)
    assert moved.mu == reduced.mu and np.allclose(moved.sigma, optics_model.cartesian(reduced.sigma, model.uc), rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("u_par, want", [(-1.0, -1), (1.0, 1), (3.0, 0)])
def test_qwz_hall_conductivity_against_berry_flux(u_par, want):
    """Property 5 with the CPU test's tolerance: 2e-3, five times the formula's own discretisation error on 12 x 12."""
    model, _, _ = _qwz(u_par)
    mesh = (12, 12)
    chern = int(model.berry_flux(mesh, 1).chern[0][0, 0])
    sigma = model.optical_conductivity(mesh, [0.0], eta=0.05, temperature=0.02, energy=0.0).sigma[0]
    hall = 2.0 * np.pi * sigma[0, 1].real
    print("QWZ u = %+g on 12 x 12: 2 pi sigma_xy(0) = %+.6f, berry_flux C = %+d, deviation %.2e" % (u_par, hall, chern, abs(hall - chern)))
    assert chern == want and abs(hall - chern) <= 2e-3


def test_a_sparse_model_against_its_dense_twin():
    dense, r_vec, hop = _silicon()
    sparse, _, _ = _silicon(True)
    mesh, n_k = (3, 4, 2), 24
    kpts = optics_model.mesh_kpoints(mesh)
    eig, _ = dense.eigh(kpts)
    D = optics_model.derivatives(r_vec, hop, kpts)
    omega = _frequencies(eig[0, -1] - eig[0, 0])
    positions = np.asarray(dense.pos, dtype=float)
    for convention, pos in ((2, None), (1, positions)):
        args = dict(eta=0.05, temperature=0.05, n_electrons=4.5, convention=convention)
        one, two = dense.optical_conductivity(mesh, omega, **args), sparse.optical_conductivity(mesh, omega, **args)
        norm = optics_model.velocity_norm(D, eig, pos)
        # (the bound as it stands; eigenvectors inside the degenerate clusters of silicon may differ between the two, which sigma does
        # not see)
        tol = _tolerance(n_k, eig, D, pos, 0.05, 0.05, omega, _derivative_rounding(r_vec, hop, norm))
        err, inside = _worst(two.sigma, one.sigma, tol)
        print("silicon CSR against dense, convention %d: max|difference| = %.3e (bound %.3e)" % (convention, err, tol.min()))
        assert two.mu.mu == pytest.approx(one.mu.mu, abs=1e-12) and inside


# ---- 4. identities of bits (property 4) ------------------------------------------------------------------------------------------------
def _three_orbital_model():
    r_vec, hop, pos = syn.dense_model_arrays(3, 6, syn.MODEL_SEED + 1910, dim=2)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def test_bits_do_not_depend_on_chunk_handles_lists_passes_or_the_call():
    """20 x 15 = 300 points: two summation groups, and two handles are cut at point 256."""
    mesh = (20, 15)
    model = _three_orbital_model()
    omega = np.array([0.0, 0.4, -0.4, 2.5, 0.4, -7.0, 1e6, 0.01, 0.02])
    assert _plan(300, 3, 2, len(omega))["groups"] == 2
    for convention in (2, 1):
        args = dict(eta=1e-3, temperature=0.05, n_electrons=1.3, convention=convention)
        base = model.optical_conductivity(mesh, omega, **args)
        assert _same(base.sigma, model.optical_conductivity(mesh, omega, **args).sigma), "a second call differs"
        assert _same(base.sigma[1], base.sigma[4]), "a duplicate differs"
        order = np.random.default_rng(3).permutation(len(omega))
        assert _same(base.sigma[order], model.optical_conductivity(mesh, omega[order], **args).sigma), "the order changed bits"
        assert _same(base.sigma[[3, 6]], model.optical_conductivity(mesh, omega[[3, 6]], **args).sigma), "the rest of the list changed bits"
        model.set_option(_lib.TBK_OPT_K_CHUNK, 7)
        chunked = model.optical_conductivity(mesh, omega, **args)
        model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
        assert chunked.mu == base.mu and _same(base.sigma, chunked.sigma), ("TBK_OPT_K_CHUNK changed bits", np.abs(base.sigma - chunked.sigma).max())
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        two = twin.optical_conductivity(mesh, omega, **args)
        assert len(twin._handles) == 2 and two.mu == base.mu
        assert _same(base.sigma, two.sigma), ("two handles changed bits", np.abs(base.sigma - two.sigma).max())
        # two passes through part_bytes at the C interface: room for five frequencies' partials, four (a whole register chunk) per pass
        mesh32 = np.array(mesh, dtype=np.int32)
        pos = np.ascontiguousarray(model.pos, dtype=np.float64)
        room = 5 * 16 * 4 * 300
        assert (lambda p: (p["w_pass"], p["passes"]))(_plan(300, 3, 2, len(omega), room)) == (4, 3)
        for handles, count in ((model._handle_array()), (twin._handle_array())):
            mu, sigma = np.zeros(4), np.zeros((len(omega), 2, 2), dtype=np.complex128)
            _lib.check(_lib.lib().tbk_optical_conductivity_multi(handles, count, _lib.ptr(mesh32), 1, 1.3, 0.05, len(omega), _lib.ptr(omega), 1e-3, convention,
                                                                 _lib.ptr(pos), room, _lib.ptr(mu), _lib.ptr(sigma)))
            assert mu[0] == base.mu.mu and _same(base.sigma, sigma), ("the passes changed bits", count)


# ---- 5. timing and the C interface ------------------------------------------------------------------------------------------------------
def test_calls_are_booked_on_their_own_row():
    model, _, _ = _silicon()
    omega = np.array([0.0, 3.0, 6.5])
    args = dict(eta=0.1, temperature=0.1, n_electrons=4.5)
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_optics_timing(model._staged(), ms, ctypes.byref(calls), 1))
    plain = model.optical_conductivity((4, 4, 4), omega, **args)  # TBK_OPT_TIMING is off
    _lib.check(_lib.lib().tbk_optics_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    timed = model.optical_conductivity((4, 4, 4), omega, **args)
    _lib.check(_lib.lib().tbk_optics_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 3 frequencies: %d calls, derivative H(k) %.3f ms, rotation + epilogue %.3f ms, reductions %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0 and _same(timed.sigma, plain.sigma)
    _lib.check(_lib.lib().tbk_optics_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 0 and list(ms) == [0.0, 0.0, 0.0]


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U, D, pos = _inputs((2, 3, 2), 3)
    omega = np.array([0.0, 0.5, -0.5])
    out, four = np.zeros((3, 3, 3), dtype=np.complex128), np.zeros(4)
    nan, inf = float("nan"), float("inf")
    with_nan, with_inf = np.array([0.0, nan, 0.5]), np.array([0.0, 0.5, -inf])

    def call(dim=3, n_orb=3, nk=12, eig_=eig, U_=U, D_=D, pos_=None, mu=0.0, T=0.1, n_w=3, omega_=omega, eta=0.05, room=0, out_=out):
        return lib.tbk_optics_from_eigensystem(0, dim, n_orb, nk, _lib.ptr(eig_), _lib.ptr(U_), _lib.ptr(D_), _lib.ptr(pos_), mu, T, n_w, _lib.ptr(omega_), eta,
                                               room, _lib.ptr(out_))

    assert call() == _lib.TBK_OK and call(pos_=pos) == _lib.TBK_OK and call(n_w=1) == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(n_orb=0), call(nk=0), call(eig_=None), call(U_=None), call(D_=None), call(out_=None), call(mu=nan), call(mu=inf),
           call(T=0.0), call(T=-0.1), call(T=nan), call(T=inf), call(n_w=0), call(n_w=-1), call(n_w=2 ** 23 + 1), call(omega_=None), call(omega_=with_nan),
           call(omega_=with_inf), call(eta=0.0), call(eta=-0.05), call(eta=nan), call(eta=inf), call(eta=1e-200), call(room=-1)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    assert call(room=16 * 9 * 12 - 1) == _lib.TBK_ERR_MEMORY  # not one frequency fits
    model, _, _ = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    positions = np.ascontiguousarray(model.pos, dtype=np.float64)
    mesh, zero = np.array([2, 3, 2], dtype=np.int32), np.array([2, 0, 2], dtype=np.int32)
    plan = (ctypes.c_int64 * 5)()
    m32, pw, pp, p4, po = _lib.ptr(mesh), _lib.ptr(omega), _lib.ptr(positions), _lib.ptr(four), _lib.ptr(out)

    def whole(handle_=handle, mesh_=m32, mode=0, value=0.0, T=0.1, n_w=3, omega_=pw, eta=0.05, convention=2, pos_=pp, room=0, mu_=p4, out_=po):
        return lib.tbk_optical_conductivity(handle_, mesh_, mode, value, T, n_w, omega_, eta, convention, pos_, room, mu_, out_)

    assert whole() == _lib.TBK_OK and whole(convention=1) == _lib.TBK_OK and whole(pos_=None) == _lib.TBK_OK
    bad = [whole(handle_=None), whole(mesh_=None), whole(mode=2), whole(value=inf), whole(mode=1, value=0.0), whole(mode=1, value=8.0),
           whole(mode=1, value=nan), whole(T=0.0), whole(T=-1.0), whole(T=nan), whole(T=inf), whole(convention=0), whole(convention=3),
           whole(convention=1, pos_=None), whole(mu_=None), whole(out_=None), whole(mesh_=_lib.ptr(zero)), whole(n_w=0), whole(n_w=2 ** 23 + 1),
           whole(omega_=None), whole(omega_=_lib.ptr(with_nan)), whole(omega_=_lib.ptr(with_inf)), whole(eta=0.0), whole(eta=-1.0), whole(eta=nan),
           whole(eta=inf), whole(room=-1),
           lib.tbk_optical_conductivity_multi(twice, 2, m32, 1, 4.0, 0.1, 3, pw, 0.05, 2, pp, 0, p4, po),
           lib.tbk_optical_conductivity_multi(None, 1, m32, 1, 4.0, 0.1, 3, pw, 0.05, 2, pp, 0, p4, po),
           lib.tbk_optics_plan(0, 8, 3, 3, 0, plan), lib.tbk_optics_plan(64, 0, 3, 3, 0, plan), lib.tbk_optics_plan(64, 8, 1, 3, 0, plan),
           lib.tbk_optics_plan(64, 8, 4, 3, 0, plan), lib.tbk_optics_plan(64, 8, 3, 0, 0, plan), lib.tbk_optics_plan(64, 8, 3, 2 ** 23 + 1, 0, plan),
           lib.tbk_optics_plan(64, 8, 3, 3, -1, plan), lib.tbk_optics_plan(64, 8, 3, 3, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    assert whole(room=16 * 9 * 12 - 1) == _lib.TBK_ERR_MEMORY


def test_a_small_model_on_a_long_mesh_stays_on_one_h_of_k_arithmetic():
    """17^3 = 4913 points of silicon: a chunk of the whole mesh would take the H(k) tiles and shorter ones the matrix-vector kernel; the
    walk stays at 4096 points at most, so TBK_OPT_K_CHUNK above, at and below that and two handles give the same bits."""
    model, _, _ = _silicon()
    mesh, omega = (17, 17, 17), np.array([0.0, 1.5, 4.0])
    args = dict(eta=0.05, temperature=0.05, n_electrons=4.0, convention=1)
    base = model.optical_conductivity(mesh, omega, **args)
    for chunk in (5000, 4096, 1000):
        model.set_option(_lib.TBK_OPT_K_CHUNK, chunk)
        got = model.optical_conductivity(mesh, omega, **args)
        assert got.mu == base.mu and _same(base.sigma, got.sigma), (chunk, np.abs(base.sigma - got.sigma).max())
    model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.optical_conductivity(mesh, omega, **args)
    assert two.mu == base.mu and _same(base.sigma, two.sigma), np.abs(base.sigma - two.sigma).max()
