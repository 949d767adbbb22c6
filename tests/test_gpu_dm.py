"""
The phase-table, projector and Fourier kernels (csrc/tbk_dm.hip) against tools/dm_model.py on identical (w, U), and
`Model.density_matrix` against its properties and against host-side projectors of the same mesh.

Bound of the kernels: every element of rho is a sum of NK n_orb terms whose moduli add up to at most 1 (Cauchy-Schwarz on the unit
rows of U), so tol_rho = 4 (NK n_orb + 32) 2^-53 covers the roundings of both sides and of the complex multiply.
The properties of a whole call (rho(-R) = rho(R)^H, the inverse transform over the dual cell, above the spectrum) take the same
tol_rho; one handle against two takes 2 tol_rho.  The silicon gap case against the valence projector built on the host from
`Model.eigh`: 1e-9, the whole-call bound of DESIGN 13.5.  The band energy: tol_rho on every element times 2 sum |hop|, plus 1e-12
sum |band_energy| -- rho and `occupations().band_energy` come from the same device eigensystem and the same weights.  Every case
prints its measured maximum.
"""

import ctypes
import itertools
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
import dm_model  # noqa: E402  pylint: disable=wrong-import-position
import dos_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

_CACHE = {}


def tol_rho(n_k, n_orb):
    return 4.0 * (n_k * n_orb + 32) * 2.0 ** -53


def _eigensystem(mesh, n):
    """Random ascending bands (the lowest one full at mu = 0.1) and random unitary U, shared by the cases and never written."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(4100 + 37 * n_k + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, tuple(mesh) + (n,)), axis=-1)
        eig[..., 0] -= 2.0
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
        w = np.full(eig.shape, np.nan)  # the kernel's own weights: both sides contract the same numbers
        _lib.check(_lib.lib().tbk_tetra_weights_from_eigenvalues(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), 0.1, _lib.ptr(w)))
        for array in (eig, U, w):
            array.setflags(write=False)
        _CACHE[key] = (eig, U, w)
    return _CACHE[key]


def _vectors(mesh, n_r, seed):
    """n_r vectors from {-3 .. 3}^dim; from three on, the last two are the first one shifted by whole mesh periods and a duplicate
    of the second (of the first when there is no second)."""
    dim = len(mesh)
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, size=(max(1, n_r - 2), dim)).astype(np.int64)
    if n_r < 3:
        return base[:n_r], None, None
    shift = np.array([(-1) ** d * (d + 1) * mesh[d] for d in range(dim)], dtype=np.int64)
    twin = min(1, len(base) - 1)
    R = np.concatenate([base, (base[0] + shift)[None, :], base[twin][None, :]])
    return np.ascontiguousarray(R), (0, n_r - 2), (twin, n_r - 1)


def _from_eigensystem(mesh, eig, U, R, k_chunk, energy=0.1):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    R = np.ascontiguousarray(R, dtype=np.int64)
    out = np.full((len(R), n, n), np.nan + 0j, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_density_matrix_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), float(energy),
                                                              k_chunk, len(R), _lib.ptr(R), _lib.ptr(out)))
    return out


def _plan(rows, n_orb, n_r):
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.lib().tbk_dm_plan(rows, n_orb, n_r, out))
    return {"nr_pad": out[0], "slices": out[1], "kps": out[2]}


def _kernel_case(mesh, n, n_r, chunks=(0, 5, 1)):
    eig, U, w = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    R, shifted, duplicate = _vectors(mesh, n_r, 5200 + n_r)
    want = dm_model.density_matrix(w, U, mesh, R)
    bound, worst = tol_rho(n_k, n), 0.0
    for chunk in chunks:
        got = _from_eigensystem(mesh, eig, U, R, chunk)
        err = np.abs(got - want).max()
        worst = max(worst, err)
        assert np.all(np.isfinite(got.view(float))) and err <= bound, (mesh, n, n_r, chunk, err, bound)
        if shifted:
            assert np.array_equal(got[shifted[0]], got[shifted[1]]), (mesh, n, n_r, chunk, "a whole mesh period changed bits")
            assert np.array_equal(got[duplicate[0]], got[duplicate[1]]), (mesh, n, n_r, chunk, "a duplicate differs")
        if chunk == chunks[0]:
            assert np.array_equal(got, _from_eigensystem(mesh, eig, U, R, chunk)), (mesh, n, n_r, "two calls differ")
    return worst, bound


# ---- 1. the kernels against the model on the same (w, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 17, 33, 65])
def test_kernels_match_the_model_on_2x3x2(n):
    mesh = (2, 3, 2)
    assert _plan(12, n, 33)["slices"] == 1  # twelve points: one slice
    for n_r in (1, 5, 16, 17, 33):
        worst, bound = _kernel_case(mesh, n, n_r)
        print("mesh %s n = %d NR = %d: max|rho - model| = %.3e (bound %.3e)" % (mesh, n, n_r, worst, bound))


@pytest.mark.parametrize("mesh", [(3, 4), (1, 5)])
def test_kernels_match_the_model_in_two_dimensions(mesh):
    worst, bound = _kernel_case(mesh, 9, 17)
    print("mesh %s n = 9 NR = 17: max|rho - model| = %.3e (bound %.3e)" % (mesh, worst, bound))


def test_sliced_contraction_matches_the_model():
    mesh, n, n_r = (4, 4, 4), 8, 33
    plan = _plan(64, n, n_r)
    print("plan of 64 points, 8 orbitals, 33 vectors:", plan)
    assert plan["slices"] > 1 and plan["kps"] % 4 == 0 and plan["slices"] * plan["kps"] >= 64 and plan["nr_pad"] == 48
    worst, bound = _kernel_case(mesh, n, n_r, chunks=(0, 5, 1, 24))  # 5 and 24: chunks that end inside a slice and inside a group
    print("mesh %s n = %d NR = %d, %d slices: max|rho - model| = %.3e (bound %.3e)" % (mesh, n, n_r, plan["slices"], worst, bound))


def test_phase_reduction_near_the_ends_of_the_integers():
    mesh, n = (2, 3, 2), 3
    eig, U, _ = _eigensystem(mesh, n)
    R = np.array([[1, -2, 3], [1 + 2 * 2 ** 30, -2 - 3 * (2 ** 31 // 3), 3 + 2 * (2 ** 30 - 1)], [1 - 2 * 2 ** 30, -2, 3 - 2 ** 31],
                  [1 + 2 * 2 ** 61, -2 - 3 * 2 ** 61, 3], [1 - 2 ** 63, -2, 3]], dtype=np.int64)
    assert np.array_equal(np.mod(R, np.array(mesh)), np.mod(R[:1], np.array(mesh)).repeat(len(R), axis=0))  # all congruent
    got = _from_eigensystem(mesh, eig, U, R, 0)
    for other in got[1:]:
        assert np.array_equal(got[0], other)


# ---- 2. whole calls ------------------------------------------------------------------------------------------------------------------
def _silicon():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])


def _dense9(dim):
    r_vec, hop, pos = syn.dense_model_arrays(9, 6, syn.MODEL_SEED + 1400 + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def test_silicon_gap_case_is_the_valence_projector():
    model, mesh, m = _silicon(), (2, 3, 2), 4
    n, n_k = model.size, 12
    level = model.fermi_level(mesh, m)
    assert level.lower < level.upper
    result = model.density_matrix(mesh, n_electrons=m)
    assert isinstance(result, tbmodels_amd.DensityMatrix) and isinstance(result.mu, tbmodels_amd._model.FermiLevel)
    assert result.mu == level  # bit for bit
    r_vec, _ = model.packed_hop()
    assert result.R.dtype == np.int64 and np.array_equal(result.R, r_vec) and result.rho.shape == (len(r_vec), n, n)
    vec = model.eigh(dos_model.mesh_kpoints(mesh))[1]
    w = np.zeros((n_k, n))
    w[:, :m] = 1.0 / n_k
    want = dm_model.density_matrix(w, vec, mesh, result.R)
    err = np.abs(result.rho - want).max()
    print("silicon %s, 4 electrons, %d vectors: max|rho - valence projector| = %.3e" % (mesh, len(r_vec), err))
    assert err <= 1e-9
    origin = model.density_matrix(mesh, n_electrons=m, R=(0, 0, 0))  # one vector
    assert origin.rho.shape == (1, n, n) and origin.R.shape == (1, 3)
    occ = model.occupations(mesh, n_electrons=m)
    err_q = np.abs(np.diagonal(origin.rho[0]).real - occ.orbital_occ).max()
    print("silicon: max|diag rho(0) - orbital_occ| = %.3e, |tr rho(0) - N| = %.3e" % (err_q, abs(np.trace(origin.rho[0]).real - level.nos)))
    assert err_q <= n * 2.0 ** -40 + tol_rho(n_k, n)
    assert np.abs(np.diagonal(origin.rho[0]).imag).max() <= tol_rho(n_k, n)


@pytest.mark.parametrize("dim, mesh", [(3, (2, 3, 2)), (2, (3, 4))])
def test_properties_of_a_metallic_call(dim, mesh):
    model, n_el = _dense9(dim), 3.1
    n, n_k = model.size, int(np.prod(mesh))
    tol = tol_rho(n_k, n)
    # property 1 and 2: the whole dual cell and the negated vectors in one call
    cell = np.array(list(itertools.product(*[range(x) for x in mesh])), dtype=np.int64)
    both = model.density_matrix(mesh, n_electrons=n_el, R=np.concatenate([cell, -cell]))
    assert both.mu == model.fermi_level(mesh, n_el)
    rho, minus = both.rho[:n_k], both.rho[n_k:]
    err_1 = np.abs(minus - np.conj(np.transpose(rho, (0, 2, 1)))).max()
    print("dense 9 %s: max|rho(-R) - rho(R)^H| = %.3e (bound %.3e)" % (mesh, err_1, tol))
    assert err_1 <= tol
    occ = model.occupations(mesh, n_electrons=n_el)
    assert np.abs(np.diagonal(rho[0]).real - occ.orbital_occ).max() <= n * 2.0 ** -40 + tol
    assert abs(np.trace(rho[0]).real - both.mu.nos) <= n * 2.0 ** -40 + tol
    kpts = dos_model.mesh_kpoints(mesh)
    vec = model.eigh(kpts)[1]
    P = dm_model.projectors(model.tetra_weights(mesh, both.mu.mu), vec)
    for index in (1, n_k - 1):
        back = np.einsum("r,rij->ij", np.exp(2j * np.pi * (cell @ kpts[index])), rho)
        err_2 = np.abs(back - n_k * P[index]).max()
        print("dense 9 %s: inverse transform at mesh point %d: %.3e (bound %.3e)" % (mesh, index, err_2, tol))
        assert err_2 <= tol
    # property 3: the stored half of the hoppings
    stored = model.density_matrix(mesh, n_electrons=n_el)
    r_vec, hop = model.packed_hop()
    assert np.array_equal(stored.R, r_vec)
    got, want = dm_model.band_energy(stored.rho, hop), occ.band_energy.sum()
    bound = tol * 2 * np.abs(hop).sum() + 1e-12 * np.abs(occ.band_energy).sum()
    print("dense 9 %s: band energy from rho %.15g, from occupations %.15g (bound %.3e)" % (mesh, got, want, bound))
    assert abs(got - want) <= bound


def test_above_and_below_the_spectrum():
    model, mesh = _dense9(3), (2, 3, 2)
    n, n_k = model.size, 12
    edges = model.band_edges(mesh)
    R = np.array([[0, 0, 0], [2, 3, -2], [1, 0, 0], [0, -1, 1], [4, 0, 0], [2, 3, 1]], dtype=np.int64)
    above = model.density_matrix(mesh, energy=float(edges.emax.max()) + 1.0, R=R).rho
    want = np.zeros((len(R), n, n), dtype=complex)
    want[[0, 1, 4]] = np.eye(n)  # R = 0 modulo the mesh
    err = np.abs(above - want).max()
    print("above the spectrum: max|rho - (identity or 0)| = %.3e (bound %.3e)" % (err, tol_rho(n_k, n)))
    assert err <= tol_rho(n_k, n)
    below = model.density_matrix(mesh, energy=float(edges.emin.min()) - 1.0, R=R).rho
    assert np.all(below == 0.0)


def test_csr_twin_and_two_handles():
    model, mesh, m = _silicon(), (2, 3, 2), 4
    tol = tol_rho(12, model.size)
    one = model.density_matrix(mesh, n_electrons=m)
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    csr = sparse.density_matrix(mesh, n_electrons=m)
    err = np.abs(csr.rho - one.rho).max()
    print("silicon, CSR against dense: %.3e (bound %.3e)" % (err, tol))
    assert err <= tol
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.density_matrix(mesh, n_electrons=m)
    assert len(twin._handles) == 2 and two.mu == one.mu
    err = np.abs(two.rho - one.rho).max()
    print("silicon, two handles against one: %.3e (bound %.3e)" % (err, 2 * tol))
    assert err <= 2 * tol
    metal, twin = _dense9(3), _dense9(3)
    twin.devices = [0, 0]
    a, b = metal.density_matrix(mesh, n_electrons=3.1), twin.density_matrix(mesh, n_electrons=3.1)
    err = np.abs(a.rho - b.rho).max()
    print("dense 9, two handles against one: %.3e (bound %.3e)" % (err, 2 * tol_rho(12, 9)))
    assert a.mu == b.mu and err <= 2 * tol_rho(12, 9)
    assert np.array_equal(a.rho, metal.density_matrix(mesh, n_electrons=3.1).rho)  # the same call again: the same bits


# ---- 3. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    model.density_matrix((4, 4, 4), n_electrons=4.5)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_dm_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    occ_ms, occ_calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_occ_timing(model._staged(), occ_ms, ctypes.byref(occ_calls), 0))
    assert occ_calls.value == 0  # the occupations family counts its own calls
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    model.density_matrix((4, 4, 4), n_electrons=4.5)
    _lib.check(_lib.lib().tbk_dm_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4): %d calls, phase table %.3f ms, projectors %.3f ms, contraction %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_dm_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 0 and list(ms) == [0.0, 0.0, 0.0]


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U, _ = _eigensystem((2, 3, 2), 9)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    zero = np.array([2, 0, 2], dtype=np.int32)
    R = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    rho, four = np.zeros((2, 9, 9), dtype=np.complex128), np.zeros(4)
    nan, inf = float("nan"), float("inf")

    def call(dim=3, mesh_=mesh, n_orb=9, eig_=eig, U_=U, energy=0.0, chunk=0, n_r=2, R_=R, out=rho):
        return lib.tbk_density_matrix_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), energy, chunk, n_r,
                                                       _lib.ptr(R_), _lib.ptr(out))

    assert call() == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=zero), call(mesh_=None), call(eig_=None), call(U_=None), call(R_=None), call(out=None),
           call(n_orb=0), call(energy=nan), call(energy=-inf), call(chunk=-1), call(n_r=0), call(n_r=-3)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 3)()
    rho8 = np.zeros((2, 8, 8), dtype=np.complex128)
    m32, pr, p4, po = _lib.ptr(mesh), _lib.ptr(R), _lib.ptr(four), _lib.ptr(rho8)
    bad = [lib.tbk_density_matrix(None, m32, 0, 0.0, 2, pr, p4, po), lib.tbk_density_matrix(handle, None, 0, 0.0, 2, pr, p4, po),
           lib.tbk_density_matrix(handle, m32, 2, 0.0, 2, pr, p4, po), lib.tbk_density_matrix(handle, m32, 0, inf, 2, pr, p4, po),
           lib.tbk_density_matrix(handle, m32, 1, 0.0, 2, pr, p4, po), lib.tbk_density_matrix(handle, m32, 1, 8.0, 2, pr, p4, po),
           lib.tbk_density_matrix(handle, m32, 1, nan, 2, pr, p4, po), lib.tbk_density_matrix(handle, m32, 0, 0.0, 0, pr, p4, po),
           lib.tbk_density_matrix(handle, m32, 0, 0.0, 2, None, p4, po), lib.tbk_density_matrix(handle, m32, 0, 0.0, 2, pr, None, po),
           lib.tbk_density_matrix(handle, m32, 0, 0.0, 2, pr, p4, None), lib.tbk_density_matrix(handle, _lib.ptr(zero), 1, 4.0, 2, pr, p4, po),
           lib.tbk_density_matrix_multi(twice, 2, m32, 1, 4.0, 2, pr, p4, po), lib.tbk_density_matrix_multi(None, 1, m32, 1, 4.0, 2, pr, p4, po),
           lib.tbk_dm_timing(None, ms, ctypes.byref(calls), 0), lib.tbk_dm_timing(handle, None, ctypes.byref(calls), 0),
           lib.tbk_dm_timing(handle, ms, None, 0), lib.tbk_dm_plan(0, 8, 2, plan), lib.tbk_dm_plan(64, 0, 2, plan), lib.tbk_dm_plan(64, 8, 0, plan),
           lib.tbk_dm_plan(64, 8, 2, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
