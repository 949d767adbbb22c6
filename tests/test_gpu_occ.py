"""
The point-weight, band-sum and contraction kernels (csrc/tbk_occ.hip) against tools/occ_model.py on identical inputs, and
`Model.tetra_weights` / `Model.occupations` against the same model fed with `eigenval_array` / `eigh` of the same mesh.

Inputs of section 1: `tetra_exact.tie_rich_inputs` and plain seeded random rows sorted ascending (the kinds of tests/test_gpu_fermi.py)
on the meshes 2 x 3 x 2, 4 x 4 x 4, 3 x 2 x 1, 2 x 1 x 1, 1 x 5 and 3 x 4 with 1, 3, 8 and 65 orbitals (65: a point's bands cross a
wave; 2 x 3 x 2 x 65 = 780 items span four workgroups).

Bounds.  Weights against exact: 1e-13 in NK |w - exact| -- a corner weight is about a dozen roundings of quantities <= 1, below
5e-15 absolute; 24 of them over S = 6 give 2e-14; the bound is that times 5.  Sum of the weights against the probe kernel:
n_orb 2^-40 + 1e-13.  f and q against the model: 1e-11, the project's fixed-point-kernel bound (worst case 2^-41 per term over NK
terms, divided by NK); eb: 1e-12 max|E|.  Whole calls: 1e-9, times n_orb for the orbital occupations.  Every case prints
its measured maxima.
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
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import occ_model  # noqa: E402  pylint: disable=wrong-import-position
import tetra_exact as exact  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

CASES = [
    ("ties", (2, 3, 2), 3), ("ties", (4, 4, 4), 1), ("ties", (3, 2, 1), 8), ("ties", (2, 1, 1), 3), ("ties", (1, 5), 8), ("ties", (3, 4), 3),
    ("random", (2, 3, 2), 65), ("random", (3, 4), 65), ("random", (4, 4, 4), 8), ("random", (1, 5), 1), ("random", (3, 2, 1), 3),
    ("random", (2, 1, 1), 1),
]
_CACHE = {}


def _eig(kind, mesh, n_orb):
    key = ("eig", kind, mesh, n_orb)
    if key not in _CACHE:
        if kind == "ties":
            eig = exact.tie_rich_inputs(mesh, n_orb, 1)[0]
        else:
            rng = np.random.default_rng(7000 + 100 * len(mesh) + 10 * int(np.prod(mesh)) + n_orb)
            eig = np.sort(rng.uniform(-1.0, 1.0, tuple(mesh) + (n_orb,)), axis=-1)
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eig.setflags(write=False)
        _CACHE[key] = eig
    return _CACHE[key]


def _mesh32(eig):
    return np.ascontiguousarray(eig.shape[:-1], dtype=np.int32)


def _weights(eig, energy):
    mesh, flat = _mesh32(eig), np.ascontiguousarray(eig, dtype=np.float64)
    out = np.full(eig.shape, np.nan)
    _lib.check(_lib.lib().tbk_tetra_weights_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), float(energy),
                                                             _lib.ptr(out)))
    return out


def _nos_at(eig, energy):
    mesh, flat = _mesh32(eig), np.ascontiguousarray(eig, dtype=np.float64)
    energies, out = np.array([float(energy)]), np.full(1, np.nan)
    _lib.check(_lib.lib().tbk_nos_at_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), _lib.ptr(energies), 1,
                                                      _lib.ptr(out)))
    return out[0]


def _occupations(eig, U, energy, k_chunk):
    mesh, flat = _mesh32(eig), np.ascontiguousarray(eig, dtype=np.float64)
    n = eig.shape[-1]
    q, f, eb = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    _lib.check(_lib.lib().tbk_occupations_from_eigensystem(0, len(mesh), _lib.ptr(mesh), n, _lib.ptr(flat), _lib.ptr(U), float(energy), k_chunk,
                                                           _lib.ptr(q), _lib.ptr(f), _lib.ptr(eb)))
    return q, f, eb


def _energies(eig, seed):
    """mu on a corner of every rank of one simplex, one ulp above and below a corner, on and around the ends of the spectrum."""
    corners = np.sort(dos_model.simplex_corners(eig)[0].reshape(-1, eig.ndim), axis=-1)
    pick = corners[np.random.default_rng(seed).integers(len(corners))]
    lo, hi = float(eig.min()), float(eig.max())
    inside = [float(x) for x in pick] + [float(np.nextafter(pick[1], np.inf)), float(np.nextafter(pick[-2], -np.inf))]
    return inside, [lo - 0.5, float(np.nextafter(lo, -np.inf))], [hi, hi + 0.5]


# ---- 1. the weights kernel against exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mesh, n_orb", CASES)
def test_weights_kernel_matches_exact(kind, mesh, n_orb):
    eig = _eig(kind, mesh, n_orb)
    n_k = int(np.prod(mesh))
    inside, below, above = _energies(eig, 17)
    worst = worst_sum = 0.0
    for mu in inside + below + above:
        got = _weights(eig, mu)
        want = occ_model.point_weights_exact(eig, mu)
        worst = max(worst, n_k * np.abs(got - want).max())
        worst_sum = max(worst_sum, abs(got.sum() - _nos_at(eig, mu)))
        assert np.all(got >= 0.0) and np.all(n_k * got <= 1.0 + 1e-15)
    for mu in below:
        assert np.all(_weights(eig, mu) == 0.0)
    for mu in above:
        assert np.all(_weights(eig, mu) == 1.0 / n_k)
    print("%s %s x %d: NK max|w - exact| = %.3e, max|sum w - N(probe kernel)| = %.3e" % (kind, mesh, n_orb, worst, worst_sum))
    assert worst <= 1e-13, (kind, mesh, n_orb, worst)
    assert worst_sum <= n_orb * 2.0 ** -40 + 1e-13, (kind, mesh, n_orb, worst_sum)


def test_subnormal_gap_corners_are_finite_and_within_the_bound():
    eig = np.array([-0.5, 0.25, -0.25, 0.125, 0.0, -0.125, 5e-324, 0.5]).reshape(2, 2, 2, 1)  # v000, v001, v010, v011, v100, v101, v110, v111
    corners = dos_model.simplex_corners(eig)[0][0, 0, 0, 0]  # order (0, 1, 2) of cell 0: v000, v100, v110, v111
    assert list(corners) == [-0.5, 0.0, 5e-324, 0.5]
    got, want = _weights(eig, 0.0), occ_model.point_weights_exact(eig, 0.0)
    err = 8 * np.abs(got - want).max()
    print("subnormal gap: NK max|w - exact| = %.3e" % err)
    assert np.all(np.isfinite(got)) and err <= 1e-13


@pytest.mark.parametrize("exponent", [-100, 100])
@pytest.mark.parametrize("kind, mesh, n_orb", [("ties", (2, 3, 2), 3), ("random", (3, 4), 65)])
def test_scaling_by_a_power_of_two_changes_no_bit(kind, mesh, n_orb, exponent):
    eig = _eig(kind, mesh, n_orb)
    factor = 2.0 ** exponent
    for mu in _energies(eig, 19)[0]:
        assert np.array_equal(_weights(eig, mu), _weights(eig * factor, mu * factor)), (kind, mesh, mu)


@pytest.mark.parametrize("kind, mesh, n_orb", [("random", (2, 3, 2), 65), ("ties", (1, 5), 8)])
def test_two_calls_give_the_same_bits(kind, mesh, n_orb):
    eig = _eig(kind, mesh, n_orb)
    for mu in _energies(eig, 23)[0][:3]:
        assert np.array_equal(_weights(eig, mu), _weights(eig, mu))


# ---- 2. band sums and the contraction against the model -----------------------------------------------------------------------------------
def _eigensystem(n):
    key = ("system", n)
    if key not in _CACHE:
        mesh = (2, 3, 2)
        rng = np.random.default_rng(900 + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, mesh + (n,)), axis=-1)
        eig[..., 0] -= 2.0  # the lowest band lies below mu at every point: full
        U = np.linalg.qr(rng.normal(size=(12, n, n)) + 1j * rng.normal(size=(12, n, n)))[0]
        _CACHE[key] = (np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128))
    return _CACHE[key]


@pytest.mark.parametrize("n", [9, 17, 33, 65])
def test_occupation_kernels_match_the_model_for_every_chunk(n):
    eig, U = _eigensystem(n)
    mu = 0.1
    w = _weights(eig, mu)  # the kernel's own weights
    want_q, want_f, want_eb = occ_model.occupations(w, eig, U)
    results = {chunk: _occupations(eig, U, mu, chunk) for chunk in (0, 5, 1)}
    q, f, eb = results[0]
    err_q, err_f, err_eb = np.abs(q - want_q).max(), np.abs(f - want_f).max(), np.abs(eb - want_eb).max()
    gap = abs(q.sum() - f.sum())
    print("n = %d: max|q - model| = %.3e, max|f - model| = %.3e, max|eb - model| = %.3e (|E|max = %.3f), |sum q - sum f| = %.3e"
          % (n, err_q, err_f, err_eb, np.abs(eig).max(), gap))
    assert err_q <= 1e-11 and err_f <= 1e-11 and err_eb <= 1e-12 * np.abs(eig).max(), (n, err_q, err_f, err_eb)
    assert f[0] == 1.0 and np.all(f >= 0.0) and np.all(f <= 1.0)
    assert gap <= n * 2.0 ** -40
    for chunk in (5, 1):
        assert np.array_equal(results[chunk][0], q) and np.array_equal(results[chunk][1], f), (n, chunk)
        assert np.array_equal(results[chunk][2], eb)


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------------
def _models():
    g = load_golden("silicon")
    yield "silicon", tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"]), (2, 3, 2), 4
    for dim, mesh in ((3, (2, 3, 2)), (2, (3, 4))):
        r_vec, hop, pos = syn.dense_model_arrays(9, 6, syn.MODEL_SEED + 1400 + dim, dim=dim)
        yield "dense 9 orbitals", tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos), mesh, 3.1


def _check_whole_call(label, model, mesh, n_electrons, eig, vec):
    n, n_k, scale = model.size, int(np.prod(mesh)), np.abs(eig).max()
    level = model.fermi_level(mesh, n_electrons)
    occ = model.occupations(mesh, n_electrons=n_electrons)
    assert isinstance(occ, tbmodels_amd._model.Occupations) and isinstance(occ.mu, tbmodels_amd._model.FermiLevel)
    assert occ.mu == level, (label, occ.mu, level)  # bit for bit
    w = model.tetra_weights(mesh, level.mu)
    assert w.shape == tuple(mesh) + (n,)
    want_w = occ_model.point_weights(eig, level.mu)
    err_w = n_k * np.abs(w - want_w).max()
    want_q, want_f, want_eb = occ_model.occupations(want_w, eig, vec)
    by_energy = model.occupations(mesh, energy=level.mu)
    assert by_energy.mu.mu == by_energy.mu.lower == by_energy.mu.upper == level.mu
    assert abs(by_energy.mu.nos - w.sum()) <= n * 2.0 ** -40 + 1e-13
    assert np.array_equal(by_energy.orbital_occ, occ.orbital_occ) and np.array_equal(by_energy.band_occ, occ.band_occ)
    assert np.array_equal(by_energy.band_energy, occ.band_energy)
    err_f, err_eb = np.abs(occ.band_occ - want_f).max(), np.abs(occ.band_energy - want_eb).max()
    print("%s %s n = %s: NK max|w - model| = %.3e, max|f - model| = %.3e, max|eb - model| = %.3e (|E|max = %.3f)"
          % (label, mesh, n_electrons, err_w, err_f, err_eb, scale))
    assert err_w <= 1e-9 and err_f <= 1e-9 and err_eb <= 1e-9 * scale, (label, err_w, err_f, err_eb)
    assert abs(occ.orbital_occ.sum() - occ.band_occ.sum()) <= n * 2.0 ** -40
    if level.lower < level.upper:  # the gap case: full and empty bands, a basis-independent projector
        m = int(n_electrons)
        assert np.array_equal(occ.band_occ, np.array([1.0] * m + [0.0] * (n - m))), occ.band_occ
        want_q = (np.abs(vec[:, :, :m]) ** 2).sum(axis=2).mean(axis=0)
    err_q = np.abs(occ.orbital_occ - want_q).max()
    print("%s %s n = %s: max|q - model| = %.3e" % (label, mesh, n_electrons, err_q))
    assert err_q <= 1e-9 * n, (label, err_q)
    return w, occ


def test_model_methods_against_the_model_of_the_same_mesh():
    gaps = 0
    for label, model, mesh, n_electrons in _models():
        kpts = dos_model.mesh_kpoints(mesh)
        eig = np.ascontiguousarray(np.array(model.eigenval_array(kpts)).reshape(tuple(mesh) + (model.size,)))
        vec = model.eigh(kpts)[1]
        model.set_option(_lib.TBK_OPT_TIMING, 1)
        w1, occ1 = _check_whole_call(label, model, mesh, n_electrons, eig, vec)
        gaps += int(occ1.mu.lower < occ1.mu.upper)
        ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
        _lib.check(_lib.lib().tbk_occ_timing(model._staged_all()[0], ms, ctypes.byref(calls), 1))
        print("%s %s: %d calls, kernels %.3f / %.3f / %.3f ms" % (label, mesh, calls.value, ms[0], ms[1], ms[2]))
        assert calls.value == 3 and min(ms) > 0.0
        model.set_option(_lib.TBK_OPT_K_CHUNK, 5)  # chunks that are no whole planes: no bit of q moves
        assert np.array_equal(model.occupations(mesh, n_electrons=n_electrons).orbital_occ, occ1.orbital_occ)
        # two handles on one device: the slabs with both neighbour planes
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        w2, occ2 = _check_whole_call(label + ", two handles", twin, mesh, n_electrons, eig, vec)
        assert len(twin._handles) == 2
        same = np.array_equal(w1, w2)
        print("%s %s: one handle and two give %s weights" % (label, mesh, "the same bits of the" if same else "different"))
        if same:  # the same eigenvalues reached both: the integer sums cannot differ
            assert np.array_equal(occ1.band_occ, occ2.band_occ) and np.array_equal(occ1.orbital_occ, occ2.orbital_occ)
        assert np.abs(occ1.band_energy - occ2.band_energy).max() <= 1e-12 * np.abs(eig).max()
    assert gaps == 1  # silicon at n = 4


def test_untimed_calls_are_counted_without_time():
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    model.occupations((4, 4, 4), n_electrons=4.5)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_occ_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]


# ---- 4. arguments -----------------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    for mesh in ((4, 4), (4, 4, 4, 4), (4, 0, 4), (4, -2, 4), (4, 2.5, 4), (4.0, 4.0, 4.0), 4, (2 ** 11, 2 ** 10, 2 ** 10)):
        with pytest.raises(ValueError):
            model.tetra_weights(mesh, 0.0)
        with pytest.raises(ValueError):
            model.occupations(mesh, n_electrons=4)
    for kwargs in ({}, {"energy": 0.0, "n_electrons": 4}, {"energy": np.nan}, {"energy": np.inf}, {"energy": "0"}, {"energy": True},
                   {"n_electrons": 0}, {"n_electrons": 8}, {"n_electrons": np.nan}, {"n_electrons": "4"}, {"n_electrons": -1.0}):
        with pytest.raises(ValueError):
            model.occupations((2, 2, 2), **kwargs)
    for energy in (np.nan, -np.inf, None, "1", 1j):
        with pytest.raises(ValueError):
            model.tetra_weights((2, 2, 2), energy)
    with pytest.raises(TypeError):
        model.occupations((2, 2, 2), 0.0)  # keyword only
    with pytest.raises(ValueError):
        one_d.tetra_weights((8,), 0.0)
    with pytest.raises(ValueError):
        one_d.occupations((8,), energy=0.0)
    assert not hasattr(tbmodels_amd.KdotpModel, "tetra_weights") and not hasattr(tbmodels_amd.KdotpModel, "occupations")


def test_c_argument_errors():
    lib = _lib.lib()
    eig = np.ascontiguousarray(_eig("random", (2, 3, 2), 65)[..., :8])
    U = np.ascontiguousarray(np.broadcast_to(np.eye(8, dtype=np.complex128), (12, 8, 8)))
    mesh = np.array([2, 3, 2], dtype=np.int32)
    w, q, f, eb, four = np.zeros((12, 8)), np.zeros(8), np.zeros(8), np.zeros(8), np.zeros(4)

    def weights(dim=3, mesh_=mesh, n_orb=8, eig_=eig, energy=0.0, out=w):
        return lib.tbk_tetra_weights_from_eigenvalues(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), energy, _lib.ptr(out))

    def occ(dim=3, mesh_=mesh, n_orb=8, eig_=eig, U_=U, energy=0.0, chunk=0, q_=q, f_=f, eb_=eb):
        return lib.tbk_occupations_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), energy, chunk, _lib.ptr(q_),
                                                    _lib.ptr(f_), _lib.ptr(eb_))

    assert weights() == occ() == _lib.TBK_OK
    zero = np.array([2, 0, 2], dtype=np.int32)
    nan, inf = float("nan"), float("inf")
    bad = [weights(dim=1), weights(dim=4), weights(mesh_=zero), weights(mesh_=None), weights(eig_=None), weights(out=None), weights(n_orb=0),
           weights(energy=nan), weights(energy=inf),
           occ(dim=1), occ(mesh_=zero), occ(mesh_=None), occ(eig_=None), occ(U_=None), occ(q_=None), occ(f_=None), occ(eb_=None), occ(n_orb=0),
           occ(energy=nan), occ(energy=-inf), occ(chunk=-1)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    # the handle entry points (a k.p model has no such method: test above)
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    m32, pw, p4, pq, pf, pe = _lib.ptr(mesh), _lib.ptr(w), _lib.ptr(four), _lib.ptr(q), _lib.ptr(f), _lib.ptr(eb)
    bad = [lib.tbk_tetra_weights(None, m32, 0.0, pw), lib.tbk_tetra_weights(handle, None, 0.0, pw), lib.tbk_tetra_weights(handle, m32, 0.0, None),
           lib.tbk_tetra_weights(handle, m32, nan, pw), lib.tbk_tetra_weights(handle, _lib.ptr(zero), 0.0, pw),
           lib.tbk_tetra_weights_multi(twice, 2, m32, 0.0, pw), lib.tbk_tetra_weights_multi(None, 1, m32, 0.0, pw),
           lib.tbk_occupations(None, m32, 0, 0.0, p4, pq, pf, pe), lib.tbk_occupations(handle, None, 0, 0.0, p4, pq, pf, pe),
           lib.tbk_occupations(handle, m32, 0, 0.0, None, pq, pf, pe), lib.tbk_occupations(handle, m32, 0, 0.0, p4, None, pf, pe),
           lib.tbk_occupations(handle, m32, 0, 0.0, p4, pq, None, pe), lib.tbk_occupations(handle, m32, 0, 0.0, p4, pq, pf, None),
           lib.tbk_occupations(handle, m32, 2, 0.0, p4, pq, pf, pe), lib.tbk_occupations(handle, m32, -1, 0.0, p4, pq, pf, pe),
           lib.tbk_occupations(handle, m32, 0, inf, p4, pq, pf, pe), lib.tbk_occupations(handle, m32, 1, 0.0, p4, pq, pf, pe),
           lib.tbk_occupations(handle, m32, 1, 8.0, p4, pq, pf, pe), lib.tbk_occupations(handle, m32, 1, nan, p4, pq, pf, pe),
           lib.tbk_occupations(handle, _lib.ptr(zero), 1, 4.0, p4, pq, pf, pe),
           lib.tbk_occupations_multi(twice, 2, m32, 1, 4.0, p4, pq, pf, pe), lib.tbk_occupations_multi(None, 1, m32, 1, 4.0, p4, pq, pf, pe),
           lib.tbk_occ_timing(None, ms, ctypes.byref(calls), 0), lib.tbk_occ_timing(handle, None, ctypes.byref(calls), 0),
           lib.tbk_occ_timing(handle, ms, None, 0)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
