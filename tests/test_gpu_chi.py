"""
The Fermi-table, overlap, pair and reduction kernels (csrc/tbk_chi.hip) against tools/chi_model.py on identical (E, U), and
`Model.susceptibility` against its properties and against the model fed with the eigensystem `Model.eigh` returns for the same mesh.

Bound: chi_model.tolerance, tol_chi of DESIGN.md 15.4 -- derived from the number formats, the sizes and an allowance of 2 ulps for
exp and expm1 per side; nothing measured on the kernels enters it.  A whole call is compared with the model on the eigensystem of
`Model.eigh` (the same solver on the same k list: the same bits as the resident one), so the bound is the same.  Identities of bits
(properties 5, 6, 7, mu against `fermi_level`, two handles against one) are asserted as such.  Every case prints its measured maximum.
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
import chi_model  # noqa: E402  pylint: disable=wrong-import-position
import dos_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

MU = 0.1
TEMPERATURES = (0.05, 0.5)
_CACHE = {}


def _eigensystem(mesh, n):
    """Random ascending bands and random unitary U (QR of complex Gaussians), shared by the cases and never written.  Band 0 is flat
    (equal values at k and k+q: the y = 0 branch between different points), bands 1 and 2 are an exact degenerate pair inside every
    k-point (three orbitals or more), and mu = 0.1 lies inside the others."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(6100 + 41 * n_k + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
        eig[:, 0] = -1.25 if n > 1 else 0.125
        if n >= 3:
            eig[:, 2] = eig[:, 1]
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        for array in (eig, U):
            array.setflags(write=False)
        _CACHE[key] = (eig, U)
    return _CACHE[key]


def _vectors(mesh):
    """0, +-e_d, a vector with every component non-zero, the same shifted by whole mesh periods, a duplicate of +e_0."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], (full + shift)[None, :], unit[:1]])
    return np.ascontiguousarray(q), (1 + 2 * dim, 2 + 2 * dim), (1, 3 + 2 * dim)


def _phases(n_q, n, pairs):
    """A random table of unit phases; the second row of every pair is a copy of the first."""
    angle = np.random.default_rng(77 + n).uniform(0.0, 2.0 * np.pi, (n_q, n))
    table = np.cos(angle) + 1j * np.sin(angle)
    for first, second in pairs:
        table[second] = table[first]
    return np.ascontiguousarray(table)


def _from_eigensystem(mesh, eig, U, q, T, phases=None, mu=MU):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.int64)
    out = np.full(len(q), np.nan)
    _lib.check(_lib.lib().tbk_chi_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), float(mu), float(T), len(q),
                                                   _lib.ptr(q), _lib.ptr(phases), _lib.ptr(out)))
    return out


def _plan(n_k, n_orb, n_q, matrix_elements=True, part_bytes=0):
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.lib().tbk_chi_plan(n_k, n_orb, n_q, int(matrix_elements), part_bytes, out))
    return {"template": out[0], "blocks": out[1], "batch": out[2], "batches": out[3]}


def _kernel_case(mesh, n):
    eig, U = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, shifted, duplicate = _vectors(mesh)
    table = _phases(len(q), n, (shifted, duplicate))
    order = np.random.default_rng(9).permutation(len(q))
    report = []
    for T in TEMPERATURES:
        for what, vec, phases in (("overlaps", U, None), ("overlaps with phases", U, table), ("pairs", None, None)):
            want = chi_model.susceptibility(eig, vec, mesh, q, MU, T, vec is not None, phases)
            got = _from_eigensystem(mesh, eig, vec, q, T, phases)
            bound = chi_model.tolerance(n_k, n, T, vec is not None)
            err = np.abs(got - want).max()
            report.append("%s T = %g: %.3e (bound %.3e)" % (what, T, err, bound))
            assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and err <= bound, (mesh, n, T, what, err, bound)
            assert got[shifted[0]] == got[shifted[1]], (mesh, n, T, what, "a whole mesh period changed bits")  # property 6
            assert got[duplicate[0]] == got[duplicate[1]], (mesh, n, T, what, "a duplicate differs")  # property 7 ...
            assert np.array_equal(got, _from_eigensystem(mesh, eig, vec, q, T, phases)), (mesh, n, T, what, "two calls differ")
            moved = None if phases is None else np.ascontiguousarray(phases[order])
            assert np.array_equal(got[order], _from_eigensystem(mesh, eig, vec, q[order], T, moved)), (mesh, n, T, what, "the order changed bits")
            for index in (0, len(q) - 3):
                alone = _from_eigensystem(mesh, eig, vec, q[index:index + 1], T, None if phases is None else np.ascontiguousarray(phases[index:index + 1]))
                assert alone[0] == got[index], (mesh, n, T, what, "the rest of the list changed bits")
    return report


# ---- 1. the kernels against the model on the same (E, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16, 17, 33, 64, 65])
def test_kernels_match_the_model_on_2x3x2(n):
    plan = _plan(12, n, 9)
    assert plan["template"] == (1 if n <= 16 else 4) and plan["blocks"] == (1 if n <= 64 else 4) and plan["batches"] == 1
    assert _plan(12, n, 9, matrix_elements=False)["template"] == 0
    for line in _kernel_case((2, 3, 2), n):
        print("mesh (2, 3, 2) n = %d max|chi - model|, %s" % (n, line))


@pytest.mark.parametrize("mesh, n", [((3, 4), 9), ((1, 5), 9), ((4, 4, 4), 8)])
def test_kernels_match_the_model_on_other_meshes(mesh, n):
    for line in _kernel_case(mesh, n):
        print("mesh %s n = %d max|chi - model|, %s" % (mesh, n, line))


def test_a_long_list_goes_in_batches():
    mesh, n, n_q, T = (2, 3, 2), 3, 4100, 0.05
    plan = _plan(12, n, n_q)
    print("plan of 12 points, 3 orbitals, %d vectors:" % n_q, plan)
    assert plan["batches"] >= 2 and plan["batch"] * plan["batches"] >= n_q > plan["batch"]
    small = _plan(12, 65, 10, part_bytes=3 * 12 * 4 * 8)  # the memory argument: room for the partials of three vectors
    assert small == {"template": 4, "blocks": 4, "batch": 3, "batches": 4}
    assert _plan(12, 65, 10, part_bytes=8)["batch"] == 0  # not one vector fits
    eig, U = _eigensystem(mesh, n)
    q = np.random.default_rng(21).integers(-7, 8, size=(n_q, 3)).astype(np.int64)
    for vec in (U, None):
        want = chi_model.susceptibility(eig, vec, mesh, q, MU, T, vec is not None)
        got = _from_eigensystem(mesh, eig, vec, q, T)
        err, bound = np.abs(got - want).max(), chi_model.tolerance(12, n, T, vec is not None)
        print("%d vectors in %d batches, %s: max|chi - model| = %.3e (bound %.3e)" % (n_q, plan["batches"], "overlaps" if vec is not None else "pairs", err, bound))
        assert err <= bound
        for index in (plan["batch"] - 1, plan["batch"], n_q - 1):  # on both sides of the batch boundary: the bits of a call of its own
            assert got[index] == _from_eigensystem(mesh, eig, vec, q[index:index + 1], T)[0]


def test_extreme_temperatures_and_chemical_potentials():
    mesh, n = (2, 3, 2), 17
    eig, U = _eigensystem(mesh, n)
    q, _, _ = _vectors(mesh)
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # property 5: every f (or every 1 - f) is 0
            for vec in (U, None):
                got = _from_eigensystem(mesh, eig, vec, q, T, mu=mu)
                assert np.all(got == 0.0) and not np.any(np.signbit(got)), (T, mu, got)
    hot = 1e9 * float(np.ptp(eig))
    got = _from_eigensystem(mesh, eig, U, q, hot)  # property 4
    err, bound = np.abs(4.0 * hot * got - n).max(), 4.0 * hot * chi_model.tolerance(12, n, hot) + 1e-17 * n
    print("T = 1e9 bandwidths: max|4 T chi - n| = %.3e (bound %.3e)" % (err, bound))
    assert err <= bound
    cold = _from_eigensystem(mesh, eig, U, q, 1e-6)
    want = chi_model.susceptibility(eig, U, mesh, q, MU, 1e-6)
    print("T = 1e-6: chi =", cold, "max|chi - model| = %.3e (bound %.3e)" % (np.abs(cold - want).max(), chi_model.tolerance(12, n, 1e-6)))
    assert np.all(np.isfinite(cold)) and np.all(cold >= 0.0) and np.abs(cold - want).max() <= chi_model.tolerance(12, n, 1e-6)


# ---- 2. whole calls ------------------------------------------------------------------------------------------------------------------
def _silicon(sparse=False):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    if sparse:
        model.set_sparse()
    return model


def _dense9(dim):
    r_vec, hop, pos = syn.dense_model_arrays(9, 6, syn.MODEL_SEED + 1400 + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


CALLS = {"silicon": (lambda: _silicon(), (2, 3, 2), 4.5), "silicon CSR": (lambda: _silicon(True), (2, 3, 2), 4.5),
         "dense 9, 3-D": (lambda: _dense9(3), (2, 3, 2), 3.1), "dense 9, 2-D": (lambda: _dense9(2), (3, 4), 3.1)}


@pytest.mark.parametrize("name", list(CALLS))
def test_properties_of_a_whole_call(name):
    make, mesh, n_el = CALLS[name]
    model = make()
    n, n_k = model.size, int(np.prod(mesh))
    q, shifted, duplicate = _vectors(mesh)
    plus, minus = list(range(1, 1 + len(mesh))), list(range(1 + len(mesh), 1 + 2 * len(mesh)))
    kpts = dos_model.mesh_kpoints(mesh)
    eig, vec = model.eigh(kpts)
    level = model.fermi_level(mesh, n_el)
    for T in TEMPERATURES:
        tol, tol_pair = chi_model.tolerance(n_k, n, T), chi_model.tolerance(n_k, n, T, False)
        result = model.susceptibility(mesh, q, temperature=T, n_electrons=n_el)
        assert isinstance(result, tbmodels_amd.Susceptibility) and result.mu == level  # bit for bit
        assert result.q.dtype == np.int64 and np.array_equal(result.q, q) and result.chi.shape == (len(q),) and result.chi.dtype == np.float64
        chi = result.chi
        assert np.all(np.isfinite(chi)) and np.all(chi >= 0.0)  # property 1
        err_1 = np.abs(chi[plus] - chi[minus]).max()
        err_2 = abs(chi[0] - chi_model.static_limit(eig, level.mu, T))  # property 2
        err_m = np.abs(chi - chi_model.susceptibility(eig, vec, mesh, q, level.mu, T)).max()
        assert chi[shifted[0]] == chi[shifted[1]] and chi[duplicate[0]] == chi[duplicate[1]]  # properties 6 and 7
        first = model.susceptibility(mesh, q, temperature=T, n_electrons=n_el, convention=1)
        assert first.mu == level
        err_c = np.abs(first.chi - chi_model.susceptibility(eig, vec, mesh, q, level.mu, T, True, chi_model.phase_table(mesh, q, model.pos))).max()
        err_c1 = np.abs(first.chi[plus] - first.chi[minus]).max()
        assert np.all(first.chi >= 0.0) and first.chi[0] == chi[0]  # D(0) = 1
        pair = model.susceptibility(mesh, q, temperature=T, energy=level.mu, matrix_elements=False)
        assert pair.mu.mu == level.mu and np.all(pair.chi >= 0.0)
        err_3 = np.abs(pair.chi - chi_model.susceptibility(model.eigenval_array(kpts), None, mesh, q, level.mu, T, False)).max()  # property 3
        print("%s %s T = %g: chi(q) - chi(-q) %.3e, chi(0) - static limit %.3e, chi - model %.3e, convention 1 - model %.3e, its inversion %.3e "
              "(bound %.3e); pairs - model %.3e (bound %.3e)" % (name, mesh, T, err_1, err_2, err_m, err_c, err_c1, tol, err_3, tol_pair))
        assert max(err_1, err_2, err_m, err_c, err_c1) <= tol and err_3 <= tol_pair
    edges = model.band_edges(mesh)
    hot = 1e9 * float(edges.emax.max() - edges.emin.min())
    for convention in (1, 2):  # property 4
        chi = model.susceptibility(mesh, q, temperature=hot, n_electrons=n_el, convention=convention).chi
        err, bound = np.abs(4.0 * hot * chi - n).max(), 4.0 * hot * chi_model.tolerance(n_k, n, hot) + 1e-17 * n
        print("%s convention %d, T = 1e9 bandwidths: max|4 T chi - n| = %.3e (bound %.3e)" % (name, convention, err, bound))
        assert err <= bound
    for me in (True, False):  # property 5
        below = model.susceptibility(mesh, q, temperature=0.05, energy=float(edges.emin.min()) - 746.0 * 0.05, matrix_elements=me).chi
        assert np.all(below == 0.0) and not np.any(np.signbit(below))
    cold = model.susceptibility(mesh, q, temperature=1e-6, n_electrons=n_el).chi
    print("%s T = 1e-6: chi =" % name, cold)
    assert np.all(np.isfinite(cold)) and np.all(cold >= 0.0)


def test_two_handles_give_the_bits_of_one():
    for make, mesh, n_el in (CALLS["silicon"], CALLS["dense 9, 2-D"]):
        model = make()
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        q, _, _ = _vectors(mesh)
        for kwargs in ({}, {"convention": 1}, {"matrix_elements": False}):
            one = model.susceptibility(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs)
            two = twin.susceptibility(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs)
            assert len(twin._handles) == 2 and two.mu == one.mu
            assert np.array_equal(one.chi, two.chi), (kwargs, np.abs(one.chi - two.chi).max())
            assert np.array_equal(one.chi[:1], twin.susceptibility(mesh, q[:1], temperature=0.05, n_electrons=n_el, **kwargs).chi)  # one vector, two handles
            assert np.array_equal(one.chi, model.susceptibility(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs).chi)  # the same call again


# ---- 3. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    q = np.array([[1, 0, 0], [2, 1, 0]], dtype=np.int64)
    model.susceptibility((4, 4, 4), q, temperature=0.1, n_electrons=4.5)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    timed = model.susceptibility((4, 4, 4), q, temperature=0.1, n_electrons=4.5)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 2 vectors: %d calls, Fermi tables %.3f ms, overlaps %.3f ms, reduction %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    assert np.array_equal(timed.chi, model.susceptibility((4, 4, 4), q, temperature=0.1, n_electrons=4.5).chi)  # the chunk changes no bit
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    assert calls.value == 1


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U = _eigensystem((2, 3, 2), 9)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    zero = np.array([2, 0, 2], dtype=np.int32)
    q = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    table = _phases(2, 9, ())
    chi, four = np.zeros(2), np.zeros(4)
    nan, inf = float("nan"), float("inf")

    def call(dim=3, mesh_=mesh, n_orb=9, eig_=eig, U_=U, mu=0.0, T=0.1, n_q=2, q_=q, phases=None, out=chi):
        return lib.tbk_chi_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), mu, T, n_q, _lib.ptr(q_), _lib.ptr(phases),
                                            _lib.ptr(out))

    assert call() == _lib.TBK_OK and call(U_=None) == _lib.TBK_OK and call(phases=table) == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=zero), call(mesh_=None), call(eig_=None), call(q_=None), call(out=None), call(n_orb=0),
           call(mu=nan), call(mu=inf), call(T=0.0), call(T=-0.1), call(T=nan), call(T=inf), call(n_q=0), call(n_q=-3), call(U_=None, phases=table)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    pos = np.ascontiguousarray(model.pos, dtype=np.float64)
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 4)()
    m32, pq, pp, p4, po = _lib.ptr(mesh), _lib.ptr(q), _lib.ptr(pos), _lib.ptr(four), _lib.ptr(chi)

    def whole(handle_=handle, mesh_=m32, mode=0, value=0.0, T=0.1, n_q=2, q_=pq, me=1, convention=2, pos_=pp, mu_=p4, out=po):
        return lib.tbk_susceptibility(handle_, mesh_, mode, value, T, n_q, q_, me, convention, pos_, mu_, out)

    assert whole() == _lib.TBK_OK and whole(convention=1) == _lib.TBK_OK and whole(pos_=None) == _lib.TBK_OK
    bad = [whole(handle_=None), whole(mesh_=None), whole(mode=2), whole(value=inf), whole(mode=1, value=0.0), whole(mode=1, value=8.0),
           whole(mode=1, value=nan), whole(T=0.0), whole(T=-1.0), whole(T=nan), whole(T=inf), whole(n_q=0), whole(q_=None), whole(convention=0),
           whole(convention=3), whole(convention=1, pos_=None), whole(mu_=None), whole(out=None), whole(mesh_=_lib.ptr(zero)),
           lib.tbk_susceptibility_multi(twice, 2, m32, 1, 4.0, 0.1, 2, pq, 1, 2, pp, p4, po),
           lib.tbk_susceptibility_multi(None, 1, m32, 1, 4.0, 0.1, 2, pq, 1, 2, pp, p4, po),
           lib.tbk_chi_timing(None, ms, ctypes.byref(calls), 0), lib.tbk_chi_timing(handle, None, ctypes.byref(calls), 0),
           lib.tbk_chi_timing(handle, ms, None, 0), lib.tbk_chi_plan(0, 8, 2, 1, 0, plan), lib.tbk_chi_plan(64, 0, 2, 1, 0, plan),
           lib.tbk_chi_plan(64, 8, 0, 1, 0, plan), lib.tbk_chi_plan(64, 8, 2, 1, -1, plan), lib.tbk_chi_plan(64, 8, 2, 1, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
