"""
The dynamic epilogue, pair and reduction kernels (csrc/tbk_chi.hip) against tools/chi_model.py `dynamic_susceptibility` on identical
(E, U), and `Model.dynamic_susceptibility` against its properties, against `Model.susceptibility` and against the model fed with the
eigensystem `Model.eigh` returns for the same mesh.

Bound: chi_model.dynamic_tolerance, per frequency and in either component -- derived from the number formats, the
sizes and allowances of 2 for exp, expm1 and the quotient per side; nothing measured on the kernels enters it.  Identities of bits
(properties 5, 6, 7, the q batches, the frequency passes, mu against `fermi_level`, two handles against one) are asserted as such.
Every case prints its measured maximum.
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
ETAS = (0.05, 1e-3)
_CACHE = {}


def _eigensystem(mesh, n):
    """Random ascending bands and random unitary U (QR of complex Gaussians), shared by the cases and never written.  Band 0 is flat
    (equal values at k and k+q: g = 0 between different points), bands 1 and 2 are an exact degenerate pair inside every k-point (three
    orbitals or more), and mu = 0.1 lies inside the others."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(8100 + 41 * n_k + n)
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
    """0, +-e_d, a vector with every component non-zero, its negative, the first shifted by whole mesh periods, a duplicate of +e_0;
    the index lists of the (q, -q) pairs, the (vector, shifted) pair and the (original, duplicate) pair."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], -full[None, :], (full + shift)[None, :], unit[:1]])
    plus, minus = list(range(1, 1 + dim)) + [1 + 2 * dim], list(range(1 + dim, 1 + 2 * dim)) + [2 + 2 * dim]
    return np.ascontiguousarray(q), plus, minus, (1 + 2 * dim, 3 + 2 * dim), (1, 4 + 2 * dim)


MIRROR = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 2])  # omega -> -omega in the list of _frequencies


def _frequencies(eig_a, eig_b):
    """0, +-0.2, +-0.7, +-one exact level difference (x = 0 for that pair), +-1e6, a duplicate of 0.2: ten, more than one register chunk."""
    level = float(eig_b - eig_a)
    return np.array([0.0, 0.2, -0.2, 0.7, -0.7, level, -level, 1e6, -1e6, 0.2])


def _phases(n_q, n, pairs):
    """A random table of unit phases; the second row of every pair is a copy of the first."""
    angle = np.random.default_rng(177 + n).uniform(0.0, 2.0 * np.pi, (n_q, n))
    table = np.cos(angle) + 1j * np.sin(angle)
    for first, second in pairs:
        table[second] = table[first]
    return np.ascontiguousarray(table)


def _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases=None, mu=MU, part_bytes=0):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.int64)
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    out = np.full((len(q), len(omega)), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_dynamic_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), float(mu), float(T),
                                                           len(q), _lib.ptr(q), _lib.ptr(phases), len(omega), _lib.ptr(omega), float(eta),
                                                           int(part_bytes), _lib.ptr(out)))
    return out


def _plan(n_k, n_orb, n_q, n_w, matrix_elements=True, part_bytes=0):
    out = (ctypes.c_int64 * 7)()
    _lib.check(_lib.lib().tbk_chi_dynamic_plan(n_k, n_orb, n_q, n_w, int(matrix_elements), part_bytes, out))
    return {"template": out[0], "blocks": out[1], "batch": out[2], "batches": out[3], "w_pass": out[4], "passes": out[5], "chunk": out[6]}


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _worst(got, want, tol):
    gap = got - want
    return float(np.maximum(np.abs(gap.real), np.abs(gap.imag)).max()), bool(np.all(np.abs(gap.real) <= tol) and np.all(np.abs(gap.imag) <= tol))


def _kernel_case(mesh, n):
    eig, U = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, _, _, shifted, duplicate = _vectors(mesh)
    omega = _frequencies(eig[0, 0], eig[chi_model.shifted_points(mesh, q[1])[0], n - 1])
    spread = 2.0 * float(np.ptp(eig)) + np.abs(omega)
    table = _phases(len(q), n, (shifted, duplicate))
    q_order, w_order = np.random.default_rng(9).permutation(len(q)), np.random.default_rng(10).permutation(len(omega))
    chunk = _plan(n_k, n, len(q), len(omega))["chunk"]
    report = []
    for T in TEMPERATURES:
        for eta in ETAS:
            for what, vec, phases in (("overlaps", U, None), ("overlaps with phases", U, table), ("pairs", None, None)):
                want = chi_model.dynamic_susceptibility(eig, vec, mesh, q, MU, T, omega, eta, vec is not None, phases)
                got = _from_eigensystem(mesh, eig, vec, q, T, omega, eta, phases)
                bound = chi_model.dynamic_tolerance(n_k, n, T, eta, spread, vec is not None)[None, :]
                err, inside = _worst(got, want, bound)
                report.append("%s T = %g eta = %g: %.3e (bound %.3e - %.3e)" % (what, T, eta, err, bound.min(), bound.max()))
                where = (mesh, n, T, eta, what)
                assert np.all(np.isfinite(_bits(got))) and inside, where + (err,)
                assert _same(got[shifted[0]], got[shifted[1]]), where + ("a whole mesh period changed bits",)  # property 6
                assert _same(got[duplicate[0]], got[duplicate[1]]) and _same(got[:, 1], got[:, 9]), where + ("a duplicate differs",)  # property 7 ...
                assert _same(got, _from_eigensystem(mesh, eig, vec, q, T, omega, eta, phases)), where + ("two calls differ",)
                moved = None if phases is None else np.ascontiguousarray(phases[q_order])
                assert _same(got[q_order][:, w_order], _from_eigensystem(mesh, eig, vec, q[q_order], T, omega[w_order], eta, moved)), where + ("the order changed bits",)
                for index, j in ((0, 0), (len(q) - 4, 5), (1, 8)):
                    alone = _from_eigensystem(mesh, eig, vec, q[index:index + 1], T, omega[j:j + 1], eta,
                                              None if phases is None else np.ascontiguousarray(phases[index:index + 1]))
                    assert _same(alone[0, 0], got[index, j]), where + ("the rest of the lists changed bits",)
    # lists of one frequency less than a register chunk, a whole chunk and one more: the bits of the ten-frequency list, position by position
    T, eta = 0.05, 1e-3
    many = np.concatenate([omega, 0.05 * np.arange(1, chunk + 2)])
    for vec in (U, None):
        base = _from_eigensystem(mesh, eig, vec, q[:3], T, many, eta)
        for count in (chunk - 1, chunk, chunk + 1):
            got = _from_eigensystem(mesh, eig, vec, q[:3], T, many[:count], eta)
            assert _same(got, base[:, :count]), (mesh, n, count, "the length of the list changed bits")
            tail = _from_eigensystem(mesh, eig, vec, q[:3], T, many[len(many) - count:], eta)
            assert _same(tail, base[:, len(many) - count:]), (mesh, n, count, "the place in the chunk changed bits")
    return report


# ---- 1. the kernels against the model on the same (E, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16, 17, 33, 64, 65])
def test_kernels_match_the_model_on_2x3x2(n):
    plan = _plan(12, n, 11, 10)
    assert plan["template"] == (1 if n <= 16 else 4) and plan["blocks"] == (1 if n <= 64 else 4)
    assert (plan["batch"], plan["batches"], plan["w_pass"], plan["passes"]) == (11, 1, 10, 1) and plan["chunk"] >= 2
    assert _plan(12, n, 11, 10, matrix_elements=False)["template"] == 0
    for line in _kernel_case((2, 3, 2), n):
        print("mesh (2, 3, 2) n = %d max|chi - model|, %s" % (n, line))


@pytest.mark.parametrize("mesh, n", [((3, 4), 9), ((1, 5), 9), ((4, 4, 4), 8)])
def test_kernels_match_the_model_on_other_meshes(mesh, n):
    for line in _kernel_case(mesh, n):
        print("mesh %s n = %d max|chi - model|, %s" % (mesh, n, line))


def test_a_long_list_of_vectors_goes_in_batches():
    mesh, n, n_q, T, eta = (2, 3, 2), 3, 4100, 0.05, 1e-3
    omega = np.array([0.3, -1.1])
    plan = _plan(12, n, n_q, 2)
    print("plan of 12 points, 3 orbitals, %d vectors, 2 frequencies:" % n_q, plan)
    assert plan["batch"] == 4096 and plan["batches"] == 2 and plan["w_pass"] == 2 and plan["passes"] == 1
    eig, U = _eigensystem(mesh, n)
    q = np.random.default_rng(21).integers(-7, 8, size=(n_q, 3)).astype(np.int64)
    spread = 2.0 * float(np.ptp(eig)) + np.abs(omega)
    for vec in (U, None):
        want = chi_model.dynamic_susceptibility(eig, vec, mesh, q, MU, T, omega, eta, vec is not None)
        got = _from_eigensystem(mesh, eig, vec, q, T, omega, eta)
        bound = chi_model.dynamic_tolerance(12, n, T, eta, spread, vec is not None)[None, :]
        err, inside = _worst(got, want, bound)
        print("%d vectors in %d batches, %s: max|chi - model| = %.3e (bound %.3e)" % (n_q, plan["batches"], "overlaps" if vec is not None else "pairs", err, bound.min()))
        assert inside
        for index in (plan["batch"] - 1, plan["batch"], n_q - 1):  # on both sides of the batch boundary: the bits of a call of its own
            assert _same(got[index], _from_eigensystem(mesh, eig, vec, q[index:index + 1], T, omega, eta)[0])


@pytest.mark.parametrize("n, fit", [(9, 5), (17, 8), (65, 8)])
def test_frequencies_go_in_passes_when_the_partials_do_not_fit(n, fit):
    """part_bytes with room for `fit` (q, omega) pairs and ten frequencies: two passes, of 5 + 5 (less than a register chunk fits: the
    pass is what fits) or 8 + 2 (whole chunks), one vector per batch."""
    mesh, T, eta = (2, 3, 2), 0.05, 1e-3
    eig, U = _eigensystem(mesh, n)
    q = _vectors(mesh)[0][:4]
    omega = _frequencies(eig[0, 0], eig[chi_model.shifted_points(mesh, q[1])[0], n - 1])
    blocks = 4 if n > 64 else 1
    room = fit * 16 * 12 * blocks + 15
    plan = _plan(12, n, len(q), len(omega), part_bytes=room)
    print("plan of 12 points, %d orbitals, 4 vectors, 10 frequencies in %d bytes:" % (n, room), plan)
    assert plan["chunk"] == 8 and (plan["batch"], plan["batches"], plan["w_pass"], plan["passes"]) == (1, 4, fit, 2)
    assert _plan(12, n, len(q), len(omega), part_bytes=16 * 12 * blocks - 1)["batch"] == 0  # not one (q, omega) fits
    assert _plan(12, n, len(q), len(omega), part_bytes=10 * 16 * 12 * blocks)["passes"] == 1
    assert (lambda p: (p["batch"], p["batches"]))(_plan(12, n, len(q), len(omega), part_bytes=25 * 16 * 12 * blocks)) == (2, 2)
    for vec in (U, None):
        whole = _from_eigensystem(mesh, eig, vec, q, T, omega, eta)
        passes = _from_eigensystem(mesh, eig, vec, q, T, omega, eta, part_bytes=room if vec is not None else fit * 16 * 12)
        assert _same(whole, passes), (n, fit, "the passes changed bits")
        for j in (fit - 1, fit):  # either side of the pass boundary: the bits of a call of its own
            assert _same(passes[:, j], _from_eigensystem(mesh, eig, vec, q, T, omega[j:j + 1], eta)[:, 0])
        want = chi_model.dynamic_susceptibility(eig, vec, mesh, q, MU, T, omega, eta, vec is not None)
        err, inside = _worst(passes, want, chi_model.dynamic_tolerance(12, n, T, eta, 2.0 * float(np.ptp(eig)) + np.abs(omega), vec is not None)[None, :])
        print("n = %d, %s, two passes: max|chi - model| = %.3e" % (n, "overlaps" if vec is not None else "pairs", err))
        assert inside
    out = np.zeros((4, 10), dtype=np.complex128)
    mesh32, q64 = np.array(mesh, dtype=np.int32), np.ascontiguousarray(q)
    assert _lib.lib().tbk_chi_dynamic_from_eigensystem(0, 3, _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), MU, T, 4, _lib.ptr(q64), None, 10, _lib.ptr(omega),
                                                       eta, 16 * 12 * blocks - 1, _lib.ptr(out)) == _lib.TBK_ERR_MEMORY


def test_extreme_chemical_potentials_give_plus_zero():
    mesh, n = (2, 3, 2), 17
    eig, U = _eigensystem(mesh, n)
    q = _vectors(mesh)[0]
    omega = _frequencies(eig[0, 0], eig[1, n - 1])
    for T in TEMPERATURES:
        for eta in ETAS:
            for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # property 5: every f (or every 1 - f) is 0
                for vec in (U, None):
                    flat = _bits(_from_eigensystem(mesh, eig, vec, q, T, omega, eta, mu=mu))
                    assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (T, eta, mu)
    small = _bits(_from_eigensystem(mesh, eig[:, :3].copy(), np.ascontiguousarray(U[:, :3, :3]), q, 0.05, omega, 1e-3, mu=-1.25 - 746.0 * 0.05))
    assert np.all(small == 0.0) and not np.any(np.signbit(small))  # (the one-tile template)


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
    q, plus, minus, shifted, duplicate = _vectors(mesh)
    kpts = dos_model.mesh_kpoints(mesh)
    eig, vec = model.eigh(kpts)
    plain = model.eigenval_array(kpts)
    level = model.fermi_level(mesh, n_el)
    omega = _frequencies(eig[0, 0], eig[chi_model.shifted_points(mesh, q[1])[0], n - 1])
    spread = 2.0 * float(np.ptp(eig)) + np.abs(omega)
    for T in TEMPERATURES:
        tol_static = chi_model.tolerance(n_k, n, T)
        for eta in ETAS:
            tol = chi_model.dynamic_tolerance(n_k, n, T, eta, spread)[None, :]
            tol_pair = chi_model.dynamic_tolerance(n_k, n, T, eta, spread, False)[None, :]
            result = model.dynamic_susceptibility(mesh, q, omega, eta=eta, temperature=T, n_electrons=n_el)
            assert isinstance(result, tbmodels_amd.DynamicSusceptibility) and result.mu == level  # bit for bit
            assert result.q.dtype == np.int64 and np.array_equal(result.q, q) and result.omega.dtype == np.float64 and np.array_equal(result.omega, omega)
            chi = result.chi
            assert chi.shape == (len(q), len(omega)) and chi.dtype == np.complex128 and np.all(np.isfinite(_bits(chi)))
            err_m, ok_m = _worst(chi, chi_model.dynamic_susceptibility(eig, vec, mesh, q, level.mu, T, omega, eta), tol)
            first = model.dynamic_susceptibility(mesh, q, omega, eta=eta, temperature=T, n_electrons=n_el, convention=1)
            assert first.mu == level and _same(first.chi[0], chi[0])  # D(0) = 1
            err_c, ok_c = _worst(first.chi, chi_model.dynamic_susceptibility(eig, vec, mesh, q, level.mu, T, omega, eta, True,
                                                                             chi_model.phase_table(mesh, q, model.pos)), tol)
            pair = model.dynamic_susceptibility(mesh, q, omega, eta=eta, temperature=T, energy=level.mu, matrix_elements=False)
            assert pair.mu.mu == level.mu
            err_p, ok_p = _worst(pair.chi, chi_model.dynamic_susceptibility(plain, None, mesh, q, level.mu, T, omega, eta, False), tol_pair)
            errs = {"1": 0.0, "2": -np.inf, "3": np.inf}
            for values, bound in ((chi, tol), (first.chi, tol), (pair.chi, tol_pair)):
                for a, b in zip(plus + [0], minus + [0]):  # property 1: chi(-q, -omega + i eta) = conj chi(q, omega + i eta)
                    err, ok = _worst(values[b][MIRROR], np.conj(values[a]), bound[0])
                    errs["1"] = max(errs["1"], err)
                    assert ok, (name, T, eta, "conjugation", err)
                for a, b in zip(plus, minus):  # property 3: omega [Im chi(q, omega) + Im chi(-q, omega)] >= 0
                    absorptive = omega * (values[a].imag + values[b].imag)
                    errs["3"] = min(errs["3"], absorptive.min())
                    assert np.all(absorptive >= -2.0 * np.abs(omega) * bound[0]), (name, T, eta, "absorptive sign")
            # property 2: 0 <= Re chi(q, i eta) <= chi_static(q) of the static call with the same arguments, both bounds as slack
            for kwargs, values, bound, bound_static in (({}, chi, tol, tol_static), ({"convention": 1}, first.chi, tol, tol_static),
                                                        ({"matrix_elements": False}, pair.chi, tol_pair, chi_model.tolerance(n_k, n, T, False))):
                static = model.susceptibility(mesh, q, temperature=T, n_electrons=n_el, **kwargs)
                assert static.mu == level
                errs["2"] = max(errs["2"], (values[:, 0].real - static.chi).max())
                assert np.all(values[:, 0].real >= -bound[0, 0]) and np.all(values[:, 0].real <= static.chi + bound[0, 0] + bound_static), (name, T, eta, kwargs)
            err_4 = np.abs(_bits(chi[0])).max()  # property 4: no response at q = 0 with matrix elements, convention 2
            assert np.all(np.abs(_bits(chi[0])) <= np.repeat(tol[0], 2))
            assert _same(chi[shifted[0]], chi[shifted[1]]) and _same(chi[duplicate[0]], chi[duplicate[1]]) and _same(chi[:, 1], chi[:, 9])  # 6 and 7
            print("%s %s T = %g eta = %g: chi - model %.3e, convention 1 - model %.3e (bound %.3e - %.3e), pairs - model %.3e (bound %.3e); conjugation "
                  "%.3e, Re chi(i eta) - static at most %.3e, omega (Im chi(q) + Im chi(-q)) at least %.3e, |chi(0, z)| at most %.3e"
                  % (name, mesh, T, eta, err_m, err_c, tol.min(), tol.max(), err_p, tol_pair.min(), errs["1"], errs["2"], errs["3"], err_4))
            assert ok_m and ok_c and ok_p
    edges = model.band_edges(mesh)
    for me in (True, False):  # property 5
        below = model.dynamic_susceptibility(mesh, q, omega, eta=1e-3, temperature=0.05, energy=float(edges.emin.min()) - 746.0 * 0.05, matrix_elements=me).chi
        assert np.all(_bits(below) == 0.0) and not np.any(np.signbit(_bits(below)))
    one = model.dynamic_susceptibility(mesh, q[1], 0.2, eta=0.05, temperature=0.05, n_electrons=n_el)  # one vector, one number
    assert one.chi.shape == (1, 1) and one.omega.shape == (1,)
    assert _same(one.chi[0, 0], model.dynamic_susceptibility(mesh, q, omega, eta=0.05, temperature=0.05, n_electrons=n_el).chi[1, 1])


def test_two_handles_give_the_bits_of_one():
    for make, mesh, n_el in (CALLS["silicon"], CALLS["dense 9, 2-D"]):
        model = make()
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        q = _vectors(mesh)[0]
        omega = np.array([0.0, 0.4, -0.4, 2.5, 0.4, -7.0, 1e6, 0.01, 0.02])
        for kwargs in ({}, {"convention": 1}, {"matrix_elements": False}):
            args = dict(eta=1e-3, temperature=0.05, n_electrons=n_el, **kwargs)
            one = model.dynamic_susceptibility(mesh, q, omega, **args)
            two = twin.dynamic_susceptibility(mesh, q, omega, **args)
            assert len(twin._handles) == 2 and two.mu == one.mu
            assert _same(one.chi, two.chi), (kwargs, np.abs(one.chi - two.chi).max())
            assert _same(one.chi[:1], twin.dynamic_susceptibility(mesh, q[:1], omega, **args).chi)  # one vector, two handles
            assert _same(one.chi, model.dynamic_susceptibility(mesh, q, omega, **args).chi)  # the same call again


# ---- 3. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_booked_with_the_static_ones_and_the_chunk_changes_no_bit():
    model = _silicon()
    q = np.array([[1, 0, 0], [2, 1, 0]], dtype=np.int64)
    omega = np.array([0.0, 3.0, 6.5])
    args = dict(eta=0.1, temperature=0.1, n_electrons=4.5)
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    plain = model.dynamic_susceptibility((4, 4, 4), q, omega, **args)  # TBK_OPT_TIMING is off
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    timed = model.dynamic_susceptibility((4, 4, 4), q, omega, **args)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 2 vectors, 3 frequencies: %d calls, Fermi tables %.3f ms, overlaps + dynamic epilogue %.3f ms, reduction %.3f ms"
          % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    assert _same(timed.chi, plain.chi) and _same(timed.chi, model.dynamic_susceptibility((4, 4, 4), q, omega, **args).chi)  # the chunk changes no bit


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U = _eigensystem((2, 3, 2), 9)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    zero = np.array([2, 0, 2], dtype=np.int32)
    q = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    omega = np.array([0.0, 0.5, -0.5])
    table = _phases(2, 9, ())
    chi, four = np.zeros((2, 3), dtype=np.complex128), np.zeros(4)
    nan, inf = float("nan"), float("inf")
    with_nan, with_inf = np.array([0.0, nan, 0.5]), np.array([0.0, 0.5, -inf])

    def call(dim=3, mesh_=mesh, n_orb=9, eig_=eig, U_=U, mu=0.0, T=0.1, n_q=2, q_=q, phases=None, n_w=3, omega_=omega, eta=0.05, room=0, out=chi):
        return lib.tbk_chi_dynamic_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), mu, T, n_q, _lib.ptr(q_), _lib.ptr(phases),
                                                    n_w, _lib.ptr(omega_), eta, room, _lib.ptr(out))

    assert call() == _lib.TBK_OK and call(U_=None) == _lib.TBK_OK and call(phases=table) == _lib.TBK_OK and call(n_w=1) == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=zero), call(mesh_=None), call(eig_=None), call(q_=None), call(out=None), call(n_orb=0),
           call(mu=nan), call(mu=inf), call(T=0.0), call(T=-0.1), call(T=nan), call(T=inf), call(n_q=0), call(n_q=-3), call(U_=None, phases=table),
           call(n_w=0), call(n_w=-1), call(n_w=2 ** 23 + 1), call(omega_=None), call(omega_=with_nan), call(omega_=with_inf), call(eta=0.0),
           call(eta=-0.05), call(eta=nan), call(eta=inf), call(eta=1e-200), call(room=-1)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    pos = np.ascontiguousarray(model.pos, dtype=np.float64)
    plan = (ctypes.c_int64 * 7)()
    m32, pq, pw, pp, p4, po = _lib.ptr(mesh), _lib.ptr(q), _lib.ptr(omega), _lib.ptr(pos), _lib.ptr(four), _lib.ptr(chi)

    def whole(handle_=handle, mesh_=m32, mode=0, value=0.0, T=0.1, n_q=2, q_=pq, n_w=3, omega_=pw, eta=0.05, me=1, convention=2, pos_=pp, mu_=p4, out=po):
        return lib.tbk_dynamic_susceptibility(handle_, mesh_, mode, value, T, n_q, q_, n_w, omega_, eta, me, convention, pos_, mu_, out)

    assert whole() == _lib.TBK_OK and whole(convention=1) == _lib.TBK_OK and whole(pos_=None) == _lib.TBK_OK and whole(me=0) == _lib.TBK_OK
    bad = [whole(handle_=None), whole(mesh_=None), whole(mode=2), whole(value=inf), whole(mode=1, value=0.0), whole(mode=1, value=8.0),
           whole(mode=1, value=nan), whole(T=0.0), whole(T=-1.0), whole(T=nan), whole(T=inf), whole(n_q=0), whole(q_=None), whole(convention=0),
           whole(convention=3), whole(convention=1, pos_=None), whole(mu_=None), whole(out=None), whole(mesh_=_lib.ptr(zero)),
           whole(n_w=0), whole(n_w=2 ** 23 + 1), whole(omega_=None), whole(omega_=_lib.ptr(with_nan)), whole(omega_=_lib.ptr(with_inf)),
           whole(eta=0.0), whole(eta=-1.0), whole(eta=nan), whole(eta=inf),
           lib.tbk_dynamic_susceptibility_multi(twice, 2, m32, 1, 4.0, 0.1, 2, pq, 3, pw, 0.05, 1, 2, pp, p4, po),
           lib.tbk_dynamic_susceptibility_multi(None, 1, m32, 1, 4.0, 0.1, 2, pq, 3, pw, 0.05, 1, 2, pp, p4, po),
           lib.tbk_chi_dynamic_plan(0, 8, 2, 3, 1, 0, plan), lib.tbk_chi_dynamic_plan(64, 0, 2, 3, 1, 0, plan), lib.tbk_chi_dynamic_plan(64, 8, 0, 3, 1, 0, plan),
           lib.tbk_chi_dynamic_plan(64, 8, 2, 0, 1, 0, plan), lib.tbk_chi_dynamic_plan(64, 8, 2, 2 ** 23 + 1, 1, 0, plan),
           lib.tbk_chi_dynamic_plan(64, 8, 2, 3, 1, -1, plan), lib.tbk_chi_dynamic_plan(64, 8, 2, 3, 1, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
