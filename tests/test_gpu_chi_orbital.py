"""
The rank-K update and slice reduction kernels of the orbital-resolved susceptibility (csrc/tbk_chi.hip) against
tools/chi_model.py `orbital_susceptibility` on identical (E, U), and `Model.orbital_susceptibility` against its properties and against
the model fed with the eigensystem `Model.eigh` returns for the same mesh.

Bound: chi_model.orbital_tolerance per component of an element -- derived from the number formats, the sizes and an
allowance of 2 ulps for exp and expm1 per side; nothing measured on the kernels enters it.  Identities of bits (exact Hermiticity,
properties 5, 6, 8 and 9, mu against `fermi_level`, two handles against one, q batches) are asserted as such.  Every case prints its
measured maximum.
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
_MODEL = {}


def _eigensystem(mesh, n):
    """`_eigensystem` of tests/test_gpu_chi.py: random ascending bands, band 0 flat, bands 1 and 2 an exact degenerate pair inside every
    k-point, random unitary U; shared by the cases and never written."""
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
    """0, +-e_d, a vector with every component non-zero, its negative, the same shifted by whole mesh periods, a duplicate of +e_0; and
    the index lists of the (q, -q) pairs, the (vector, shifted) pair and the (original, duplicate) pair."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], -full[None, :], (full + shift)[None, :], unit[:1]])
    plus, minus = list(range(1, 1 + dim)) + [1 + 2 * dim], list(range(1 + dim, 1 + 2 * dim)) + [2 + 2 * dim]
    return np.ascontiguousarray(q), plus, minus, (1 + 2 * dim, 3 + 2 * dim), (1, 4 + 2 * dim)


def _phases(n_q, n, pairs):
    """A random table of unit phases; the second row of every pair is a copy of the first."""
    angle = np.random.default_rng(277 + n).uniform(0.0, 2.0 * np.pi, (n_q, n))
    table = np.cos(angle) + 1j * np.sin(angle)
    for first, second in pairs:
        table[second] = table[first]
    return np.ascontiguousarray(table)


def _from_eigensystem(mesh, eig, U, q, T, phases=None, mu=MU, orbitals=None, part_bytes=0, k_slice=0):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.int64)
    chosen = None if orbitals is None else np.ascontiguousarray(orbitals, dtype=np.int32)
    m = n if chosen is None else len(chosen)
    out = np.full((len(q), m, m), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_orbital_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), float(mu), float(T),
                                                           len(q), _lib.ptr(q), _lib.ptr(phases), m, _lib.ptr(chosen), int(part_bytes),
                                                           int(k_slice), _lib.ptr(out)))
    return out


def _plan(n_k, n_orb, m, n_q, part_bytes=0, k_slice=0):
    out = (ctypes.c_int64 * 6)()
    _lib.check(_lib.lib().tbk_chi_orbital_plan(n_k, n_orb, m, n_q, part_bytes, k_slice, out))
    return {"template": out[0], "blocks": out[1], "k_slice": out[2], "slices": out[3], "batch": out[4], "batches": out[5]}


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _worst(got, want):
    gap = np.asarray(got) - np.asarray(want)
    return float(max(np.abs(gap.real).max(), np.abs(gap.imag).max()))


def _model_result(mesh, n, T, with_phases):
    """The NumPy model on the eleven vectors: computed once per case and shared."""
    key = (mesh, n, T, with_phases)
    if key not in _MODEL:
        eig, U = _eigensystem(mesh, n)
        q, _, _, shifted, duplicate = _vectors(mesh)
        table = _phases(len(q), n, (shifted, duplicate)) if with_phases else None
        result = chi_model.orbital_susceptibility(eig, U, mesh, q, MU, T, table)
        result.setflags(write=False)
        _MODEL[key] = result
    return _MODEL[key]


def _exactly_hermitian(chi):
    diagonal = np.ascontiguousarray(np.diagonal(chi, axis1=-2, axis2=-1).imag)
    return bool(np.array_equal(chi, np.conj(np.swapaxes(chi, -1, -2))) and np.all(diagonal == 0.0) and not np.any(np.signbit(diagonal)))


def _kernel_case(mesh, n, temperatures=TEMPERATURES, tables=(False, True), identities=True):
    eig, U = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, plus, minus, shifted, duplicate = _vectors(mesh)
    order = np.random.default_rng(9).permutation(len(q))
    report = []
    for T in temperatures:
        bound = chi_model.orbital_tolerance(n_k, n, T)
        for with_phases in tables:
            phases = _phases(len(q), n, (shifted, duplicate)) if with_phases else None
            where = (mesh, n, T, "phases" if with_phases else "no phases")
            got = _from_eigensystem(mesh, eig, U, q, T, phases)
            err = _worst(got, _model_result(mesh, n, T, with_phases))
            report.append("%s T = %g: %.3e (bound %.3e)" % (where[3], T, err, bound))
            assert np.all(np.isfinite(_bits(got))) and err <= bound, where + (err, bound)
            assert _exactly_hermitian(got), where + ("not exactly Hermitian",)
            assert _same(got[shifted[0]], got[shifted[1]]), where + ("a whole mesh period changed bits",)  # property 6
            assert _same(got[duplicate[0]], got[duplicate[1]]), where + ("a duplicate differs",)  # property 8 ...
            if not identities:
                continue
            assert _same(got, _from_eigensystem(mesh, eig, U, q, T, phases)), where + ("two calls differ",)
            moved = None if phases is None else np.ascontiguousarray(phases[order])
            assert _same(got[order], _from_eigensystem(mesh, eig, U, q[order], T, moved)), where + ("the order changed bits",)
            for index in (0, len(q) - 4):
                alone = _from_eigensystem(mesh, eig, U, q[index:index + 1], T, None if phases is None else np.ascontiguousarray(phases[index:index + 1]))
                assert _same(alone[0], got[index]), where + ("the rest of the list changed bits",)
            # properties 1 - 4 on the device's results
            lowest = np.linalg.eigvalsh(got).min()
            assert lowest >= -bound * n, where + ("not positive semidefinite", lowest)
            scalar = np.full(len(q), np.nan)
            _lib.check(_lib.lib().tbk_chi_from_eigensystem(0, len(mesh), _lib.ptr(np.ascontiguousarray(mesh, dtype=np.int32)), n, _lib.ptr(eig),
                                                           _lib.ptr(U), MU, float(T), len(q), _lib.ptr(q), _lib.ptr(phases), _lib.ptr(scalar)))
            total = got.sum(axis=(1, 2))
            margin = n * n * bound + chi_model.tolerance(n_k, n, T)
            assert np.abs(total.real - scalar).max() <= margin and np.abs(total.imag).max() <= margin, where + ("the sum rule",)
            if not with_phases:  # (a random table is not D(-q) = conj D(q))
                for a, b in zip(plus + [0], minus + [0]):
                    assert _worst(got[b], got[a].T) <= bound, where + ("chi(-q) is not the transpose", a, b)
    return report


# ---- 1. the kernels against the model on the same (E, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16, 17, 33, 64])
def test_kernels_match_the_model_on_2x3x2(n):
    plan = _plan(12, n, n, 11)
    assert plan["template"] == (1 if n <= 16 else 4) and plan["blocks"] == 1 and plan["batches"] == 1 and plan["batch"] == 11
    assert plan["k_slice"] * plan["slices"] >= 12 > plan["k_slice"] * (plan["slices"] - 1)
    for line in _kernel_case((2, 3, 2), n):
        print("mesh (2, 3, 2) n = %d max|chi - model|, %s" % (n, line))


def test_kernels_match_the_model_at_65_orbitals():
    plan = _plan(12, 65, 65, 11)
    assert plan["template"] == 4 and plan["blocks"] == 3  # the blocks (0, 0), (0, 1), (1, 1)
    for line in _kernel_case((2, 3, 2), 65, temperatures=(0.05,), tables=(True,), identities=False):
        print("mesh (2, 3, 2) n = 65 max|chi - model|, %s" % line)


def test_kernels_match_the_model_on_4x4x4():
    plan = _plan(64, 8, 8, 11)
    assert plan["template"] == 1 and plan["slices"] >= 2  # several slices in one workgroup
    for line in _kernel_case((4, 4, 4), 8):
        print("mesh (4, 4, 4) n = 8 max|chi - model|, %s" % line)


def test_a_selection_has_the_bits_of_the_full_matrix():
    mesh, n, T = (2, 3, 2), 33, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, shifted, duplicate = _vectors(mesh)
    rng = np.random.default_rng(91)
    for phases in (None, _phases(len(q), n, (shifted, duplicate))):
        full = _from_eigensystem(mesh, eig, U, q, T, phases)
        for size in (1, 3, 16, 17):  # one tile (the other template) up to 16, the blocks of 64 from 17
            for chosen in (rng.permutation(n)[:size], np.concatenate([[n - 1], rng.permutation(n - 1)[:size - 1]])):
                assert _plan(12, n, size, len(q))["template"] == (1 if size <= 16 else 4)
                got = _from_eigensystem(mesh, eig, U, q, T, phases, orbitals=chosen)
                assert got.shape == (len(q), size, size) and _exactly_hermitian(got)
                assert _same(got, full[:, chosen][:, :, chosen]), (size, chosen.tolist(), "the selection changed bits")  # property 9
        everything = rng.permutation(n)
        assert _same(_from_eigensystem(mesh, eig, U, q, T, phases, orbitals=everything), full[:, everything][:, :, everything])


@pytest.mark.parametrize("mesh, n, wide, narrow", [((2, 3, 2), 65, [64, 3, 20], [64, 3]), ((1, 2), 257, list(range(240, 257)), [256, 250])])
def test_more_bands_than_one_round_of_weights(mesh, n, wide, narrow):
    """The weights t[b][b'] are made for 256 (64 in the one-tile template) b' at a time: 65 bands take two rounds in the one-tile
    template, 257 two in the other and five in the one-tile template.  Selections keep the model cheap."""
    eig, U = _eigensystem(mesh, n)
    n_k, T = int(np.prod(mesh)), 0.05
    q, _, _, shifted, duplicate = _vectors(mesh)
    phases = _phases(len(q), n, (shifted, duplicate))
    bound = chi_model.orbital_tolerance(n_k, n, T)
    assert _plan(n_k, n, len(wide), len(q))["template"] == (4 if len(wide) > 16 else 1) and _plan(n_k, n, len(narrow), len(q))["template"] == 1
    got = _from_eigensystem(mesh, eig, U, q, T, phases, orbitals=wide)
    err = _worst(got, chi_model.orbital_susceptibility(eig, U, mesh, q, MU, T, phases, wide))
    print("mesh %s n = %d, %d selected: max|chi - model| = %.3e (bound %.3e)" % (mesh, n, len(wide), err, bound))
    assert err <= bound and _exactly_hermitian(got)
    small = _from_eigensystem(mesh, eig, U, q, T, phases, orbitals=narrow)
    at = [wide.index(o) for o in narrow]
    assert _same(small, got[:, at][:, :, at]), (mesh, n, "the selection changed bits")  # property 9


def test_q_batches_change_no_bit():
    mesh, n, T = (2, 3, 2), 17, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _, _ = _vectors(mesh)
    plan = _plan(12, n, n, len(q))
    per_vector = 16 * plan["slices"] * 64 * 64
    whole = _from_eigensystem(mesh, eig, U, q, T)
    for room in (1, 2):
        forced = _plan(12, n, n, len(q), part_bytes=room * per_vector + 8)
        assert forced["batch"] == room and forced["batches"] == (len(q) + room - 1) // room and forced["k_slice"] == plan["k_slice"]
        got = _from_eigensystem(mesh, eig, U, q, T, part_bytes=room * per_vector + 8)
        assert _same(got, whole), (room, "the batches changed bits")
        for index in (room - 1, room, len(q) - 1):  # either side of a batch boundary: the bits of a call of its own
            assert _same(got[index], _from_eigensystem(mesh, eig, U, q[index:index + 1], T)[0])
    assert _plan(12, n, n, len(q), part_bytes=per_vector - 8)["batch"] == 0
    out = np.zeros((len(q), n, n), dtype=np.complex128)
    mesh32 = np.array(mesh, dtype=np.int32)
    assert _lib.lib().tbk_chi_orbital_from_eigensystem(0, 3, _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), MU, T, len(q), _lib.ptr(q), None, n,
                                                       None, per_vector - 8, 0, _lib.ptr(out)) == _lib.TBK_ERR_MEMORY


def test_forced_slices_stay_within_the_bound():
    mesh, n, T = (5, 5, 5), 3, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _, _ = _vectors(mesh)
    own = _plan(125, n, n, len(q))
    print("plan of 125 points, 3 orbitals:", own)
    assert 1 < own["k_slice"] < 125 and 125 % own["k_slice"] != 0 and own["slices"] == -(-125 // own["k_slice"])
    assert _plan(125, n, 1, 1)["k_slice"] == own["k_slice"] == _plan(125, n, 2, 4000, part_bytes=1 << 20)["k_slice"]  # of (NK, n_orb) alone
    want = chi_model.orbital_susceptibility(eig, U, mesh, q, MU, T)
    bound = chi_model.orbital_tolerance(125, n, T)
    runs = {0: _from_eigensystem(mesh, eig, U, q, T)}
    assert _same(runs[0], _from_eigensystem(mesh, eig, U, q, T)) and _same(runs[0], _from_eigensystem(mesh, eig, U, q, T, k_slice=own["k_slice"]))
    for k_slice in (1, 5, 125):
        assert _plan(125, n, n, len(q), k_slice=k_slice)["slices"] == -(-125 // k_slice)
        runs[k_slice] = _from_eigensystem(mesh, eig, U, q, T, k_slice=k_slice)
    for k_slice, got in runs.items():
        print("k_slice = %d: max|chi - model| = %.3e (bound %.3e)" % (k_slice, _worst(got, want), bound))
        assert _worst(got, want) <= bound and _exactly_hermitian(got)
        for other in runs.values():
            assert _worst(got, other) <= bound


def test_extreme_temperatures_and_chemical_potentials():
    mesh, n = (2, 3, 2), 17
    eig, U = _eigensystem(mesh, n)
    q, _, _, shifted, duplicate = _vectors(mesh)
    table = _phases(len(q), n, (shifted, duplicate))
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # property 5
            for phases in (None, table):
                flat = _bits(_from_eigensystem(mesh, eig, U, q, T, phases, mu=mu))
                assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (T, mu)
    hot = 1e9 * float(np.ptp(eig))
    for phases in (None, table):  # property 4
        got = _from_eigensystem(mesh, eig, U, q, hot, phases)
        err, bound = _worst(4.0 * hot * got, np.eye(n)[None]), 4.0 * hot * chi_model.orbital_tolerance(12, n, hot) + 1e-8
        print("T = 1e9 bandwidths: max|4 T chi - 1| = %.3e (bound %.3e)" % (err, bound))
        assert err <= bound


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
    eig, vec = model.eigh(dos_model.mesh_kpoints(mesh))
    level = model.fermi_level(mesh, n_el)
    chosen = np.array([n - 1, 0, 2])
    for T in TEMPERATURES:
        tol = chi_model.orbital_tolerance(n_k, n, T)
        result = model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el)
        assert isinstance(result, tbmodels_amd.OrbitalSusceptibility) and result.mu == level  # bit for bit
        assert result.q.dtype == np.int64 and np.array_equal(result.q, q) and result.orbitals.dtype == np.int64
        assert np.array_equal(result.orbitals, np.arange(n)) and result.chi.shape == (len(q), n, n) and result.chi.dtype == np.complex128
        chi = result.chi
        assert _exactly_hermitian(chi) and np.linalg.eigvalsh(chi).min() >= -tol * n  # property 1
        err_m = _worst(chi, chi_model.orbital_susceptibility(eig, vec, mesh, q, level.mu, T))
        scalar = model.susceptibility(mesh, q, temperature=T, n_electrons=n_el).chi
        err_2 = np.abs(chi.sum(axis=(1, 2)) - scalar).max() / (n * n * tol + chi_model.tolerance(n_k, n, T))  # property 2
        err_3 = max(_worst(chi[b], chi[a].T) for a, b in zip(plus, minus))  # property 3
        assert _same(chi[shifted[0]], chi[shifted[1]]) and _same(chi[duplicate[0]], chi[duplicate[1]])  # properties 6 and 8
        first = model.orbital_susceptibility(mesh, q, temperature=T, energy=level.mu, convention=1)
        assert first.mu.mu == level.mu and _exactly_hermitian(first.chi) and _same(first.chi[0], chi[0])  # D(0) = 1
        err_c = _worst(first.chi, chi_model.orbital_susceptibility(eig, vec, mesh, q, level.mu, T, chi_model.phase_table(mesh, q, model.pos)))
        err_c3 = max(_worst(first.chi[b], first.chi[a].T) for a, b in zip(plus, minus))
        part = model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el, orbitals=chosen)
        assert np.array_equal(part.orbitals, chosen) and _same(part.chi, chi[:, chosen][:, :, chosen])  # property 9
        print("%s %s T = %g: chi - model %.3e, chi(-q) - chi(q)^T %.3e, convention 1 - model %.3e, its inversion %.3e (bound %.3e); "
              "sum rule %.3e of its margin" % (name, mesh, T, err_m, err_3, err_c, err_c3, tol, err_2))
        assert max(err_m, err_3, err_c, err_c3) <= tol and err_2 <= 1.0
    edges = model.band_edges(mesh)
    below = model.orbital_susceptibility(mesh, q, temperature=0.05, energy=float(edges.emin.min()) - 746.0 * 0.05).chi  # property 5
    assert np.all(_bits(below) == 0.0) and not np.any(np.signbit(_bits(below)))


def test_two_handles_give_the_bits_of_one():
    for make, mesh, n_el in (CALLS["silicon"], CALLS["dense 9, 2-D"]):
        model = make()
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        q, _, _, _, _ = _vectors(mesh)
        for kwargs in ({}, {"convention": 1}, {"orbitals": [3, 1]}):
            one = model.orbital_susceptibility(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs)
            two = twin.orbital_susceptibility(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs)
            assert len(twin._handles) == 2 and two.mu == one.mu
            assert _same(one.chi, two.chi), (kwargs, _worst(one.chi, two.chi))
            assert _same(one.chi[:1], twin.orbital_susceptibility(mesh, q[:1], temperature=0.05, n_electrons=n_el, **kwargs).chi)
            assert _same(one.chi, model.orbital_susceptibility(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs).chi)  # the same call again


# ---- 3. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    q = np.array([[1, 0, 0], [2, 1, 0]], dtype=np.int64)
    model.orbital_susceptibility((4, 4, 4), q, temperature=0.1, n_electrons=4.5)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    timed = model.orbital_susceptibility((4, 4, 4), q, temperature=0.1, n_electrons=4.5)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 2 vectors: %d calls, Fermi tables %.3f ms, rank-K update %.3f ms, reduction %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    assert _same(timed.chi, model.orbital_susceptibility((4, 4, 4), q, temperature=0.1, n_electrons=4.5).chi)  # the chunk changes no bit


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U = _eigensystem((2, 3, 2), 9)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    zero = np.array([2, 0, 2], dtype=np.int32)
    q = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    table = _phases(2, 9, ())
    some, twice_same, beyond, negative = (np.array(v, dtype=np.int32) for v in ([4, 0, 8], [4, 0, 4], [4, 9, 0], [4, -1, 0]))
    chi, four = np.zeros((2, 9, 9), dtype=np.complex128), np.zeros(4)
    nan, inf = float("nan"), float("inf")

    def call(dim=3, mesh_=mesh, n_orb=9, eig_=eig, U_=U, mu=0.0, T=0.1, n_q=2, q_=q, phases=None, m=9, orbitals=None, part_bytes=0, k_slice=0, out=chi):
        return lib.tbk_chi_orbital_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), mu, T, n_q, _lib.ptr(q_),
                                                    _lib.ptr(phases), m, _lib.ptr(orbitals), part_bytes, k_slice, _lib.ptr(out))

    assert call() == _lib.TBK_OK and call(phases=table) == _lib.TBK_OK and call(m=3, orbitals=some) == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=zero), call(mesh_=None), call(eig_=None), call(U_=None), call(q_=None), call(out=None),
           call(n_orb=0), call(mu=nan), call(mu=inf), call(T=0.0), call(T=-0.1), call(T=nan), call(T=inf), call(n_q=0), call(n_q=-3), call(m=0),
           call(m=-1), call(m=10), call(m=3), call(m=3, orbitals=twice_same), call(m=3, orbitals=beyond), call(m=3, orbitals=negative),
           call(part_bytes=-1), call(k_slice=-1)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    pos = np.ascontiguousarray(model.pos, dtype=np.float64)
    plan = (ctypes.c_int64 * 6)()
    out8 = np.zeros((2, 8, 8), dtype=np.complex128)
    three = np.array([7, 0, 3], dtype=np.int32)
    m32, pq, pp, p4, po = _lib.ptr(mesh), _lib.ptr(q), _lib.ptr(pos), _lib.ptr(four), _lib.ptr(out8)

    def whole(handle_=handle, mesh_=m32, mode=0, value=0.0, T=0.1, n_q=2, q_=pq, m=8, orbitals=None, convention=2, pos_=pp, mu_=p4, out=po):
        return lib.tbk_orbital_susceptibility(handle_, mesh_, mode, value, T, n_q, q_, m, _lib.ptr(orbitals), convention, pos_, mu_, out)

    assert whole() == _lib.TBK_OK and whole(convention=1) == _lib.TBK_OK and whole(pos_=None) == _lib.TBK_OK and whole(m=3, orbitals=three) == _lib.TBK_OK
    bad = [whole(handle_=None), whole(mesh_=None), whole(mode=2), whole(value=inf), whole(mode=1, value=0.0), whole(mode=1, value=8.0),
           whole(T=0.0), whole(T=nan), whole(n_q=0), whole(q_=None), whole(convention=0), whole(convention=1, pos_=None), whole(mu_=None),
           whole(out=None), whole(mesh_=_lib.ptr(zero)), whole(m=0), whole(m=9), whole(m=3), whole(m=3, orbitals=np.array([7, 7, 3], dtype=np.int32)),
           whole(m=3, orbitals=np.array([8, 0, 3], dtype=np.int32)),
           lib.tbk_orbital_susceptibility_multi(twice, 2, m32, 1, 4.0, 0.1, 2, pq, 8, None, 2, pp, p4, po),
           lib.tbk_orbital_susceptibility_multi(None, 1, m32, 1, 4.0, 0.1, 2, pq, 8, None, 2, pp, p4, po),
           lib.tbk_chi_orbital_plan(0, 8, 8, 2, 0, 0, plan), lib.tbk_chi_orbital_plan(64, 0, 1, 2, 0, 0, plan),
           lib.tbk_chi_orbital_plan(64, 8, 0, 2, 0, 0, plan), lib.tbk_chi_orbital_plan(64, 8, 9, 2, 0, 0, plan),
           lib.tbk_chi_orbital_plan(64, 8, 8, 0, 0, 0, plan), lib.tbk_chi_orbital_plan(64, 8, 8, 2, -1, 0, plan),
           lib.tbk_chi_orbital_plan(64, 8, 8, 2, 0, -1, plan), lib.tbk_chi_orbital_plan(64, 8, 8, 2, 0, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
