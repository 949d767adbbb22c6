"""
The complex-weighted rank-K update and slice reduction kernels of the orbital-resolved dynamic susceptibility (csrc/tbk_chi.hip,
DESIGN.md section 31) against tools/chi_model.py `dynamic_orbital_susceptibility` on identical (E, U), and
`Model.dynamic_orbital_susceptibility` against its properties and against the model fed with the eigensystem `Model.eigh` returns for
the same mesh.

Bound: chi_model.dynamic_orbital_tolerance per component of an element and per frequency -- derived from the number
formats, the sizes and allowances of 2 ulps for exp, expm1 and the quotient per side; nothing measured on the kernels enters it.
Identities of bits (properties 5, 6, 8 and 9, mu against `fermi_level`, two handles against one, batches and passes) are asserted as
such.  Every case prints its measured maximum.
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
LEVEL = 2.75  # the distance of the two flat bands, exactly representable: omega = +-LEVEL cancels their Delta for every k and q
_CACHE = {}


def _eigensystem(mesh, n):
    """Random ascending bands and random unitary U, shared by the cases and never written.  Band 0 is flat at -1.25, from four orbitals
    the last band is flat at +1.5 (g between them is not 0 at mu = 0.1: omega = LEVEL hits x = 0 exactly with g != 0), bands 1 and 2
    are an exact degenerate pair inside every k-point (three orbitals or more)."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(3100 + 41 * n_k + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
        eig[:, 0] = -1.25 if n > 1 else 0.125
        if n >= 3:
            eig[:, 2] = eig[:, 1]
        if n >= 4:
            eig[:, n - 1] = 1.5
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        for array in (eig, U):
            array.setflags(write=False)
        _CACHE[key] = (eig, U)
    return _CACHE[key]


def _vectors(mesh):
    """0, +e_0, -e_0, a vector with every component non-zero, its negative, the same shifted by whole mesh periods, a duplicate of +e_0;
    the index lists of the (q, -q) pairs, the (vector, shifted) pair and the (original, duplicate) pair."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)[:1]
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], -full[None, :], (full + shift)[None, :], unit])
    return np.ascontiguousarray(q), [0, 1, 3], [0, 2, 4], (3, 5), (1, 6)


def _chunk():
    return _plan(12, 3, 3, 1, 1)["chunk"]


MIRROR = ((0, 0), (1, 2), (2, 1), (3, 4), (4, 3))  # (omega, -omega) in the list of _frequencies


def _frequencies(count=None):
    """0, +-0.2, +-LEVEL (the exact hit), 0.7, a duplicate of 0.2, then 0.05 k: 2 CHI_OWC + 3 of them, at least seven."""
    count = max(7, 2 * _chunk() + 3) if count is None else count
    return np.concatenate([[0.0, 0.2, -0.2, LEVEL, -LEVEL, 0.7, 0.2], 0.05 * np.arange(1, max(2, count))])[:count].copy()


def _phases(n_q, n, pairs):
    """A random table of unit phases; the second row of every pair is a copy of the first."""
    angle = np.random.default_rng(377 + n).uniform(0.0, 2.0 * np.pi, (n_q, n))
    table = np.cos(angle) + 1j * np.sin(angle)
    for first, second in pairs:
        table[second] = table[first]
    return np.ascontiguousarray(table)


def _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases=None, mu=MU, orbitals=None, part_bytes=0, k_slice=0):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.int64)
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    chosen = None if orbitals is None else np.ascontiguousarray(orbitals, dtype=np.int32)
    m = n if chosen is None else len(chosen)
    out = np.full((len(q), len(omega), m, m), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_orbital_dynamic_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), float(mu),
                                                                   float(T), len(q), _lib.ptr(q), _lib.ptr(phases), m, _lib.ptr(chosen),
                                                                   len(omega), _lib.ptr(omega), float(eta), int(part_bytes), int(k_slice),
                                                                   _lib.ptr(out)))
    return out


def _plan(n_k, n_orb, m, n_q, n_w, part_bytes=0, k_slice=0):
    out = (ctypes.c_int64 * 10)()
    _lib.check(_lib.lib().tbk_chi_orbital_dynamic_plan(n_k, n_orb, m, n_q, n_w, part_bytes, k_slice, out))
    return {"template": out[0], "blocks": out[1], "k_slice": out[2], "slices": out[3], "chunk": out[4], "batch": out[5], "batches": out[6],
            "w_pass": out[7], "passes": out[8], "per_launch": out[9]}


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _worst(got, want, tol=None):
    gap = np.asarray(got) - np.asarray(want)
    worst = float(max(np.abs(gap.real).max(), np.abs(gap.imag).max()))
    if tol is None:
        return worst
    return worst, bool(np.all(np.abs(gap.real) <= tol) and np.all(np.abs(gap.imag) <= tol))


def _bound(eig, n_k, T, eta, omega):
    """`dynamic_orbital_tolerance` per frequency, shaped for [q][omega][i][j]."""
    spread = 2.0 * float(np.ptp(eig)) + np.abs(np.asarray(omega, dtype=float))
    return chi_model.dynamic_orbital_tolerance(n_k, eig.shape[-1], T, eta, spread)[None, :, None, None]


def _herm(mat):
    return (mat + np.conj(np.swapaxes(mat, -1, -2))) / 2.0


def _absorptive(mat):
    return (mat - np.conj(np.swapaxes(mat, -1, -2))) / 2.0j


def _kernel_case(mesh, n, settings=((0.05, 0.05), (0.5, 1e-3)), tables=(False, True), identities=True):
    eig, U = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, plus, minus, shifted, duplicate = _vectors(mesh)
    omega = _frequencies()
    q_order, w_order = np.random.default_rng(9).permutation(len(q)), np.random.default_rng(10).permutation(len(omega))
    report = []
    for T, eta in settings:
        bound = _bound(eig, n_k, T, eta, omega)
        for with_phases in tables:
            phases = _phases(len(q), n, (shifted, duplicate)) if with_phases else None
            where = (mesh, n, T, eta, "phases" if with_phases else "no phases")
            want = chi_model.dynamic_orbital_susceptibility(eig, U, mesh, q, MU, T, omega, eta, phases)
            got = _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases)
            err, inside = _worst(got, want, bound)
            report.append("%s T = %g eta = %g: %.3e (bound %.3e - %.3e)" % (where[4], T, eta, err, bound.min(), bound.max()))
            assert np.all(np.isfinite(_bits(got))) and inside, where + (err,)
            assert _same(got[shifted[0]], got[shifted[1]]), where + ("a whole mesh period changed bits",)  # property 6
            assert _same(got[duplicate[0]], got[duplicate[1]]) and _same(got[:, 1], got[:, 6]), where + ("a duplicate differs",)  # property 8 ...
            if not identities:
                continue
            assert _same(got, _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases)), where + ("two calls differ",)
            moved = None if phases is None else np.ascontiguousarray(phases[q_order])
            assert _same(got[q_order][:, w_order], _from_eigensystem(mesh, eig, U, q[q_order], T, omega[w_order], eta, moved)), where + ("the order changed bits",)
            for index, j in ((0, 0), (3, 3), (1, len(omega) - 1)):
                alone = _from_eigensystem(mesh, eig, U, q[index:index + 1], T, omega[j:j + 1], eta,
                                          None if phases is None else np.ascontiguousarray(phases[index:index + 1]))
                assert _same(alone[0, 0], got[index, j]), where + ("the rest of the lists changed bits",)
    return report


# ---- 1. the kernels against the model on the same (E, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16, 17, 33, 64, 65])
def test_kernels_match_the_model_on_2x3x2(n):
    n_w = len(_frequencies())
    plan = _plan(12, n, n, 7, n_w)
    assert plan["template"] == (1 if n <= 16 else 4) and plan["blocks"] == (1 if n <= 64 else 4)  # all nb^2 ordered blocks
    assert (plan["batch"], plan["batches"], plan["w_pass"], plan["passes"]) == (7, 1, n_w, 1) and plan["chunk"] in (1, 2, 4)
    assert plan["k_slice"] * plan["slices"] >= 12 > plan["k_slice"] * (plan["slices"] - 1)
    big = n > 17
    for line in _kernel_case((2, 3, 2), n, settings=((0.05, 0.05),) if big else ((0.05, 0.05), (0.5, 1e-3)), identities=n <= 64):
        print("mesh (2, 3, 2) n = %d max|chi - model|, %s" % (n, line))


def test_nine_blocks_at_129_orbitals():
    mesh, n, T, eta = (1, 2), 129, 0.05, 0.05
    assert _plan(2, n, n, 3, 3)["blocks"] == 9
    eig, U = _eigensystem(mesh, n)
    q = _vectors(mesh)[0][[1, 3, 5]]
    omega = _frequencies()[[0, 3, 5]]
    phases = _phases(3, n, ((1, 2),))
    got = _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases)
    err, inside = _worst(got, chi_model.dynamic_orbital_susceptibility(eig, U, mesh, q, MU, T, omega, eta, phases), _bound(eig, 2, T, eta, omega))
    print("mesh (1, 2) n = 129: max|chi - model| = %.3e" % err)
    assert inside and _same(got[1], got[2])


@pytest.mark.parametrize("mesh, n, wide, narrow", [((2, 3, 2), 65, [64, 3, 20], [64, 3]), ((1, 2), 257, list(range(240, 257)), [256, 250])])
def test_more_bands_than_one_round_of_weights(mesh, n, wide, narrow):
    """The weights c[omega][b'] are made for 256 (64 in the one-tile template) b' at a time: 65 bands take two rounds in the one-tile
    template, 257 two in the other and five in the one-tile template.  Selections keep the model cheap."""
    eig, U = _eigensystem(mesh, n)
    n_k, T, eta = int(np.prod(mesh)), 0.05, 0.05
    q, _, _, shifted, duplicate = _vectors(mesh)
    omega = _frequencies()
    phases = _phases(len(q), n, (shifted, duplicate))
    assert _plan(n_k, n, len(wide), len(q), len(omega))["template"] == (4 if len(wide) > 16 else 1)
    assert _plan(n_k, n, len(narrow), len(q), len(omega))["template"] == 1
    got = _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases, orbitals=wide)
    want = chi_model.dynamic_orbital_susceptibility(eig, U, mesh, q, MU, T, omega, eta, phases, wide)
    err, inside = _worst(got, want, _bound(eig, n_k, T, eta, omega))
    print("mesh %s n = %d, %d selected: max|chi - model| = %.3e" % (mesh, n, len(wide), err))
    assert inside
    small = _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases, orbitals=narrow)
    at = [wide.index(o) for o in narrow]
    assert _same(small, got[:, :, at][:, :, :, at]), (mesh, n, "the selection changed bits")  # property 9


def test_kernels_match_the_model_on_4x4x4():
    plan = _plan(64, 8, 8, 7, 7)
    assert plan["template"] == 1 and plan["slices"] >= 2  # several slices in one workgroup
    for line in _kernel_case((4, 4, 4), 8):
        print("mesh (4, 4, 4) n = 8 max|chi - model|, %s" % line)


@pytest.mark.parametrize("n", [9, 17])
def test_the_length_of_the_list_changes_no_bit(n):
    """NW = 1, CHI_OWC, CHI_OWC + 1 and 2 CHI_OWC + 3: position by position the bits of the long list, from its head and from its tail
    (another place in the register chunk)."""
    mesh, T, eta = (2, 3, 2), 0.05, 1e-3
    eig, U = _eigensystem(mesh, n)
    q = _vectors(mesh)[0][:4]
    chunk = _chunk()
    omega = _frequencies(2 * chunk + 3)
    base = _from_eigensystem(mesh, eig, U, q, T, omega, eta)
    want = chi_model.dynamic_orbital_susceptibility(eig, U, mesh, q, MU, T, omega, eta)
    assert _worst(base, want, _bound(eig, 12, T, eta, omega))[1]
    for count in (1, chunk, chunk + 1, 2 * chunk + 3):
        assert _same(_from_eigensystem(mesh, eig, U, q, T, omega[:count], eta), base[:, :count]), (n, count, "the length of the list changed bits")
        tail = _from_eigensystem(mesh, eig, U, q, T, omega[len(omega) - count:], eta)
        assert _same(tail, base[:, len(omega) - count:]), (n, count, "the place in the chunk changed bits")


def test_a_selection_has_the_bits_of_the_full_matrix():
    mesh, n, T, eta = (2, 3, 2), 33, 0.05, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, shifted, duplicate = _vectors(mesh)
    omega = _frequencies()[:4]
    rng = np.random.default_rng(91)
    for phases in (None, _phases(len(q), n, (shifted, duplicate))):
        full = _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases)
        for size in (1, 3, 16, 17):  # one tile (the other template) up to 16, the blocks of 64 from 17
            for chosen in (rng.permutation(n)[:size], np.concatenate([[n - 1], rng.permutation(n - 1)[:size - 1]])):
                assert _plan(12, n, size, len(q), len(omega))["template"] == (1 if size <= 16 else 4)
                got = _from_eigensystem(mesh, eig, U, q, T, omega, eta, phases, orbitals=chosen)
                assert got.shape == (len(q), len(omega), size, size)
                assert _same(got, full[:, :, chosen][:, :, :, chosen]), (size, chosen.tolist(), "the selection changed bits")  # property 9
        everything = rng.permutation(n)
        assert _same(_from_eigensystem(mesh, eig, U, q, T, omega, eta, phases, orbitals=everything), full[:, :, everything][:, :, :, everything])


def test_batches_and_passes_change_no_bit():
    mesh, n, T, eta = (2, 3, 2), 17, 0.05, 1e-3
    eig, U = _eigensystem(mesh, n)
    q = _vectors(mesh)[0]
    omega = _frequencies()
    n_w = len(omega)
    plan = _plan(12, n, n, len(q), n_w)
    chunk = plan["chunk"]
    per_pair = 16 * plan["slices"] * 64 * 64
    whole = _from_eigensystem(mesh, eig, U, q, T, omega, eta)
    for room in (1, 2, chunk + 1, n_w, 2 * n_w + 1):
        forced = _plan(12, n, n, len(q), n_w, part_bytes=room * per_pair + 8)
        if room >= n_w:  # whole vectors per batch
            assert (forced["batch"], forced["w_pass"], forced["passes"]) == (room // n_w, n_w, 1)
        else:  # one vector per batch, passes of whole register chunks when one fits
            want_pass = room // chunk * chunk if room >= chunk else room
            assert (forced["batch"], forced["batches"], forced["w_pass"], forced["passes"]) == (1, len(q), want_pass, -(-n_w // want_pass))
        assert forced["k_slice"] == plan["k_slice"] and forced["per_launch"] == forced["batch"] * forced["w_pass"]
        got = _from_eigensystem(mesh, eig, U, q, T, omega, eta, part_bytes=room * per_pair + 8)
        assert _same(got, whole), (room, "the batches or passes changed bits")
    assert _plan(12, n, n, len(q), n_w, part_bytes=per_pair - 8)["batch"] == 0
    out = np.zeros((len(q), n_w, n, n), dtype=np.complex128)
    mesh32 = np.array(mesh, dtype=np.int32)
    assert _lib.lib().tbk_chi_orbital_dynamic_from_eigensystem(0, 3, _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), MU, T, len(q), _lib.ptr(q), None,
                                                               n, None, n_w, _lib.ptr(omega), eta, per_pair - 8, 0,
                                                               _lib.ptr(out)) == _lib.TBK_ERR_MEMORY


def test_forced_slices_stay_within_the_bound():
    mesh, n, T, eta = (5, 5, 5), 3, 0.05, 0.05
    eig, U = _eigensystem(mesh, n)
    q = _vectors(mesh)[0]
    omega = _frequencies()[:4]
    own = _plan(125, n, n, len(q), len(omega))
    print("plan of 125 points, 3 orbitals:", own)
    assert 1 < own["k_slice"] < 125 and own["slices"] == -(-125 // own["k_slice"])
    # the library's slice length is a function of (NK, n_orb) alone
    for m, n_q, n_w, room in ((1, 1, 1, 0), (2, 4000, 3, 1 << 20), (3, 5, 600, 0), (3, 2, 9, 1 << 16)):
        assert _plan(125, n, m, n_q, n_w, part_bytes=room)["k_slice"] == own["k_slice"]
    want = chi_model.dynamic_orbital_susceptibility(eig, U, mesh, q, MU, T, omega, eta)
    bound = _bound(eig, 125, T, eta, omega)
    runs = {0: _from_eigensystem(mesh, eig, U, q, T, omega, eta)}
    assert _same(runs[0], _from_eigensystem(mesh, eig, U, q, T, omega, eta, k_slice=own["k_slice"]))
    for k_slice in (1, 5, 125):
        assert _plan(125, n, n, len(q), len(omega), k_slice=k_slice)["slices"] == -(-125 // k_slice)
        runs[k_slice] = _from_eigensystem(mesh, eig, U, q, T, omega, eta, k_slice=k_slice)
    for k_slice, got in runs.items():
        err, inside = _worst(got, want, bound)
        print("k_slice = %d: max|chi - model| = %.3e (bound %.3e)" % (k_slice, err, bound.min()))
        assert inside
        for other in runs.values():
            assert _worst(got, other, bound)[1]


def test_a_chemical_potential_outside_the_spectrum_gives_plus_zero():
    mesh, n = (2, 3, 2), 17
    eig, U = _eigensystem(mesh, n)
    q, _, _, shifted, duplicate = _vectors(mesh)
    omega = _frequencies()
    table = _phases(len(q), n, (shifted, duplicate))
    for T in (0.05, 0.5):
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # property 5
            for phases in (None, table):
                flat = _bits(_from_eigensystem(mesh, eig, U, q, T, omega, 0.05, phases, mu=mu))
                assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (T, mu)


@pytest.mark.parametrize("n", [9, 17])
def test_properties_of_the_kernels_output(n):
    mesh, T, eta = (2, 3, 2), 0.05, 0.05
    eig, U = _eigensystem(mesh, n)
    n_k = 12
    q, plus, minus, _, _ = _vectors(mesh)
    omega = _frequencies()
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    got = _from_eigensystem(mesh, eig, U, q, T, omega, eta)
    bound = _bound(eig, n_k, T, eta, omega)
    tol = float(bound.max())
    # 1. chi(-q, -omega) = conj chi(q, omega)
    for a, b in zip(plus, minus):
        for j, jm in MIRROR:
            assert _worst(got[b, jm], np.conj(got[a, j])) <= float(bound[0, j, 0, 0]), ("property 1", a, b, j)
    # 2. the sum over (i, j) is the scalar dynamic susceptibility of the same inputs
    scalar = np.full((len(q), len(omega)), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_dynamic_from_eigensystem(0, 3, _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), MU, T, len(q), _lib.ptr(q), None,
                                                           len(omega), _lib.ptr(omega), eta, 0, _lib.ptr(scalar)))
    spread = 2.0 * float(np.ptp(eig)) + np.abs(omega)
    margin = n * n * bound[:, :, 0, 0] + chi_model.dynamic_tolerance(n_k, n, T, eta, spread)[None, :]
    assert _worst(got.sum(axis=(2, 3)), scalar, margin)[1], "property 2"
    # 3. the static limit in the Loewner order
    static = np.full((len(q), n, n), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_orbital_from_eigensystem(0, 3, _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), MU, T, len(q), _lib.ptr(q), None, n,
                                                           None, 0, 0, _lib.ptr(static)))
    part = _herm(got[:, 0])
    low, gap = np.linalg.eigvalsh(part).min(), np.linalg.eigvalsh(static - part).min()
    print("n = %d: lowest eigenvalue of Herm chi(q, i eta) %.3e, of static - Herm %.3e" % (n, low, gap))
    assert low >= -n * tol and gap >= -n * (tol + chi_model.orbital_tolerance(n_k, n, T)), "property 3"
    # 4. the absorptive part
    for a, b in zip(plus, minus):
        for j, w in enumerate(omega):
            both = w * (_absorptive(got[a, j]) + _absorptive(got[b, j]).T)
            if w == 0.0:
                assert np.all(both == 0.0)
            else:
                assert np.linalg.eigvalsh(both).min() >= -n * 2.0 * abs(w) * float(bound[0, j, 0, 0]), ("property 4", a, j)


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
OMEGA = np.array([0.0, 0.3, -0.3, 1.1, 0.3])


@pytest.mark.parametrize("name", list(CALLS))
def test_properties_of_a_whole_call(name):
    make, mesh, n_el = CALLS[name]
    model = make()
    n, n_k = model.size, int(np.prod(mesh))
    q, plus, minus, shifted, duplicate = _vectors(mesh)
    eig, vec = model.eigh(dos_model.mesh_kpoints(mesh))
    level = model.fermi_level(mesh, n_el)
    chosen = np.array([n - 1, 0, 2])
    T, eta = 0.05, 0.05
    bound = _bound(eig, n_k, T, eta, OMEGA)
    result = model.dynamic_orbital_susceptibility(mesh, q, OMEGA, eta=eta, temperature=T, n_electrons=n_el)
    assert isinstance(result, tbmodels_amd.DynamicOrbitalSusceptibility) and result.mu == level  # bit for bit
    assert result.q.dtype == np.int64 and np.array_equal(result.q, q) and result.orbitals.dtype == np.int64
    assert result.omega.dtype == np.float64 and np.array_equal(result.omega, OMEGA) and np.array_equal(result.orbitals, np.arange(n))
    chi = result.chi
    assert chi.shape == (len(q), len(OMEGA), n, n) and chi.dtype == np.complex128
    err_m, inside = _worst(chi, chi_model.dynamic_orbital_susceptibility(eig, vec, mesh, q, level.mu, T, OMEGA, eta), bound)
    assert inside, (name, err_m)
    assert _same(chi[shifted[0]], chi[shifted[1]]) and _same(chi[duplicate[0]], chi[duplicate[1]]) and _same(chi[:, 1], chi[:, 4])  # 6 and 8
    for a, b in zip(plus, minus):  # property 1
        for j, jm in ((0, 0), (1, 2), (2, 1)):
            assert _worst(chi[b, jm], np.conj(chi[a, j])) <= float(bound[0, j, 0, 0])
    scalar = model.dynamic_susceptibility(mesh, q, OMEGA, eta=eta, temperature=T, n_electrons=n_el).chi  # property 2
    spread = 2.0 * float(np.ptp(eig)) + np.abs(OMEGA)
    assert _worst(chi.sum(axis=(2, 3)), scalar, n * n * bound[:, :, 0, 0] + chi_model.dynamic_tolerance(n_k, n, T, eta, spread)[None, :])[1]
    first = model.dynamic_orbital_susceptibility(mesh, q, OMEGA, eta=eta, temperature=T, energy=level.mu, convention=1)
    assert first.mu.mu == level.mu and _same(first.chi[0], chi[0])  # energy= as given; D(0) = 1
    table = chi_model.phase_table(mesh, q, model.pos)
    err_c, inside = _worst(first.chi, chi_model.dynamic_orbital_susceptibility(eig, vec, mesh, q, level.mu, T, OMEGA, eta, table), bound)
    assert inside, (name, "convention 1", err_c)
    part = model.dynamic_orbital_susceptibility(mesh, q, OMEGA, eta=eta, temperature=T, n_electrons=n_el, orbitals=chosen)
    assert np.array_equal(part.orbitals, chosen) and _same(part.chi, chi[:, :, chosen][:, :, :, chosen])  # property 9
    print("%s %s: chi - model %.3e, convention 1 - model %.3e (bound %.3e)" % (name, mesh, err_m, err_c, bound.min()))
    edges = model.band_edges(mesh)
    below = model.dynamic_orbital_susceptibility(mesh, q, OMEGA, eta=eta, temperature=T, energy=float(edges.emin.min()) - 746.0 * T).chi  # property 5
    assert np.all(_bits(below) == 0.0) and not np.any(np.signbit(_bits(below)))


def test_two_handles_give_the_bits_of_one():
    for make, mesh, n_el in (CALLS["silicon"], CALLS["dense 9, 2-D"]):
        model = make()
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        q = _vectors(mesh)[0]
        for kwargs in ({}, {"convention": 1}, {"orbitals": [3, 1]}):
            one = model.dynamic_orbital_susceptibility(mesh, q, OMEGA, eta=0.05, temperature=0.05, n_electrons=n_el, **kwargs)
            two = twin.dynamic_orbital_susceptibility(mesh, q, OMEGA, eta=0.05, temperature=0.05, n_electrons=n_el, **kwargs)
            assert len(twin._handles) == 2 and two.mu == one.mu
            assert _same(one.chi, two.chi), (kwargs, _worst(one.chi, two.chi))
            assert _same(one.chi[:1], twin.dynamic_orbital_susceptibility(mesh, q[:1], OMEGA, eta=0.05, temperature=0.05, n_electrons=n_el, **kwargs).chi)


# ---- 3. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    q = np.array([[1, 0, 0], [2, 1, 0]], dtype=np.int64)
    kwargs = dict(eta=0.05, temperature=0.1, n_electrons=4.5)
    model.dynamic_orbital_susceptibility((4, 4, 4), q, OMEGA, **kwargs)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    timed = model.dynamic_orbital_susceptibility((4, 4, 4), q, OMEGA, **kwargs)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 2 vectors, 5 frequencies: %d calls, Fermi tables %.3f ms, rank-K update %.3f ms, reduction %.3f ms"
          % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    assert _same(timed.chi, model.dynamic_orbital_susceptibility((4, 4, 4), q, OMEGA, **kwargs).chi)  # the chunk changes no bit


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U = _eigensystem((2, 3, 2), 9)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    zero = np.array([2, 0, 2], dtype=np.int32)
    q = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    table = _phases(2, 9, ())
    w = np.array([0.0, 0.4, -0.4])
    w_nan, w_inf = np.array([0.0, float("nan"), 1.0]), np.array([0.0, float("inf"), 1.0])
    some, twice_same, beyond, negative = (np.array(v, dtype=np.int32) for v in ([4, 0, 8], [4, 0, 4], [4, 9, 0], [4, -1, 0]))
    chi, four = np.zeros((2, 3, 9, 9), dtype=np.complex128), np.zeros(4)
    nan, inf = float("nan"), float("inf")

    def call(dim=3, mesh_=mesh, n_orb=9, eig_=eig, U_=U, mu=0.0, T=0.1, n_q=2, q_=q, phases=None, m=9, orbitals=None, n_w=3, w_=w, eta=0.05,
             part_bytes=0, k_slice=0, out=chi):
        return lib.tbk_chi_orbital_dynamic_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), mu, T, n_q, _lib.ptr(q_),
                                                            _lib.ptr(phases), m, _lib.ptr(orbitals), n_w, _lib.ptr(w_), eta, part_bytes, k_slice,
                                                            _lib.ptr(out))

    assert call() == _lib.TBK_OK and call(phases=table) == _lib.TBK_OK and call(m=3, orbitals=some) == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=zero), call(mesh_=None), call(eig_=None), call(U_=None), call(q_=None), call(out=None),
           call(n_orb=0), call(mu=nan), call(mu=inf), call(T=0.0), call(T=-0.1), call(T=nan), call(T=inf), call(n_q=0), call(n_q=-3), call(m=0),
           call(m=-1), call(m=10), call(m=3), call(m=3, orbitals=twice_same), call(m=3, orbitals=beyond), call(m=3, orbitals=negative),
           call(part_bytes=-1), call(k_slice=-1), call(n_w=0), call(n_w=-1), call(n_w=65536), call(w_=None), call(w_=w_nan), call(w_=w_inf),
           call(eta=0.0), call(eta=-0.05), call(eta=nan), call(eta=inf), call(eta=1e-170)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    pos = np.ascontiguousarray(model.pos, dtype=np.float64)
    plan = (ctypes.c_int64 * 10)()
    out8 = np.zeros((2, 3, 8, 8), dtype=np.complex128)
    three = np.array([7, 0, 3], dtype=np.int32)
    m32, pq, pp, p4, po, pw = _lib.ptr(mesh), _lib.ptr(q), _lib.ptr(pos), _lib.ptr(four), _lib.ptr(out8), _lib.ptr(w)

    def whole(handle_=handle, mesh_=m32, mode=0, value=0.0, T=0.1, n_q=2, q_=pq, n_w=3, w_=pw, eta=0.05, m=8, orbitals=None, convention=2, pos_=pp,
              mu_=p4, out=po):
        return lib.tbk_dynamic_orbital_susceptibility(handle_, mesh_, mode, value, T, n_q, q_, n_w, w_, eta, m, _lib.ptr(orbitals), convention, pos_,
                                                      mu_, out)

    assert whole() == _lib.TBK_OK and whole(convention=1) == _lib.TBK_OK and whole(pos_=None) == _lib.TBK_OK and whole(m=3, orbitals=three) == _lib.TBK_OK
    bad = [whole(handle_=None), whole(mesh_=None), whole(mode=2), whole(value=inf), whole(mode=1, value=0.0), whole(mode=1, value=8.0),
           whole(T=0.0), whole(T=nan), whole(n_q=0), whole(q_=None), whole(convention=0), whole(convention=1, pos_=None), whole(mu_=None),
           whole(out=None), whole(mesh_=_lib.ptr(zero)), whole(m=0), whole(m=9), whole(m=3), whole(m=3, orbitals=np.array([7, 7, 3], dtype=np.int32)),
           whole(m=3, orbitals=np.array([8, 0, 3], dtype=np.int32)), whole(n_w=0), whole(n_w=65536), whole(w_=None), whole(w_=_lib.ptr(w_nan)),
           whole(eta=0.0), whole(eta=nan), whole(eta=1e-170),
           lib.tbk_dynamic_orbital_susceptibility_multi(twice, 2, m32, 1, 4.0, 0.1, 2, pq, 3, pw, 0.05, 8, None, 2, pp, p4, po),
           lib.tbk_dynamic_orbital_susceptibility_multi(None, 1, m32, 1, 4.0, 0.1, 2, pq, 3, pw, 0.05, 8, None, 2, pp, p4, po),
           lib.tbk_chi_orbital_dynamic_plan(0, 8, 8, 2, 3, 0, 0, plan), lib.tbk_chi_orbital_dynamic_plan(64, 0, 1, 2, 3, 0, 0, plan),
           lib.tbk_chi_orbital_dynamic_plan(64, 8, 0, 2, 3, 0, 0, plan), lib.tbk_chi_orbital_dynamic_plan(64, 8, 9, 2, 3, 0, 0, plan),
           lib.tbk_chi_orbital_dynamic_plan(64, 8, 8, 0, 3, 0, 0, plan), lib.tbk_chi_orbital_dynamic_plan(64, 8, 8, 2, 0, 0, 0, plan),
           lib.tbk_chi_orbital_dynamic_plan(64, 8, 8, 2, 65536, 0, 0, plan), lib.tbk_chi_orbital_dynamic_plan(64, 8, 8, 2, 3, -1, 0, plan),
           lib.tbk_chi_orbital_dynamic_plan(64, 8, 8, 2, 3, 0, -1, plan), lib.tbk_chi_orbital_dynamic_plan(64, 8, 8, 2, 3, 0, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
