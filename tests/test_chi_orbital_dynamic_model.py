"""
tools/chi_model.py `dynamic_orbital_susceptibility`, the NumPy statement of the orbital-resolved bare dynamic susceptibility
chi_0[i, j](q, omega + i eta), against the nine properties that define the quantity, the formula as written,
and the argument checks of `Model.dynamic_orbital_susceptibility`, which need no device.

Inputs: random ascending bands with a flat band (two from four orbitals), an exact degenerate pair in every k-point and random unitary
U, on the meshes 2 x 3 x 2, 3 x 4, 1 x 5 and 1 x 1 x 1 with 1, 3 and 9 orbitals, mu inside the bands, T in {0.05, 0.5}, eta in {0.25,
1e-3}, both conventions with random positions.  The frequencies hold 0, both signs, a duplicate and LEVEL, the exactly representable
distance of the two flat bands: x = Delta + omega = 0 with g != 0.  Bound: chi_model.dynamic_orbital_tolerance per
component of an element and per frequency for every comparison of two evaluations; the NumPy model hands the n^4 part to BLAS, so
among the identities of bits only those that repeat the same products (properties 5, 6, 8) are asserted as such on it, and property
9 within the bound -- the kernels' test asserts it bit for bit.
"""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chi_model  # noqa: E402  pylint: disable=wrong-import-position

MESHES = [(2, 3, 2), (3, 4), (1, 5), (1, 1, 1)]
ORBITALS = [1, 3, 9]
TEMPERATURES = [0.05, 0.5]
ETAS = [0.25, 1e-3]
MU = 0.1
LEVEL = 2.75
OMEGA = np.array([0.0, 0.2, -0.2, LEVEL, -LEVEL, 0.7, 0.2])
MIRROR = ((0, 0), (1, 2), (2, 1), (3, 4), (4, 3))  # (omega, -omega) in OMEGA
_CACHE = {}
_CHI = {}


def _eigensystem(mesh, n):
    """Band 0 flat at -1.25, from four orbitals the last band flat at +1.5, bands 1 and 2 an exact degenerate pair, random unitary U;
    and random positions.  Computed once, never written."""
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
        pos = rng.uniform(0.0, 1.0, size=(n, len(mesh)))
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        for array in (eig, U, pos):
            array.setflags(write=False)
        _CACHE[key] = (eig, U, pos)
    return _CACHE[key]


def _vectors(mesh):
    """0, +e_0, -e_0, a vector with every component non-zero, its negative, the same shifted by whole mesh periods, a duplicate of +e_0."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)[:1]
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], -full[None, :], (full + shift)[None, :], unit])
    return np.ascontiguousarray(q), {"plus": [0, 1, 3], "minus": [0, 2, 4], "full": 3, "shifted": 5, "duplicate": (1, 6)}


def _chi(mesh, n, T, eta, convention, q=None, omega=OMEGA, mu=MU, U=None, orbitals=None):
    """The model; the plain case (the seven vectors, OMEGA, the stored U, no selection) is computed once and shared."""
    eig, vec, pos = _eigensystem(mesh, n)
    plain = q is None and omega is OMEGA and mu == MU and U is None and orbitals is None
    key = (mesh, n, T, eta, convention)
    if plain and key in _CHI:
        return _CHI[key]
    q = _vectors(mesh)[0] if q is None else q
    phases = chi_model.phase_table(mesh, q, pos) if convention == 1 else None
    out = chi_model.dynamic_orbital_susceptibility(eig, vec if U is None else U, mesh, q, mu, T, omega, eta, phases, orbitals)
    if plain:
        out.setflags(write=False)
        _CHI[key] = out
    return out


def _tol(mesh, n, T, eta, omega=OMEGA):
    eig = _eigensystem(mesh, n)[0]
    spread = 2.0 * float(np.ptp(eig)) + np.abs(omega)
    return chi_model.dynamic_orbital_tolerance(int(np.prod(mesh)), n, T, eta, spread)


def _parts(z):
    z = np.asarray(z)
    return max(np.abs(z.real).max(), np.abs(z.imag).max())


def _inside(gap, tol):
    """Both components of [q][omega][i][j] within the bound per frequency."""
    tol = np.asarray(tol)[None, :, None, None]
    return bool(np.all(np.abs(gap.real) <= tol) and np.all(np.abs(gap.imag) <= tol))


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _herm(mat):
    return (mat + np.conj(np.swapaxes(mat, -1, -2))) / 2.0


def _absorptive(mat):
    return (mat - np.conj(np.swapaxes(mat, -1, -2))) / 2.0j


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_inversion_sum_rule_static_limit_and_absorptive_part(mesh, n):
    eig, vec, pos = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    spread = 2.0 * float(np.ptp(eig)) + np.abs(OMEGA)
    worst = [0.0, 0.0, np.inf, np.inf, np.inf]
    for T in TEMPERATURES:
        for eta in ETAS:
            tol = _tol(mesh, n, T, eta)
            for convention in (1, 2):
                chi = _chi(mesh, n, T, eta, convention)
                where = (mesh, n, T, eta, convention)
                assert chi.shape == (len(q), len(OMEGA), n, n) and chi.dtype == np.complex128 and np.all(np.isfinite(_bits(chi)))
                # property 1: chi(-q, -omega + i eta) = conj chi(q, omega + i eta); q = 0 is its own partner
                for a, b in zip(at["plus"], at["minus"]):
                    for j, jm in MIRROR:
                        gap = _parts(chi[b, jm] - np.conj(chi[a, j]))
                        worst[0] = max(worst[0], gap / tol[j])
                        assert gap <= tol[j], where + ("property 1", a, b, j, gap)
                # property 2: the sum over (i, j) is the scalar chi_0(q, z) with matrix elements
                phases = chi_model.phase_table(mesh, q, pos) if convention == 1 else None
                scalar = chi_model.dynamic_susceptibility(eig, vec, mesh, q, MU, T, OMEGA, eta, True, phases)
                margin = n * n * tol + chi_model.dynamic_tolerance(n_k, n, T, eta, spread)
                gap = chi.sum(axis=(2, 3)) - scalar
                worst[1] = max(worst[1], (np.maximum(np.abs(gap.real), np.abs(gap.imag)) / margin[None, :]).max())
                assert np.all(np.abs(gap.real) <= margin[None, :]) and np.all(np.abs(gap.imag) <= margin[None, :]), where + ("property 2",)
                # property 3: 0 <= Herm chi(q, i eta) <= the static matrix in the Loewner order (OMEGA[0] = 0)
                static = chi_model.orbital_susceptibility(eig, vec, mesh, q, MU, T, phases)
                part = _herm(chi[:, 0])
                low, room = np.linalg.eigvalsh(part).min(), np.linalg.eigvalsh(static - part).min()
                worst[2], worst[3] = min(worst[2], low), min(worst[3], room)
                assert low >= -n * tol[0], where + ("property 3: Herm chi(q, i eta) is not positive semidefinite", low)
                assert room >= -n * (tol[0] + chi_model.orbital_tolerance(n_k, n, T)), where + ("property 3: static - Herm", room)
                # property 4: the absorptive part has one sign, and is exactly 0 at omega = 0
                for a, b in zip(at["plus"], at["minus"]):
                    for j, w in enumerate(OMEGA):
                        both = w * (_absorptive(chi[a, j]) + _absorptive(chi[b, j]).T)
                        if w == 0.0:
                            assert np.all(both == 0.0), where + ("property 4 at omega = 0",)
                        else:
                            low = np.linalg.eigvalsh(both).min()
                            worst[4] = min(worst[4], low)
                            assert low >= -n * 2.0 * abs(w) * tol[j], where + ("property 4", a, j, low)
                            diagonal = np.diagonal(both).real  # 16.1's property 3 per orbital
                            assert np.all(diagonal >= -2.0 * abs(w) * tol[j]), where + ("property 4, diagonal",)
    print("mesh %s n = %d: inversion %.2e and sum rule %.2e of the bound; lowest eigenvalues: Herm %.3e, static - Herm %.3e, absorptive %.3e"
          % (mesh, n, worst[0], worst[1], worst[2], worst[3], worst[4]))


def test_the_static_limit_is_not_vacuous():
    """Property 3 on an input where it says something: on 2 x 3 x 2 with 9 orbitals the static matrix exceeds Herm chi(q, i eta) by
    far more than the allowance at eta = 0.25 (the Lorentzian factor Delta^2 / (Delta^2 + eta^2) bites) and, through the f' terms of
    the exactly degenerate pair and the flat bands at q = 0, also at eta = 1e-3; and the difference is positive semidefinite."""
    mesh, n, T = (2, 3, 2), 9, 0.05
    eig, vec, _ = _eigensystem(mesh, n)
    q = _vectors(mesh)[0]
    static = chi_model.orbital_susceptibility(eig, vec, mesh, q, MU, T)
    for eta in ETAS:
        tol = _tol(mesh, n, T, eta)[0] + chi_model.orbital_tolerance(12, n, T)
        part = _herm(_chi(mesh, n, T, eta, 2)[:, 0])
        values = np.linalg.eigvalsh(static - part)
        print("eta = %g: eigenvalues of static - Herm chi(q, i eta) from %.3e to %.3e (allowance %.3e)" % (eta, values.min(), values.max(), n * tol))
        assert values.min() >= -n * tol
        assert values[0].max() > 1e6 * n * tol  # q = 0: every pair inside a k-point, the degenerate ones carry f' on the static side only
        if eta == 0.25:
            assert values.max(axis=1).min() > 1e6 * n * tol  # every vector


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_far_outside_the_spectrum_every_bit_is_zero(mesh, n):
    eig, _, _ = _eigensystem(mesh, n)
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):
            for convention in (1, 2):
                flat = _bits(_chi(mesh, n, T, ETAS[0], convention, mu=mu))
                assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (mesh, n, T, mu, convention)  # property 5


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_column_phases_and_the_basis_of_a_degenerate_pair_do_not_matter(mesh, n):
    eig, vec, _ = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    rng = np.random.default_rng(55 + n)
    angle = rng.uniform(0.0, 2.0 * np.pi, (n_k, 1, n))
    turned = vec * (np.cos(angle) + 1j * np.sin(angle))
    if n >= 3:  # bands 1 and 2 are degenerate in every k-point: any unitary mix of the two columns is an eigenbasis
        mix = np.linalg.qr(rng.normal(size=(n_k, 2, 2)) + 1j * rng.normal(size=(n_k, 2, 2)))[0]
        turned = turned.copy()
        turned[:, :, 1:3] = np.einsum("kib,kbc->kic", turned[:, :, 1:3], mix)
    for T in TEMPERATURES:
        for eta in ETAS:
            for convention in (1, 2):
                gap = _chi(mesh, n, T, eta, convention) - _chi(mesh, n, T, eta, convention, U=turned)  # property 7
                # the turned eigenvectors are another input, each of its entries off by a few u: twice the bound covers both evaluations
                assert _inside(gap, 2.0 * _tol(mesh, n, T, eta) + 16 * n * 2.0 ** -53 / eta), (mesh, n, T, eta, convention, _parts(gap))


# selections for property 9 that fit n: a single orbital, a shuffled subset with the last orbital, a pair, all of them reversed
SELECTIONS = {1: ([0],), 3: ([1], [2, 0], [2, 1, 0]), 9: ([4], [8, 0, 3], [2, 1], list(range(8, -1, -1)))}


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_bits_do_not_depend_on_the_lists_and_selections_agree(mesh, n):
    q, at = _vectors(mesh)
    T = TEMPERATURES[0]
    q_order, w_order = np.random.default_rng(3).permutation(len(q)), np.random.default_rng(4).permutation(len(OMEGA))
    for eta in ETAS:
        tol = _tol(mesh, n, T, eta)
        for convention in (1, 2):
            chi = _chi(mesh, n, T, eta, convention)
            assert np.array_equal(_bits(chi[at["duplicate"][0]]), _bits(chi[at["duplicate"][1]]))  # property 8
            assert np.array_equal(_bits(chi[:, 1]), _bits(chi[:, 6]))
            again = _chi(mesh, n, T, eta, convention, q=np.ascontiguousarray(q[q_order]), omega=OMEGA[w_order])
            assert np.array_equal(_bits(chi[q_order][:, w_order]), _bits(again))
            for index, j in ((0, 0), (len(q) - 3, 3)):
                alone = _chi(mesh, n, T, eta, convention, q=q[index:index + 1], omega=OMEGA[j:j + 1])
                assert np.array_equal(_bits(alone[0, 0]), _bits(chi[index, j]))
            if convention == 2:
                assert np.array_equal(_bits(chi[at["full"]]), _bits(chi[at["shifted"]]))  # property 6
            for chosen in SELECTIONS[n]:  # property 9 (the model: within the bound)
                part = _chi(mesh, n, T, eta, convention, orbitals=chosen)
                assert part.shape == (len(q), len(OMEGA), len(chosen), len(chosen))
                assert _inside(part - chi[:, :, chosen][:, :, :, chosen], tol), (mesh, n, eta, convention, chosen)
    eig, vec, _ = _eigensystem(mesh, n)
    for function in (chi_model.dynamic_orbital_susceptibility, chi_model.dynamic_orbital_susceptibility_naive):  # the two validate alike
        for bad in ([], [0, 0], [n], [-1], [0.0], [[0, 0]]):
            with pytest.raises(ValueError):
                function(eig, vec, mesh, q, MU, T, OMEGA, 0.25, None, bad)
        for omega, eta in (([np.nan], 0.25), ([], 0.25), ([[0.0]], 0.25), (OMEGA, 0.0), (OMEGA, -1.0), (OMEGA, np.inf), (OMEGA, 1e-170)):
            with pytest.raises(ValueError):
                function(eig, vec, mesh, q, MU, T, omega, eta)
    with pytest.raises(ValueError):
        chi_model.dynamic_orbital_susceptibility(eig, vec, mesh, q.astype(float), MU, T, OMEGA, 0.25)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_model_against_the_formula_as_written(mesh, n):
    """The formula in complex arithmetic with f(a) - f(b) as the difference of two Fermi functions.  Condition, as in
    tests/test_chi_dynamic_model.py: |E - mu| / T < 709 for every state, so that no exponential of the plain Fermi function overflows,
    and the comparison is of ABSOLUTE errors: the difference as written is off by under 17 u however small it is, the complex quotient
    and the products with the amplitudes by another 8 u of the term plus the amplitudes' own 14 -- under the 51 u that
    dynamic_orbital_tolerance charges per unit of sum |A_i| |A_j| / eta <= 1 / eta, because its relative terms are taken at |g| = 1.
    So the bound holds for this evaluation at every pair."""
    eig, vec, pos = _eigensystem(mesh, n)
    q, _ = _vectors(mesh)
    assert np.abs(eig - MU).max() / min(TEMPERATURES) < 709.0
    worst = 0.0
    for T in TEMPERATURES:
        for eta in ETAS:
            tol = _tol(mesh, n, T, eta)
            for convention in (1, 2):
                phases = chi_model.phase_table(mesh, q, pos) if convention == 1 else None
                want = chi_model.dynamic_orbital_susceptibility_naive(eig, vec, mesh, q, MU, T, OMEGA, eta, phases)
                gap = _chi(mesh, n, T, eta, convention) - want
                worst = max(worst, (np.maximum(np.abs(gap.real), np.abs(gap.imag)) / tol[None, :, None, None]).max())
                assert _inside(gap, tol), (mesh, n, T, eta, convention, _parts(gap))
    print("mesh %s n = %d: max |model - formula as written| / bound = %.3e" % (mesh, n, worst))


def test_a_frequency_on_a_transition_is_finite():
    mesh, n, T = (2, 3, 2), 9, 0.05
    eig, vec, _ = _eigensystem(mesh, n)
    q, _ = _vectors(mesh)
    f, g = chi_model.fermi_tables(eig, MU, T)
    assert np.all((eig[:, 0] - eig[:, n - 1]) + LEVEL == 0.0)  # x = 0 exactly for the two flat bands, whatever k and q
    assert abs(chi_model.pair_difference(eig[0, 0], eig[1, n - 1], f[0, 0], g[0, 0], f[1, n - 1], g[1, n - 1], T)) > 0.9  # ... with g != 0
    for eta in ETAS:
        chi = _chi(mesh, n, T, eta, 2)[:, 3:5]
        assert np.all(np.isfinite(_bits(chi)))
        assert _parts(chi) > 0.01 / eta / n / n  # the hit carries g / eta of one pair's amplitudes


def test_the_tolerance_is_the_documented_formula():
    u = 2.0 ** -53
    n_k, n, T, eta = 12, 9, 0.05, 0.25
    spread = np.array([4.0, 5.5])
    assert chi_model.ROUNDINGS_COMPLEX_SCALE == 3 and chi_model.ROUNDINGS_AMPLITUDES == 14 and chi_model.ULP_DIV == 2
    want = 2 * (n_k * n * n + (4 * 2 + 2 + 2 + 18 + 14 + 3) + 4 + spread / eta) * u / eta
    assert np.allclose(chi_model.dynamic_orbital_tolerance(n_k, n, T, eta, spread), want, rtol=1e-14)
    assert np.allclose(want, 2 * (n_k * n * n + 51 + spread / eta) * u / eta, rtol=1e-14)
    assert chi_model.dynamic_orbital_tolerance(n_k, n, 7.0, eta, 4.0) == chi_model.dynamic_orbital_tolerance(n_k, n, T, eta, 4.0)  # T does not enter


# ---- the public interface -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("tbk_chi_orbital_dynamic_from_eigensystem", "tbk_dynamic_orbital_susceptibility", "tbk_dynamic_orbital_susceptibility_multi",
               "tbk_chi_orbital_dynamic_plan")


def test_the_built_library_has_the_new_symbols():
    library = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(library, name), name


def test_the_plan_needs_no_device():
    out = (ctypes.c_int64 * 10)()
    library = _lib.lib()
    assert library.tbk_chi_orbital_dynamic_plan(12, 17, 17, 7, 7, 0, 0, out) == _lib.TBK_OK
    template, blocks, k_slice, slices, chunk, batch, batches, w_pass, passes, per_launch = list(out)
    assert (template, blocks, batch, batches, w_pass, passes, per_launch) == (4, 1, 7, 1, 7, 1, 49) and chunk in (1, 2, 4)
    assert k_slice * slices >= 12 > k_slice * (slices - 1)
    assert library.tbk_chi_orbital_dynamic_plan(12, 65, 65, 7, 7, 0, 0, out) == _lib.TBK_OK and (out[0], out[1]) == (4, 4)  # all nb^2 blocks
    assert library.tbk_chi_orbital_dynamic_plan(12, 65, 16, 7, 7, 0, 0, out) == _lib.TBK_OK and (out[0], out[1]) == (1, 1)
    static = (ctypes.c_int64 * 6)()
    assert library.tbk_chi_orbital_plan(12, 65, 65, 7, 0, 0, static) == _lib.TBK_OK and static[1] == 3  # the static call keeps bi <= bj
    # the grid: with 65535 frequencies a vector has 65535 / chunk register chunks, so one or two vectors go into a launch
    assert library.tbk_chi_orbital_dynamic_plan(12, 3, 3, 50, 65535, 1 << 40, 0, out) == _lib.TBK_OK
    assert out[7] == 65535 and out[5] == 65535 // -(-65535 // chunk) and out[5] * -(-65535 // chunk) <= 65535
    assert library.tbk_chi_orbital_dynamic_plan(12, 3, 3, 50, 65536, 0, 0, out) == _lib.TBK_ERR_ARGUMENT


def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    q, w = [[1, 0, 0]], [0.0, 0.5]
    call = model.dynamic_orbital_susceptibility
    for kwargs in ({}, {"energy": 0.0, "n_electrons": 4}, {"energy": np.nan}, {"energy": "0"}, {"n_electrons": 0}, {"n_electrons": 8},
                   {"n_electrons": np.nan}, {"n_electrons": "4"}):
        with pytest.raises(ValueError):
            call((2, 2, 2), q, w, eta=0.1, temperature=0.1, **kwargs)
    for bad in (None, np.zeros((2, 3)), [[0.5, 0, 0]], np.zeros((2, 2), dtype=int), [0, 1], np.zeros((0, 3), dtype=int), "000", [[0, 0, 2 ** 70]],
                np.zeros((1, 3), dtype=bool)):
        with pytest.raises(ValueError):
            call((2, 2, 2), bad, w, eta=0.1, temperature=0.1, energy=0.0)
    for bad in ([], [0, 0], [8], [-1], [0.0, 1.0], [[0, 1]], "01", [True, False], [None], np.zeros((0,), dtype=int), [2 ** 70], {"orbitals": 1},
                np.array([1], dtype=np.uint64)):
        with pytest.raises(ValueError):
            call((2, 2, 2), q, w, eta=0.1, temperature=0.1, energy=0.0, orbitals=bad)
    for bad in (None, [], [[0.0, 1.0]], "0.5", [np.nan], [np.inf], [1j], [None], np.zeros(65536)):
        with pytest.raises(ValueError):
            call((2, 2, 2), q, bad, eta=0.1, temperature=0.1, energy=0.0)
    for eta in (0.0, -0.1, np.nan, np.inf, "0.1", None, True, 1e-170):
        with pytest.raises(ValueError):
            call((2, 2, 2), q, w, eta=eta, temperature=0.1, energy=0.0)
    for temperature in (0.0, -0.1, np.nan, np.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            call((2, 2, 2), q, w, eta=0.1, temperature=temperature, energy=0.0)
    for mesh in ((4, 4), (4, 0, 4), (4.0, 4.0, 4.0), 4):
        with pytest.raises(ValueError):
            call(mesh, q, w, eta=0.1, temperature=0.1, n_electrons=4)
    for kwargs in ({"convention": 0}, {"convention": 3}, {"convention": "2"}):
        with pytest.raises(ValueError):
            call((2, 2, 2), q, w, eta=0.1, temperature=0.1, energy=0.0, **kwargs)
    with pytest.raises(TypeError):
        call((2, 2, 2), q, w, eta=0.1, temperature=0.1, energy=0.0, matrix_elements=False)  # there is no such form
    with pytest.raises(TypeError):
        call((2, 2, 2), q, w, 0.1, temperature=0.1, energy=0.0)  # eta is keyword only
    with pytest.raises(TypeError):
        call((2, 2, 2), q, w, temperature=0.1, energy=0.0)  # no default eta
    with pytest.raises(ValueError):
        one_d.dynamic_orbital_susceptibility((8,), [[1]], w, eta=0.1, temperature=0.1, energy=0.0)
    # the wording the siblings share is the same text
    for other in (lambda: model.dynamic_susceptibility((2, 2, 2), q, w, eta=-1.0, temperature=0.1, energy=0.0),
                  lambda: call((2, 2, 2), q, w, eta=-1.0, temperature=0.1, energy=0.0)):
        with pytest.raises(ValueError, match="eta must be finite and positive, got -1.0"):
            other()
    for other in (lambda: model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=[1, 1]),
                  lambda: call((2, 2, 2), q, w, eta=0.1, temperature=0.1, energy=0.0, orbitals=[1, 1])):
        with pytest.raises(ValueError, match=r"orbitals must be distinct, got \[1, 1\]"):
            other()
    with pytest.raises(ValueError, match=r"q must be an integer array of shape \(NQ, 3\), got None"):
        call((2, 2, 2), None, w, eta=0.1, temperature=0.1, energy=0.0)
    assert not hasattr(tbmodels_amd.KdotpModel, "dynamic_orbital_susceptibility")
    assert tbmodels_amd.DynamicOrbitalSusceptibility._fields == ("mu", "q", "omega", "orbitals", "chi")
    assert "DynamicOrbitalSusceptibility" in tbmodels_amd.__all__


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in NEW_SYMBOLS:
        found = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert found, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        declared = [" ".join(part.split()) for part in found.group(1).split(",")]
        assert len(declared) == len(argtypes), (name, declared)
        for text, ctype in zip(declared, argtypes):
            if "*" in text:
                assert ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer), (name, text)
            else:
                assert ctype is kinds[text.rsplit(" ", 1)[0]], (name, text)
