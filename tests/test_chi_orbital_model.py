"""
tools/chi_model.py `orbital_susceptibility`, the NumPy statement of the orbital-resolved bare static susceptibility chi_0[i, j](q)
(DESIGN.md section 17), against the nine properties that define the quantity, the formula as written, and the argument checks of
`Model.orbital_susceptibility`, which need no device.

Inputs: random ascending bands with a flat band and an exact degenerate pair in every k-point, random unitary U, on the meshes
2 x 3 x 2, 3 x 4, 1 x 5 and 1 x 1 x 1 with 1, 3 and 9 orbitals, mu inside the bands, T in {0.05, 0.5}, both conventions with random
positions.  Bound: chi_model.orbital_tolerance per component of an element for every comparison of two evaluations;
the NumPy model hands the n^4 part to BLAS, so among the identities of bits only those that repeat the same products (properties 5,
6, 8, exact Hermiticity) are asserted as such on it, and property 9 within the bound -- the kernels' test asserts it bit for bit.
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
MU = 0.1
_CACHE = {}


def _eigensystem(mesh, n):
    """As `_eigensystem` of tests/test_gpu_chi.py: band 0 flat, bands 1 and 2 an exact degenerate pair, random unitary U; and random
    positions.  Computed once, never written."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(6100 + 41 * n_k + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
        eig[:, 0] = -1.25 if n > 1 else 0.125
        if n >= 3:
            eig[:, 2] = eig[:, 1]
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        pos = rng.uniform(0.0, 1.0, size=(n, len(mesh)))
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        for array in (eig, U, pos):
            array.setflags(write=False)
        _CACHE[key] = (eig, U, pos)
    return _CACHE[key]


def _vectors(mesh):
    """0, +-e_d, a vector with every component non-zero, its negative, the first shifted by whole mesh periods, a duplicate of +e_0."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], -full[None, :], (full + shift)[None, :], unit[:1]])
    names = {"plus": list(range(1, 1 + dim)) + [1 + 2 * dim], "minus": list(range(1 + dim, 1 + 2 * dim)) + [2 + 2 * dim],
             "full": 1 + 2 * dim, "shifted": 3 + 2 * dim, "duplicate": (1, 4 + 2 * dim)}
    return np.ascontiguousarray(q), names


def _chi(mesh, n, T, convention, q=None, mu=MU, U=None, orbitals=None):
    eig, vec, pos = _eigensystem(mesh, n)
    q = _vectors(mesh)[0] if q is None else q
    phases = chi_model.phase_table(mesh, q, pos) if convention == 1 else None
    return chi_model.orbital_susceptibility(eig, vec if U is None else U, mesh, q, mu, T, phases, orbitals)


def _parts(z):
    z = np.asarray(z)
    return max(np.abs(z.real).max(), np.abs(z.imag).max())


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_hermitian_psd_sum_rule_inversion_and_high_temperature(mesh, n):
    eig, vec, pos = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    worst = [0.0, 0.0, 0.0, np.inf]
    for T in TEMPERATURES:
        tol, tol_scalar = chi_model.orbital_tolerance(n_k, n, T), chi_model.tolerance(n_k, n, T)
        for convention in (1, 2):
            chi = _chi(mesh, n, T, convention)
            assert chi.shape == (len(q), n, n) and chi.dtype == np.complex128 and np.all(np.isfinite(_bits(chi)))
            # property 1, and the form of the output: exactly Hermitian, the diagonal's imaginary part +0
            assert np.array_equal(chi, np.conj(np.transpose(chi, (0, 2, 1))))
            diagonal = np.ascontiguousarray(np.diagonal(chi, axis1=1, axis2=2).imag)
            assert np.all(diagonal == 0.0) and not np.any(np.signbit(diagonal))
            lowest = np.linalg.eigvalsh(chi).min()
            worst[3] = min(worst[3], lowest)
            assert lowest >= -tol * n, (mesh, n, T, convention, lowest)
            # property 2: the sum over (i, j) is the scalar chi_0(q)
            phases = chi_model.phase_table(mesh, q, pos) if convention == 1 else None
            scalar = chi_model.susceptibility(eig, vec, mesh, q, MU, T, True, phases)
            total = chi.sum(axis=(1, 2))
            worst[0] = max(worst[0], np.abs(total.real - scalar).max() / (n * n * tol + tol_scalar))
            assert np.all(np.abs(total.real - scalar) <= n * n * tol + tol_scalar) and np.all(np.abs(total.imag) <= n * n * tol)
            # property 3: chi(-q) = chi(q)^T; q = 0 is its own partner
            for a, b in zip(at["plus"] + [0], at["minus"] + [0]):
                gap = _parts(chi[b] - chi[a].T)
                worst[1] = max(worst[1], gap / tol)
                assert gap <= tol, (mesh, n, T, convention, a, b, gap)
    hot = 1e9 * max(float(np.ptp(eig)), 1.0)
    for convention in (1, 2):  # property 4
        chi = _chi(mesh, n, hot, convention)
        gap = _parts(4.0 * hot * chi - np.eye(n)[None])
        worst[2] = max(worst[2], gap)
        assert gap <= 4.0 * hot * chi_model.orbital_tolerance(n_k, n, hot) + 1e-8  # (h(y) - 1 and 4 f (1 - f) - 1 are of the order 1 / hot)
    print("mesh %s n = %d: sum rule %.2e and inversion %.2e of the bound, |4 T chi - 1| %.2e, lowest eigenvalue %.3e" % (mesh, n, worst[0], worst[1], worst[2], worst[3]))


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_far_outside_the_spectrum_every_bit_is_zero(mesh, n):
    eig, _, _ = _eigensystem(mesh, n)
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):
            for convention in (1, 2):
                flat = _bits(_chi(mesh, n, T, convention, mu=mu))
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
        for convention in (1, 2):
            gap = _parts(_chi(mesh, n, T, convention) - _chi(mesh, n, T, convention, U=turned))  # property 7
            # the turned eigenvectors are another input, each of its entries off by a few u: twice the bound covers both evaluations
            assert gap <= 2.0 * chi_model.orbital_tolerance(n_k, n, T) + 16 * n * 2.0 ** -53 / T, (mesh, n, T, convention, gap)


# selections for property 9 that fit n: a single orbital, a shuffled subset with the last orbital, a pair, all of them reversed
SELECTIONS = {1: ([0],), 3: ([1], [2, 0], [2, 1, 0]), 9: ([4], [8, 0, 3], [2, 1], list(range(8, -1, -1)))}


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_bits_do_not_depend_on_the_list_and_selections_agree(mesh, n):
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    for T in TEMPERATURES:
        tol = chi_model.orbital_tolerance(n_k, n, T)
        for convention in (1, 2):
            chi = _chi(mesh, n, T, convention)
            assert np.array_equal(_bits(chi[at["duplicate"][0]]), _bits(chi[at["duplicate"][1]]))  # property 8
            assert np.array_equal(_bits(chi), _bits(_chi(mesh, n, T, convention)))
            order = np.random.default_rng(3).permutation(len(q))
            assert np.array_equal(_bits(chi[order]), _bits(_chi(mesh, n, T, convention, q=np.ascontiguousarray(q[order]))))
            for index in (0, len(q) - 3):
                assert np.array_equal(_bits(_chi(mesh, n, T, convention, q=q[index:index + 1])[0]), _bits(chi[index]))
            if convention == 2:
                assert np.array_equal(_bits(chi[at["full"]]), _bits(chi[at["shifted"]]))  # property 6
            for chosen in SELECTIONS[n]:  # property 9 (the model: within the bound)
                part = _chi(mesh, n, T, convention, orbitals=chosen)
                assert part.shape == (len(q), len(chosen), len(chosen))
                assert _parts(part - chi[:, chosen][:, :, chosen]) <= tol, (mesh, n, T, convention, chosen)
    for bad in ([], [0, 0], [n], [-1], [0.0], [[0, 0]], [[0]]):
        with pytest.raises(ValueError):
            _chi(mesh, n, TEMPERATURES[0], 2, orbitals=bad)
    for function in (chi_model.orbital_susceptibility, chi_model.orbital_susceptibility_naive):  # the two validate alike
        eig, vec, _ = _eigensystem(mesh, n)
        with pytest.raises(ValueError):
            function(eig, vec, mesh, q.astype(float), MU, TEMPERATURES[0])
        with pytest.raises(ValueError):
            function(eig, vec, mesh, q, MU, TEMPERATURES[0], None, [n])


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_model_against_the_formula_as_written(mesh, n):
    """F as the quotient (f(a) - f(b)) / (a - b), f' on the diagonal.  Condition: |E - mu| / T < 709, so that no exponential of the
    plain Fermi function overflows.  The difference as written is off by under 17 u in absolute terms however small it is (each f by
    (2 ULP_EXP + 3) u relative and 2 u / e from the exponential's argument, then one subtraction; tests/test_chi_dynamic_model.py
    has the same count), and the division by a - b makes that 17 u / gap per unit of sum |A_i| |A_j| <= 1, gap the smallest non-zero
    level difference of the case; exact ties take the f' branch, which is as accurate as the stable form.  So the allowance is the
    bound plus 17 u / gap."""
    eig, vec, pos = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, _ = _vectors(mesh)
    worst = 0.0
    assert np.abs(eig - MU).max() / min(TEMPERATURES) < 709.0
    for T in TEMPERATURES:
        for convention in (1, 2):
            phases = chi_model.phase_table(mesh, q, pos) if convention == 1 else None
            want = chi_model.orbital_susceptibility_naive(eig, vec, mesh, q, MU, T, phases)
            got = _chi(mesh, n, T, convention)
            diffs = np.abs(eig.reshape(-1)[:, None] - eig.reshape(-1)[None, :])
            gap = diffs[diffs > 0.0].min() if np.any(diffs > 0.0) else 1.0
            allowance = chi_model.orbital_tolerance(n_k, n, T) + 17.0 * 2.0 ** -53 / gap
            worst = max(worst, _parts(got - want) / allowance)
            assert _parts(got - want) <= allowance, (mesh, n, T, convention, _parts(got - want), allowance)
    print("mesh %s n = %d: max |model - formula as written| / allowance = %.3e" % (mesh, n, worst))


def test_the_tolerance_is_the_documented_formula():
    u = 2.0 ** -53
    n_k, n, T = 12, 9, 0.05
    c_e = c_m = 2
    c_a = 14  # two amplitudes of two complex products (three roundings per component each), the scale by t, the product
    assert chi_model.ROUNDINGS_AMPLITUDES == c_a and chi_model.ULP_EXP == c_e and chi_model.ULP_EXPM1 == c_m
    want = 2 * ((n_k * n * n + 4 * c_e + c_m + 15 + c_a) / 4 + 4) * u / T
    assert np.isclose(chi_model.orbital_tolerance(n_k, n, T), want, rtol=1e-14)
    assert np.isclose(want, (n_k * n * n / 2 + 27.5) * u / T, rtol=1e-14)


# ---- the public interface -----------------------------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    q = [[1, 0, 0]]
    for kwargs in ({}, {"energy": 0.0, "n_electrons": 4}, {"energy": np.nan}, {"energy": "0"}, {"n_electrons": 0}, {"n_electrons": 8},
                   {"n_electrons": np.nan}, {"n_electrons": "4"}):
        with pytest.raises(ValueError):
            model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, **kwargs)
    for bad in (None, np.zeros((2, 3)), [[0.5, 0, 0]], np.zeros((2, 2), dtype=int), [0, 1], np.zeros((0, 3), dtype=int), "000", [[0, 0, 2 ** 70]],
                np.zeros((1, 3), dtype=bool)):
        with pytest.raises(ValueError):
            model.orbital_susceptibility((2, 2, 2), bad, temperature=0.1, energy=0.0)
    for bad in ([], [0, 0], [8], [-1], [0.0, 1.0], [[0, 1]], "01", [True, False], [None], np.zeros((0,), dtype=int), [2 ** 70], {"orbitals": 1},
                np.array([1], dtype=np.uint64)):
        with pytest.raises(ValueError):
            model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=bad)
    for temperature in (0.0, -0.1, np.nan, np.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            model.orbital_susceptibility((2, 2, 2), q, temperature=temperature, energy=0.0)
    for mesh in ((4, 4), (4, 0, 4), (4.0, 4.0, 4.0), 4):
        with pytest.raises(ValueError):
            model.orbital_susceptibility(mesh, q, temperature=0.1, n_electrons=4)
    for kwargs in ({"convention": 0}, {"convention": 3}, {"convention": "2"}):
        with pytest.raises(ValueError):
            model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, **kwargs)
    with pytest.raises(TypeError):
        model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, matrix_elements=False)  # there is no such form
    with pytest.raises(TypeError):
        model.orbital_susceptibility((2, 2, 2), q, 0.1, energy=0.0)  # keyword only
    with pytest.raises(TypeError):
        model.orbital_susceptibility((2, 2, 2), q, energy=0.0)  # no default temperature
    with pytest.raises(ValueError):
        one_d.orbital_susceptibility((8,), [[1]], temperature=0.1, energy=0.0)
    # the wording the three methods share is the same text
    for call in (lambda: model.susceptibility((2, 2, 2), q, temperature=-1.0, energy=0.0),
                 lambda: model.orbital_susceptibility((2, 2, 2), q, temperature=-1.0, energy=0.0)):
        with pytest.raises(ValueError, match="temperature must be finite and positive, got -1.0"):
            call()
    for call in (lambda: model.susceptibility((2, 2, 2), None, temperature=0.1, energy=0.0),
                 lambda: model.orbital_susceptibility((2, 2, 2), None, temperature=0.1, energy=0.0)):
        with pytest.raises(ValueError, match=r"q must be an integer array of shape \(NQ, 3\), got None"):
            call()
    with pytest.raises(ValueError, match=r"orbitals must be distinct, got \[1, 1\]"):
        model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=[1, 1])
    assert not hasattr(tbmodels_amd.KdotpModel, "orbital_susceptibility")
    assert tbmodels_amd.OrbitalSusceptibility._fields == ("mu", "q", "orbitals", "chi") and "OrbitalSusceptibility" in tbmodels_amd.__all__


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in ("tbk_chi_orbital_from_eigensystem", "tbk_orbital_susceptibility", "tbk_orbital_susceptibility_multi", "tbk_chi_orbital_plan"):
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
