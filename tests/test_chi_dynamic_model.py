"""
tools/chi_model.py `dynamic_susceptibility`, the NumPy statement of the bare dynamic susceptibility chi_0(q, omega + i eta)
(DESIGN.md section 16), against the seven properties that define the quantity, the stable occupation difference against
f(a) - f(b) in extended precision, the formula as written in complex arithmetic, and the argument checks of
`Model.dynamic_susceptibility`, which need no device.

Inputs: random Hermitian models (hoppings to 0 and two further cells) on the meshes 2 x 3 x 2, 3 x 4, 1 x 5 and 1 x 1 x 1 with 1, 3 and
9 orbitals, eigensystems of numpy.linalg.eigh, mu inside the spectrum, T in {0.05, 0.5}, eta in {0.05, 1e-3}, both conventions with
random positions; frequencies 0, +-0.2, +-0.7, one exact level difference, 1e6 and a duplicate.  Bound: chi_model.dynamic_tolerance
 per frequency for every comparison of two evaluations, in either component; identities of bits are asserted as such.
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
import dos_model  # noqa: E402  pylint: disable=wrong-import-position

MESHES = [(2, 3, 2), (3, 4), (1, 5), (1, 1, 1)]
ORBITALS = [1, 3, 9]
TEMPERATURES = [0.05, 0.5]
ETAS = [0.05, 1e-3]
_CACHE = {}


def _system(mesh, n):
    """Eigenvalues (NK, n), eigenvectors (NK, n, n) of convention 2 of ONE Hermitian family and positions (n, dim): computed once,
    never written."""
    key = (mesh, n)
    if key not in _CACHE:
        dim = len(mesh)
        rng = np.random.default_rng(1700 + 13 * int(np.prod(mesh)) + n)
        R = np.zeros((3, dim), dtype=np.int64)
        R[1, 0], R[2, -1], R[2, 0] = 1, 1, -1
        hop = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
        kpts = dos_model.mesh_kpoints(mesh)
        ham = np.einsum("kr,rij->kij", np.exp(2j * np.pi * (kpts @ R.T)), hop)
        ham = ham + np.conj(np.transpose(ham, (0, 2, 1)))
        eig, vec = np.linalg.eigh(ham)
        pos = rng.uniform(0.0, 1.0, size=(n, dim))
        for array in (eig, vec, pos):
            array.setflags(write=False)
        _CACHE[key] = (eig, vec, pos)
    return _CACHE[key]


def _mu(eig):
    return float(np.quantile(eig, 0.4)) + 1e-3


def _vectors(mesh):
    """0, +-e_d, a vector with every component non-zero, its negative, the first shifted by whole mesh periods, a duplicate of +e_0."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], -full[None, :], (full + shift)[None, :], unit[:1]])
    names = {"zero": 0, "plus": list(range(1, 1 + dim)) + [1 + 2 * dim], "minus": list(range(1 + dim, 1 + 2 * dim)) + [2 + 2 * dim],
             "full": 1 + 2 * dim, "shifted": 3 + 2 * dim, "duplicate": (1, 4 + 2 * dim)}
    return np.ascontiguousarray(q), names


def _frequencies(mesh, n):
    """0, +-0.2, +-0.7, one exact level difference of the pair (k = 0, k + e_0) and its negative, +-1e6, a duplicate of 0.2: closed
    under omega -> -omega, `_mirror` is the permutation."""
    eig = _system(mesh, n)[0]
    level = float(eig[chi_model.shifted_points(mesh, _vectors(mesh)[0][1])[0], n - 1] - eig[0, 0])
    omega = np.array([0.0, 0.2, -0.2, 0.7, -0.7, level, -level, 1e6, -1e6, 0.2])
    mirror = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 2])
    return omega, mirror


def _spread(eig, omega):
    return 2.0 * float(np.ptp(eig)) + np.abs(omega)


def _chi(mesh, n, T, eta, convention, matrix_elements=True, q=None, mu=None, omega=None):
    eig, vec, pos = _system(mesh, n)
    q = _vectors(mesh)[0] if q is None else q
    omega = _frequencies(mesh, n)[0] if omega is None else omega
    phases = chi_model.phase_table(mesh, q, pos) if convention == 1 and matrix_elements else None
    return chi_model.dynamic_susceptibility(eig, vec, mesh, q, _mu(eig) if mu is None else mu, T, omega, eta, matrix_elements, phases)


def _parts(z):
    """max over both components of |z|."""
    z = np.asarray(z)
    return max(np.abs(z.real).max(), np.abs(z.imag).max())


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_conjugation_static_ceiling_and_absorptive_sign(mesh, n):
    eig, vec, pos = _system(mesh, n)
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    omega, mirror = _frequencies(mesh, n)
    worst = [0.0, -np.inf, np.inf]
    for T in TEMPERATURES:
        for eta in ETAS:
            for me in (True, False):
                tol = chi_model.dynamic_tolerance(n_k, n, T, eta, _spread(eig, omega), me)[None, :]
                tol_static = chi_model.tolerance(n_k, n, T, me)
                for convention in ((1, 2) if me else (2,)):
                    chi = _chi(mesh, n, T, eta, convention, me)
                    assert chi.shape == (len(q), len(omega)) and chi.dtype == np.complex128 and np.all(np.isfinite(chi.view(float)))
                    # property 1: chi(-q, -omega + i eta) = conj chi(q, omega + i eta); q = 0 is its own partner
                    for a, b in zip(at["plus"] + [at["zero"]], at["minus"] + [at["zero"]]):
                        gap = chi[b][mirror] - np.conj(chi[a])
                        worst[0] = max(worst[0], (np.maximum(np.abs(gap.real), np.abs(gap.imag)) / tol[0]).max())
                        assert np.all(np.abs(gap.real) <= tol[0]) and np.all(np.abs(gap.imag) <= tol[0]), (mesh, n, T, eta, me, convention)
                    # property 2: 0 <= Re chi(q, i eta) <= chi_static(q), with both evaluations' bounds as slack
                    phases = chi_model.phase_table(mesh, q, pos) if convention == 1 and me else None
                    static = chi_model.susceptibility(eig, vec, mesh, q, _mu(eig), T, me, phases)
                    at_zero = chi[:, 0].real
                    worst[1] = max(worst[1], (at_zero - static).max())
                    assert np.all(at_zero >= -tol[0, 0]) and np.all(at_zero <= static + tol[0, 0] + tol_static), (mesh, n, T, eta, me, convention)
                    # property 3: omega [Im chi(q, omega) + Im chi(-q, omega)] >= 0
                    for a, b in zip(at["plus"], at["minus"]):
                        absorptive = omega * (chi[a].imag + chi[b].imag)
                        worst[2] = min(worst[2], absorptive.min())
                        assert np.all(absorptive >= -2.0 * np.abs(omega) * tol[0]), (mesh, n, T, eta, me, convention)
    print("mesh %s n = %d: conjugation %.2e of the bound, Re chi(i eta) - static at most %.2e, omega (Im chi(q) + Im chi(-q)) at least %.2e"
          % (mesh, n, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_no_response_at_q_zero_with_the_eigenvectors_of_one_family(mesh, n):
    eig, _, _ = _system(mesh, n)
    n_k = int(np.prod(mesh))
    omega, _ = _frequencies(mesh, n)
    zero = np.zeros((1, len(mesh)), dtype=np.int64)
    for T in TEMPERATURES:
        for eta in ETAS:
            # property 4: M(k, 0) = U(k)^H U(k) is the identity, and g = 0 on its diagonal.  (The eigenvectors of LAPACK are orthonormal to
            # a few n u: the off-diagonal |M|^2 is of the order of (n u)^2, far inside the bound's |M|^2 term.)
            chi = _chi(mesh, n, T, eta, 2, True, q=zero)
            tol = chi_model.dynamic_tolerance(n_k, n, T, eta, _spread(eig, omega))
            assert np.all(np.abs(chi.real) <= tol) and np.all(np.abs(chi.imag) <= tol), (mesh, n, T, eta, _parts(chi))


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_far_below_and_above_the_spectrum_every_bit_is_zero(mesh, n):
    eig, _, _ = _system(mesh, n)
    for T in TEMPERATURES:
        for eta in ETAS:
            for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):
                for me in (True, False):
                    flat = _chi(mesh, n, T, eta, 2, me, mu=mu).view(float)
                    assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (mesh, n, T, eta, mu, me)  # property 5


@pytest.mark.parametrize("mesh", MESHES)
def test_bits_do_not_depend_on_the_lists(mesh):
    n, T, eta = 3, 0.05, 1e-3
    q, at = _vectors(mesh)
    omega, _ = _frequencies(mesh, n)
    for convention in (1, 2):
        chi = _chi(mesh, n, T, eta, convention).view(float).reshape(len(q), len(omega), 2)
        assert np.array_equal(chi[at["duplicate"][0]], chi[at["duplicate"][1]]) and np.array_equal(chi[:, 1], chi[:, 9])  # property 7
        assert np.array_equal(chi, _chi(mesh, n, T, eta, convention).view(float).reshape(chi.shape))
        q_order, w_order = np.random.default_rng(3).permutation(len(q)), np.random.default_rng(4).permutation(len(omega))
        moved = _chi(mesh, n, T, eta, convention, q=np.ascontiguousarray(q[q_order]), omega=omega[w_order]).view(float).reshape(chi.shape)
        assert np.array_equal(chi[q_order][:, w_order], moved)
        for index in (0, len(q) - 3):
            for j in (0, 5, len(omega) - 1):
                alone = _chi(mesh, n, T, eta, convention, q=q[index:index + 1], omega=omega[j:j + 1]).view(float).reshape(2)
                assert np.array_equal(alone, chi[index, j])
        one_number = _chi(mesh, n, T, eta, convention, omega=0.2).view(float).reshape(len(q), 1, 2)
        assert np.array_equal(one_number[:, 0], chi[:, 1])
        if convention == 2:
            assert np.array_equal(chi[at["full"]], chi[at["shifted"]])  # property 6
    for d, n_d in enumerate(mesh):  # property 6 at the ends of the integers
        moved = q.copy()
        moved[:, d] += (2 ** 62 // n_d) * n_d
        assert np.array_equal(_chi(mesh, n, T, eta, 2).view(float), _chi(mesh, n, T, eta, 2, q=moved).view(float))
    for bad in (dict(q=q.astype(float)), dict(omega=[0.1, np.nan]), dict(omega=[]), dict(omega=[[0.1]]), dict(omega=[np.inf])):
        with pytest.raises(ValueError):
            _chi(mesh, n, T, eta, 2, **bad)
    for eta_bad in (0.0, -0.05, np.nan, np.inf, 1e-200):
        with pytest.raises(ValueError):
            _chi(mesh, n, T, eta_bad, 2)


# ---- the occupation difference ------------------------------------------------------------------------------------------------------
def test_stable_difference_against_extended_precision():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble must carry a 64-bit significand for this reference"
    rng = np.random.default_rng(31)
    u = 2.0 ** -53
    for mu, T in ((0.1, 0.05), (0.1, 0.5), (-0.7, 1.0)):
        a, b = rng.normal(size=20000), rng.normal(size=20000)
        a[:200] = b[:200]  # equal energies: an exact zero
        b[200:400] = np.nextafter(a[200:400], np.inf)  # 1 ulp apart: f(a) - f(b) as written would be 0 or one ulp of f
        stable = chi_model.occupation_difference(a, b, mu, T)
        wide = lambda x: 1 / (1 + np.exp((x.astype(np.longdouble) - np.longdouble(mu)) / np.longdouble(T)))  # noqa: E731
        exact = wide(a) - wide(b)  # (the cancellation costs the 64-bit significand |a - b| / T of its 11 spare bits: see the last term)
        y = -np.abs(a - b) / T
        # relative: the two tables (2 ULP_EXP + 3) u each, expm1 and its argument (ULP_EXPM1 + 3) u, two products: 19 u, asserted at 32;
        # absolute: 2 u per table entry from the exponential's argument, times the third factor |expm1(y)| <= 1;  the reference's own
        # cancellation: 4 roundings of 2^-64 on values <= 1
        bound = 32 * u * np.abs(np.asarray(exact, dtype=float)) + 4 * u * np.abs(np.expm1(y)) + 2.0 ** -61
        err = np.abs(np.asarray(stable.astype(np.longdouble) - exact, dtype=float))
        print("mu = %g, T = %g: max |g - (f(a) - f(b))| / bound = %.3f over %d pairs" % (mu, T, (err / bound).max(), len(a)))
        assert np.all(err <= bound)
        assert np.all(stable[:200] == 0.0) and np.all(stable[200:400] >= 0.0)  # a <= b: f(a) >= f(b)
        assert np.array_equal(stable, -chi_model.occupation_difference(b, a, mu, T))  # antisymmetric, bit for bit
        assert np.all(np.abs(stable) <= 1.0)
    assert chi_model.occupation_difference(-1e300, 1e300, 0.0, 1e-6) == 1.0 and chi_model.occupation_difference(1e300, -1e300, 0.0, 1e-6) == -1.0


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_model_against_the_formula_as_written(mesh, n):
    """The formula in complex arithmetic with f(a) - f(b) as the difference of two Fermi functions.  Condition: |E - mu| / T < 709
    for every state, so that no exponential of the plain Fermi function overflows (here at most 20 / 0.05), and the comparison is of
    ABSOLUTE errors: f(a) - f(b) as written is off by a few u however small it is (each f by (2 ULP_EXP + 3) u relative and 2 u / e
    from the exponential's argument, then one subtraction: under 17 u), the complex quotient and the product with |M|^2 by another
    8 u of the term -- under the (4 ULP_EXP + ULP_EXPM1 + ULP_DIV + 18 + 4) u = 34 u that dynamic_tolerance charges per unit of |M|^2
    / eta, because its relative terms are taken at |g| = 1.  So the bound holds for this evaluation at every pair; what the
    difference as written loses is the RELATIVE accuracy of small g, which test_stable_difference_against_extended_precision covers."""
    eig, vec, pos = _system(mesh, n)
    n_k = int(np.prod(mesh))
    q, _ = _vectors(mesh)
    omega, _ = _frequencies(mesh, n)
    assert np.abs(eig - _mu(eig)).max() / min(TEMPERATURES) < 709.0
    worst = 0.0
    for T in TEMPERATURES:
        for eta in ETAS:
            for me in (True, False):
                for convention in ((1, 2) if me else (2,)):
                    phases = chi_model.phase_table(mesh, q, pos) if convention == 1 and me else None
                    got = _chi(mesh, n, T, eta, convention, me)
                    want = chi_model.dynamic_susceptibility_naive(eig, vec, mesh, q, _mu(eig), T, omega, eta, me, phases)
                    tol = chi_model.dynamic_tolerance(n_k, n, T, eta, _spread(eig, omega), me)[None, :]
                    gap = got - want
                    worst = max(worst, (np.maximum(np.abs(gap.real), np.abs(gap.imag)) / tol).max())
                    assert np.all(np.abs(gap.real) <= tol) and np.all(np.abs(gap.imag) <= tol), (mesh, n, T, eta, me, convention)
    print("mesh %s n = %d: max |model - formula as written| / bound = %.3e" % (mesh, n, worst))


def test_a_frequency_on_a_transition_is_finite():
    mesh, n, T = (2, 3, 2), 3, 0.05
    eig, vec, _ = _system(mesh, n)
    q, _ = _vectors(mesh)
    omega, _ = _frequencies(mesh, n)
    to = chi_model.shifted_points(mesh, q[1])
    assert (eig[0, 0] - eig[to[0], n - 1]) + omega[5] == 0.0  # x = 0 exactly for the pair (k = 0, b = 0) -> (k + e_0, b' = n - 1)
    for eta in ETAS:
        chi = _chi(mesh, n, T, eta, 2, q=q[1:2], omega=omega[5:6])
        want = chi_model.dynamic_susceptibility_naive(eig, vec, mesh, q[1:2], _mu(eig), T, omega[5:6], eta)
        tol = chi_model.dynamic_tolerance(12, n, T, eta, _spread(eig, omega[5:6]))
        print("eta = %g: chi at an exact transition = %r, |model - formula| = %.3e (bound %.3e)" % (eta, chi[0, 0], abs(chi[0, 0] - want[0, 0]), tol[0]))
        assert np.all(np.isfinite(chi.view(float))) and _parts(chi - want) <= tol[0]


def test_the_tolerance_is_the_documented_formula():
    u = 2.0 ** -53
    n_k, n, eta, spread = 12, 9, 1e-3, 5.0
    with_me = 2 * ((n_k * n * n + 34 + spread / eta) * n + 2 * (3 * n + 5) * n ** 1.5 + 3 * n) * u / eta
    without = 2 * ((n_k * n * n + 34 + spread / eta) * n * n) * u / eta
    assert np.isclose(chi_model.dynamic_tolerance(n_k, n, 0.05, eta, spread), with_me, rtol=1e-14)
    assert np.isclose(chi_model.dynamic_tolerance(n_k, n, 0.5, eta, spread, False), without, rtol=1e-14)
    per_frequency = chi_model.dynamic_tolerance(n_k, n, 0.05, eta, np.array([1.0, 5.0]))
    assert per_frequency.shape == (2,) and per_frequency[1] == chi_model.dynamic_tolerance(n_k, n, 0.05, eta, 5.0) > per_frequency[0]


# ---- the public interface -----------------------------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    q, omega = [[1, 0, 0]], [0.0, 0.5]
    for kwargs in ({}, {"energy": 0.0, "n_electrons": 4}, {"energy": np.nan}, {"energy": "0"}, {"n_electrons": 0}, {"n_electrons": 8},
                   {"n_electrons": np.nan}, {"n_electrons": "4"}):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility((2, 2, 2), q, omega, eta=0.05, temperature=0.1, **kwargs)
    for bad in (None, np.zeros((2, 3)), [[0.0, 1.0, 0.0]], [[0.5, 0, 0]], np.zeros((2, 2), dtype=int), [0, 1], [[0, 1, 0, 0]],
                np.zeros((0, 3), dtype=int), np.zeros((2, 2, 3), dtype=int), "000", [[0, 0, 2 ** 70]], np.zeros((1, 3), dtype=bool)):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility((2, 2, 2), bad, omega, eta=0.05, temperature=0.1, energy=0.0)
    for bad in (None, "0.1", [], [[0.1, 0.2]], np.zeros((0,)), [0.1, np.nan], [np.inf], [-np.inf, 0.0], [0.1 + 0.2j], [True, False], ["0.1"],
                np.zeros((2, 2, 2)), [None], {"omega": 1.0}):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility((2, 2, 2), q, bad, eta=0.05, temperature=0.1, energy=0.0)
    for eta in (0.0, -0.1, np.nan, np.inf, "0.1", None, True, 1e-200, [0.05]):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility((2, 2, 2), q, omega, eta=eta, temperature=0.1, energy=0.0)
    for temperature in (0.0, -0.1, np.nan, np.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility((2, 2, 2), q, omega, eta=0.05, temperature=temperature, energy=0.0)
    for mesh in ((4, 4), (4, 0, 4), (4.0, 4.0, 4.0), 4):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility(mesh, q, omega, eta=0.05, temperature=0.1, n_electrons=4)
    for kwargs in ({"convention": 0}, {"convention": 3}, {"convention": "2"}, {"matrix_elements": 1}, {"matrix_elements": None}):
        with pytest.raises(ValueError):
            model.dynamic_susceptibility((2, 2, 2), q, omega, eta=0.05, temperature=0.1, energy=0.0, **kwargs)
    with pytest.raises(TypeError):
        model.dynamic_susceptibility((2, 2, 2), q, omega, 0.05, temperature=0.1, energy=0.0)  # keyword only
    with pytest.raises(TypeError):
        model.dynamic_susceptibility((2, 2, 2), q, omega, temperature=0.1, energy=0.0)  # no default broadening
    with pytest.raises(TypeError):
        model.dynamic_susceptibility((2, 2, 2), q, omega, eta=0.05, energy=0.0)  # no default temperature
    with pytest.raises(ValueError):
        one_d.dynamic_susceptibility((8,), [[1]], omega, eta=0.05, temperature=0.1, energy=0.0)
    # the wording the two methods share is the same text
    for call in (lambda: model.susceptibility((2, 2, 2), q, temperature=-1.0, energy=0.0),
                 lambda: model.dynamic_susceptibility((2, 2, 2), q, omega, eta=0.05, temperature=-1.0, energy=0.0)):
        with pytest.raises(ValueError, match="temperature must be finite and positive, got -1.0"):
            call()
    assert not hasattr(tbmodels_amd.KdotpModel, "dynamic_susceptibility")
    assert tbmodels_amd.DynamicSusceptibility._fields == ("mu", "q", "omega", "chi")


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in ("tbk_chi_dynamic_from_eigensystem", "tbk_dynamic_susceptibility", "tbk_dynamic_susceptibility_multi", "tbk_chi_dynamic_plan"):
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
