"""
tools/chi_model.py, the NumPy statement of the bare susceptibility chi_0(q), against the seven properties
that define the quantity, the stable pair factor F against the quotient it replaces, and the argument checks of
`Model.susceptibility`, which need no device.

Inputs: random Hermitian models (hoppings to 0 and two further cells) on the meshes 2 x 3 x 2, 3 x 4, 1 x 5, 1 x 1 x 1 and 4 x 4 x 4
with 1, 3 and 9 orbitals, eigensystems of numpy.linalg.eigh, mu inside the spectrum, T in {0.05, 0.5}, both conventions with random
positions.  Bound: chi_model.tolerance (tol_chi of DESIGN 15.4) for every comparison of two evaluations; identities of bits are
asserted as such.
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

MESHES = [(2, 3, 2), (3, 4), (1, 5), (1, 1, 1), (4, 4, 4)]
ORBITALS = [1, 3, 9]
TEMPERATURES = [0.05, 0.5]
_CACHE = {}


def _system(mesh, n):
    """Eigenvalues mesh + (n,), eigenvectors (NK, n, n) of convention 2 and positions (n, dim): computed once, never written."""
    key = (mesh, n)
    if key not in _CACHE:
        dim = len(mesh)
        rng = np.random.default_rng(700 + 13 * int(np.prod(mesh)) + n)
        R = np.zeros((3, dim), dtype=np.int64)
        R[1, 0], R[2, -1], R[2, 0] = 1, 1, -1
        hop = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
        kpts = dos_model.mesh_kpoints(mesh)
        ham = np.einsum("kr,rij->kij", np.exp(2j * np.pi * (kpts @ R.T)), hop)
        ham = ham + np.conj(np.transpose(ham, (0, 2, 1)))
        eig, vec = np.linalg.eigh(ham)
        eig = np.ascontiguousarray(eig.reshape(tuple(mesh) + (n,)))
        pos = rng.uniform(0.0, 1.0, size=(n, dim))
        for array in (eig, vec, pos):
            array.setflags(write=False)
        _CACHE[key] = (eig, vec, pos)
    return _CACHE[key]


def _mu(eig):
    return float(np.quantile(eig, 0.4)) + 1e-3


def _vectors(mesh):
    """0, +-e_d, a vector with every component non-zero, the same shifted by whole mesh periods, a duplicate of +e_0."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.concatenate([np.zeros((1, dim), dtype=np.int64), unit, -unit, full[None, :], (full + shift)[None, :], unit[:1]])
    names = {"zero": 0, "plus": list(range(1, 1 + dim)), "minus": list(range(1 + dim, 1 + 2 * dim)), "full": 1 + 2 * dim, "shifted": 2 + 2 * dim,
             "duplicate": (1, 3 + 2 * dim)}
    return np.ascontiguousarray(q), names


def _chi(mesh, n, T, convention, matrix_elements=True, q=None, mu=None):
    eig, vec, pos = _system(mesh, n)
    q = _vectors(mesh)[0] if q is None else q
    phases = chi_model.phase_table(mesh, q, pos) if convention == 1 and matrix_elements else None
    return chi_model.susceptibility(eig, vec, mesh, q, _mu(eig) if mu is None else mu, T, matrix_elements, phases)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_sign_inversion_and_the_static_limit(mesh, n):
    eig, _, _ = _system(mesh, n)
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    for T in TEMPERATURES:
        tol = chi_model.tolerance(n_k, n, T)
        for convention in (1, 2):
            chi = _chi(mesh, n, T, convention)
            assert np.all(np.isfinite(chi)) and np.all(chi >= 0.0)  # property 1
            assert np.abs(chi[at["plus"]] - chi[at["minus"]]).max() <= tol, (mesh, n, T, convention)
            assert abs(chi[at["zero"]] - chi_model.static_limit(eig, _mu(eig), T)) <= tol  # property 2
            if convention == 2:  # (convention 1 takes the unreduced q in D: a whole period is another gauge there)
                assert chi[at["full"]] == chi[at["shifted"]]  # property 6
        pair = _chi(mesh, n, T, 2, matrix_elements=False)
        assert np.all(pair >= 0.0)
        assert np.abs(pair[at["plus"]] - pair[at["minus"]]).max() <= chi_model.tolerance(n_k, n, T, False)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_without_matrix_elements_only_the_eigenvalues_enter(mesh, n):
    eig, vec, _ = _system(mesh, n)
    q, _ = _vectors(mesh)
    rng = np.random.default_rng(5)
    other = np.linalg.qr(rng.normal(size=vec.shape) + 1j * rng.normal(size=vec.shape))[0]
    for T in TEMPERATURES:
        base = chi_model.susceptibility(eig, None, mesh, q, _mu(eig), T, False)
        assert np.array_equal(base, chi_model.susceptibility(eig, vec, mesh, q, _mu(eig), T, False))  # property 3
        assert np.array_equal(base, chi_model.susceptibility(eig, other, mesh, q, _mu(eig), T, False))
        # by hand at one vector: every pair of states of k and k+q with weight 1
        to = chi_model.shifted_points(mesh, q[-3])
        flat = eig.reshape(-1, n)
        want = -chi_model.pair_factor(flat[:, :, None], flat[to][:, None, :], _mu(eig), T).sum() / flat.shape[0]
        assert abs(base[-3] - want) <= chi_model.tolerance(flat.shape[0], n, T, False)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_high_temperature_limit_is_the_number_of_orbitals(mesh, n):
    eig, _, _ = _system(mesh, n)
    width = float(np.ptp(eig))
    T = 1e9 * (width if width > 0.0 else 1.0)  # (one orbital on one point has no bandwidth)
    n_k = int(np.prod(mesh))
    for convention in (1, 2):
        chi = _chi(mesh, n, T, convention)  # property 4: the rows of |M|^2 add up to 1 for any q and either convention
        # F = -(1 / 4T) (1 - O((E - mu)^2 / T^2)): 1e-17 relative at this temperature
        assert np.abs(4.0 * T * chi - n).max() <= 4.0 * T * chi_model.tolerance(n_k, n, T) + 1e-17 * n, (mesh, n, convention)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_far_below_and_above_the_spectrum_every_bit_is_zero(mesh, n):
    eig, _, _ = _system(mesh, n)
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # exp(-746) rounds to 0 (the smallest double is exp(-744.44))
            for me in (True, False):
                chi = _chi(mesh, n, T, 2, matrix_elements=me, mu=mu)
                assert np.all(chi == 0.0) and not np.any(np.signbit(chi)), (mesh, n, T, mu, me)  # property 5


@pytest.mark.parametrize("mesh", MESHES)
def test_bits_do_not_depend_on_the_list(mesh):
    n, T = 3, 0.05
    q, at = _vectors(mesh)
    for convention in (1, 2):
        chi = _chi(mesh, n, T, convention)
        assert chi[at["duplicate"][0]] == chi[at["duplicate"][1]]  # property 7
        assert np.array_equal(chi, _chi(mesh, n, T, convention))
        order = np.random.default_rng(3).permutation(len(q))
        assert np.array_equal(chi[order], _chi(mesh, n, T, convention, q=np.ascontiguousarray(q[order])))
        for index in (0, len(q) - 2):
            assert chi[index] == _chi(mesh, n, T, convention, q=q[index:index + 1])[0]
    for d, n_d in enumerate(mesh):  # property 6 at the ends of the integers
        moved = q.copy()
        moved[:, d] += (2 ** 62 // n_d) * n_d
        assert np.array_equal(_chi(mesh, n, T, 2), _chi(mesh, n, T, 2, q=moved))
    with pytest.raises(ValueError):
        _chi(mesh, n, T, 2, q=q.astype(float))


# ---- the pair factor --------------------------------------------------------------------------------------------------------------
def test_stable_factor_against_the_quotient_where_that_is_well_conditioned():
    rng = np.random.default_rng(11)
    u = 2.0 ** -53
    for mu, T in ((0.1, 0.05), (0.1, 0.5), (-0.7, 1.0)):
        a, b = rng.normal(size=20000), rng.normal(size=20000)
        keep = np.abs(a - b) >= 1e-2
        a, b = a[keep], b[keep]
        stable, naive = chi_model.pair_factor(a, b, mu, T), chi_model.pair_factor_naive(a, b, mu, T)
        assert np.all(stable <= 0.0) and np.all(stable >= -0.25 / T * (1 + 8 * u))
        assert np.array_equal(stable, chi_model.pair_factor(b, a, mu, T))  # symmetric, bit for bit
        # the quotient: each f is off by at most (x e^-x + 2) u <= 2.4 u (the error of exp's argument), the difference by 6 u
        bound = 8 * u / np.abs(a - b) + 32 * u * np.abs(stable)
        assert np.all(np.abs(stable - naive) <= bound), np.abs(stable - naive).max()


def test_stable_factor_on_and_next_to_the_diagonal():
    rng = np.random.default_rng(12)
    u = 2.0 ** -53
    for mu, T in ((0.1, 0.05), (0.1, 0.5)):
        a = np.concatenate([rng.normal(size=2000), [mu, mu + 700 * T, mu - 700 * T, mu + 650 * T]])
        x = (a.astype(np.longdouble) - np.longdouble(mu)) / np.longdouble(T)
        e = np.exp(-np.abs(x))
        derivative = np.asarray(-(e / ((1 + e) * (1 + e))) / np.longdouble(T), dtype=float)  # f' = -f (1 - f) / T, in extended precision
        on = chi_model.pair_factor(a, a, mu, T)
        # exp's argument carries 2 u |x| relative error: |x| e^-|x| <= 1 / e of it survives in f (1 - f) against 1 / 4 at most
        bound = 32 * u * np.abs(derivative) + 4 * u / T * np.exp(-np.abs(np.asarray(x, dtype=float))) * np.abs(np.asarray(x, dtype=float))
        assert np.all(np.abs(on - derivative) <= bound), np.abs(on - derivative).max()
        for other in (np.nextafter(a, np.inf), np.nextafter(a, -np.inf)):  # |a - b| = 1 ulp: the quotient would be 0 / ulp or ulp / ulp
            off = chi_model.pair_factor(a, other, mu, T)
            assert np.all(np.abs(off - derivative) <= 2 * bound + 64 * u * np.abs(derivative)), np.abs(off - derivative).max()
    assert chi_model.pair_factor(0.3, 0.3, 0.1, 1e-6) == 0.0 or chi_model.pair_factor(0.3, 0.3, 0.1, 1e-6) > -1e-300  # no overflow, no NaN
    assert np.isfinite(chi_model.pair_factor(-1e300, 1e300, 0.0, 1e-6))


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
            model.susceptibility((2, 2, 2), q, temperature=0.1, **kwargs)
    for bad in (None, np.zeros((2, 3)), [[0.0, 1.0, 0.0]], [[0.5, 0, 0]], np.zeros((2, 2), dtype=int), [0, 1], [[0, 1, 0, 0]],
                np.zeros((0, 3), dtype=int), np.zeros((2, 2, 3), dtype=int), "000", [[0, 0, 2 ** 70]], np.zeros((1, 3), dtype=bool)):
        with pytest.raises(ValueError):
            model.susceptibility((2, 2, 2), bad, temperature=0.1, energy=0.0)
    for temperature in (0.0, -0.1, np.nan, np.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            model.susceptibility((2, 2, 2), q, temperature=temperature, energy=0.0)
    for mesh in ((4, 4), (4, 0, 4), (4.0, 4.0, 4.0), 4):
        with pytest.raises(ValueError):
            model.susceptibility(mesh, q, temperature=0.1, n_electrons=4)
    for kwargs in ({"convention": 0}, {"convention": 3}, {"convention": "2"}, {"matrix_elements": 1}, {"matrix_elements": None}):
        with pytest.raises(ValueError):
            model.susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, **kwargs)
    with pytest.raises(TypeError):
        model.susceptibility((2, 2, 2), q, 0.1, energy=0.0)  # keyword only
    with pytest.raises(TypeError):
        model.susceptibility((2, 2, 2), q, energy=0.0)  # no default temperature
    with pytest.raises(ValueError):
        one_d.susceptibility((8,), [[1]], temperature=0.1, energy=0.0)
    assert not hasattr(tbmodels_amd.KdotpModel, "susceptibility")
    assert tbmodels_amd.Susceptibility._fields == ("mu", "q", "chi")


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in ("tbk_chi_from_eigensystem", "tbk_susceptibility", "tbk_susceptibility_multi", "tbk_chi_plan", "tbk_chi_timing"):
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
