"""
tools/optics_model.py, the NumPy statement of the optical conductivity every GPU test compares with, checked on
the CPU: against the formula as written in a triple loop, against the central difference of `oracle.hamilton`, its two statements of
convention 1 against each other, against the Chern number of the Qi-Wu-Zhang model and against two closed forms.  Then the public
interface without a device: the ctypes signatures of the new entry points and every argument error of `Model.optical_conductivity`.
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
from oracle import tbk_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import berry_model  # noqa: E402  pylint: disable=wrong-import-position
import chi_model  # noqa: E402  pylint: disable=wrong-import-position
import optics_model  # noqa: E402  pylint: disable=wrong-import-position

OMEGA = np.array([0.0, 0.2, -0.2, 0.7, -0.7, 1e6, -1e6, 0.2])
_CACHE = {}


def _random_model(dim, n=4):
    """Packed half-space hoppings of a random n-orbital model with lattice vectors up to |R| = 2, and positions in the cell."""
    key = (dim, n)
    if key not in _CACHE:
        rng = np.random.default_rng(5300 + 10 * dim + n)
        r_vec = np.array([[0] * dim, [1] + [0] * (dim - 1), [0, 1] + [0] * (dim - 2), [1, -1] + [0] * (dim - 2), [2, 0] + [1] * (dim - 2)],
                         dtype=np.int64)
        hop = rng.normal(size=(len(r_vec), n, n)) + 1j * rng.normal(size=(len(r_vec), n, n))
        hop[0] = (hop[0] + hop[0].conj().T) / 4.0
        pos = rng.uniform(0.0, 1.0, (n, dim))
        for array in (r_vec, hop, pos):
            array.setflags(write=False)
        _CACHE[key] = (r_vec, hop, pos)
    return _CACHE[key]


def _parts(z):
    return float(np.maximum(np.abs(np.real(z)), np.abs(np.imag(z))).max())


def _eigensystem(r_vec, hop, mesh):
    k = optics_model.mesh_kpoints(mesh)
    E, U = np.linalg.eigh(oracle.hamilton(r_vec, hop, k, 2))
    return k, E, U, optics_model.derivatives(r_vec, hop, k)


# ---- 1. the two statements of sigma --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(3, 4), (2, 3, 2)])
@pytest.mark.parametrize("with_pos", [False, True])
def test_model_against_the_formula_as_written(mesh, with_pos):
    """The quotient -(f - f') / (E - E') is well conditioned here: T = 0.3 against level spacings of order 1, no exact degeneracy."""
    r_vec, hop, pos = _random_model(len(mesh))
    k, E, U, D = _eigensystem(r_vec, hop, mesh)
    mu, T, eta = 0.1, 0.3, 0.05
    got = optics_model.conductivity(E, U, D, mu, T, OMEGA, eta, pos if with_pos else None)
    want = optics_model.conductivity_naive(E, U, D, mu, T, OMEGA, eta, pos if with_pos else None)
    norm = optics_model.velocity_norm(D, E, pos if with_pos else None)
    gaps = np.abs(E[:, :, None] - E[:, None, :])[:, ~np.eye(E.shape[1], dtype=bool)]
    # the quotient loses u / (relative gap) digits on top of the stable form's bound
    lost = 2.0 ** -52 * (np.abs(E).max() / gaps.min()) * norm ** 2 / (T * eta) * E.shape[1] ** 2
    tol = optics_model.tolerance(len(k), E.shape[1], T, eta, 2.0 * np.ptp(E) + np.abs(OMEGA), norm, 3 if with_pos else 2)[:, None, None] + lost
    err = np.maximum(np.abs((got - want).real), np.abs((got - want).imag))
    print("mesh %s, positions %s: max|model - formula| = %.3e (bound %.3e - %.3e), max|sigma| = %.3e" % (mesh, with_pos, err.max(), tol.min(), tol.max(),
                                                                                                        np.abs(got).max()))
    assert got.shape == (len(OMEGA), len(mesh), len(mesh)) and np.all(err <= tol)
    assert np.array_equal(got[1], got[7])  # a duplicate frequency
    # property 1 and property 2 of the model itself
    assert _parts(got[2] - got[1].conj()) <= tol.max() and _parts(got[4] - got[3].conj()) <= tol.max()
    for sigma in got:
        assert np.linalg.eigvalsh((sigma + sigma.conj().T) / 2.0).min() >= -tol.max()


# ---- 2. the derivative ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_derivative_against_the_central_difference_of_the_oracle(dim):
    r_vec, hop, pos = _random_model(dim)
    k = optics_model.mesh_kpoints((3, 4) if dim == 2 else (2, 3, 2)) + 0.0137
    for convention in (2, 1):
        h, tol = optics_model.derivative_step(r_vec, hop, pos if convention == 1 else None)
        for axis in range(dim):
            step = np.zeros(dim)
            step[axis] = h
            difference = (oracle.hamilton(r_vec, hop, k + step, convention, pos=pos) - oracle.hamilton(r_vec, hop, k - step, convention, pos=pos)) / (4.0 * np.pi * h)
            mine = optics_model.derivative(r_vec, hop, k, axis) if convention == 2 else optics_model.derivative_convention1(r_vec, hop, k, axis, pos)
            err = np.abs(difference - mine).max()
            print("dim %d convention %d axis %d: max|central difference - D| = %.3e (h = %.2e, bound %.3e)" % (dim, convention, axis, err, h, tol))
            assert err <= tol
            assert np.abs(mine - mine.conj().transpose(0, 2, 1)).max() == 0.0  # Hermitian by construction
    assert optics_model.derivatives(r_vec, hop, k).shape == (len(k), dim, 4, 4)


# ---- 3. convention 1, two ways -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(3, 4), (2, 3, 2)])
def test_the_two_statements_of_convention_1_agree(mesh):
    r_vec, hop, pos = _random_model(len(mesh))
    k, E, U, D = _eigensystem(r_vec, hop, mesh)
    mu, T, eta = 0.1, 0.3, 0.05
    band_basis = optics_model.conductivity(E, U, D, mu, T, OMEGA, eta, pos)
    direct = optics_model.conductivity_convention1(r_vec, hop, pos, mesh, mu, T, OMEGA, eta)
    plain = optics_model.conductivity(E, U, D, mu, T, OMEGA, eta)
    norm = optics_model.velocity_norm(D, E, pos)
    # two eigensolves of unitarily equivalent matrices: each side's backward error enters through `shift`
    shift = optics_model.eigensolver_shift(oracle.hamilton(r_vec, hop, k, 2))
    tol = optics_model.tolerance(len(k), E.shape[1], T, eta, 2.0 * np.ptp(E) + np.abs(OMEGA), norm, 3, shift=shift)[:, None, None]
    gap = band_basis - direct
    err = np.maximum(np.abs(gap.real), np.abs(gap.imag))
    moved = _parts(band_basis[0] - plain[0])
    print("mesh %s: max|band-basis term - direct derivative| = %.3e (bound %.3e - %.3e); the term itself moves sigma(0) by %.3e" % (mesh, err.max(), tol.min(),
                                                                                                                         tol.max(), moved))
    assert np.all(err <= tol) and moved > 100.0 * tol[0, 0, 0]  # the sign matters: the wrong one would be off by twice the term


# ---- 4. the Hall plateau of the Qi-Wu-Zhang model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("u_par", [-1.0, 1.0, 3.0])
def test_qwz_hall_conductivity_is_the_chern_number(u_par):
    mesh, eta, T, mu = (12, 12), 0.05, 0.02, 0.0
    r_vec, hop = optics_model.qwz_packed(u_par)
    k, E, U, D = _eigensystem(r_vec, hop, mesh)
    sigma = optics_model.conductivity(E, U, D, mu, T, [0.0], eta)[0]
    chern = int(berry_model.berry_flux(U, mesh, 1)["chern"][0][0, 0])
    hall = 2.0 * np.pi * sigma[0, 1].real
    print("QWZ u = %+g on 12 x 12: 2 pi sigma_xy(0) = %+.6f, C = %+d, deviation %.2e; sigma_yx + sigma_xy = %.2e" % (u_par, hall, chern, abs(hall - chern),
                                                                                                                  abs(sigma[1, 0] + sigma[0, 1])))
    assert chern == {-1.0: -1, 1.0: 1, 3.0: 0}[u_par]
    assert abs(hall - chern) <= 2e-3
    rounding = optics_model.tolerance(len(k), 2, T, eta, 2.0 * np.ptp(E), optics_model.velocity_norm(D))
    assert abs(sigma[1, 0] + sigma[0, 1]) <= rounding


# ---- 5. closed forms -----------------------------------------------------------------------------------------------------------------
def test_a_single_flat_band_does_not_conduct():
    r_vec = np.array([[0, 0], [1, 0]], dtype=np.int64)
    hop = np.array([[[0.35]], [[0.0]]], dtype=np.complex128)
    k, E, U, D = _eigensystem(r_vec, hop, (3, 4))
    sigma = optics_model.conductivity(E, U, D, 0.6, 0.1, OMEGA, 0.05)
    assert np.all(sigma == 0.0)


def test_one_band_cosine_model_is_the_drude_form():
    """E(k) = 2 t1 cos 2 pi k_x + 2 t2 cos 2 pi k_y: V^a = -2 t_a sin 2 pi k_a, sigma = i / (omega + i eta) <-f' v_a v_c>."""
    t1, t2, mesh, mu, T, eta = 0.8, -0.5, (6, 5), 0.3, 0.25, 0.05
    r_vec = np.array([[1, 0], [0, 1]], dtype=np.int64)
    hop = np.array([[[t1]], [[t2]]], dtype=np.complex128)
    k, E, U, D = _eigensystem(r_vec, hop, mesh)
    energy = 2.0 * t1 * np.cos(2 * np.pi * k[:, 0]) + 2.0 * t2 * np.cos(2 * np.pi * k[:, 1])
    speed = np.stack([-2.0 * t1 * np.sin(2 * np.pi * k[:, 0]), -2.0 * t2 * np.sin(2 * np.pi * k[:, 1])], axis=1)
    got = optics_model.conductivity(E, U, D, mu, T, OMEGA, eta)
    want = optics_model.drude(energy, speed, mu, T, OMEGA, eta)
    # the closed form rounds its own cos and sin: E within 2 u (|t1| + |t2|) twice over and v within 2 u relative, as `shift` and `extra`
    tol = optics_model.tolerance(len(k), 1, T, eta, 2.0 * np.ptp(E) + np.abs(OMEGA), optics_model.velocity_norm(D), extra=2.0,
                                 shift=4.0 * 2.0 ** -53 * (abs(t1) + abs(t2)))[:, None, None]
    err = np.maximum(np.abs((got - want).real), np.abs((got - want).imag))
    print("one-band cosine model on %s: max|model - Drude form| = %.3e (bound %.3e), max|sigma| = %.3e" % (mesh, err.max(), tol.min(), np.abs(got).max()))
    assert np.all(err <= tol) and np.abs(got[0, 0, 0]) > 0.1


def test_cartesian_transform_and_tolerance_formula():
    uc = np.array([[2.0, 0.0], [0.5, 1.5]])
    sigma = np.arange(8, dtype=float).reshape(2, 2, 2) + 1j
    want = np.array([uc.T @ s @ uc for s in sigma]) / 3.0
    assert np.allclose(optics_model.cartesian(sigma, uc), want, rtol=1e-15)
    u = 2.0 ** -53
    n_k, n, T, eta, spread, norm = 12, 9, 0.05, 1e-3, 5.0, 3.0
    written = 2.0 * (n_k * n * n + 58 + spread / eta + 2 * 2 * (2 * n + 3) * np.sqrt(n)) * norm ** 2 / (4 * T * eta) * u
    assert np.isclose(optics_model.tolerance(n_k, n, T, eta, spread, norm), written, rtol=1e-14)
    third = optics_model.tolerance(n_k, n, T, eta, np.array([1.0, 5.0]), norm, 3, extra=7.0)
    assert third.shape == (2,) and third[1] > optics_model.tolerance(n_k, n, T, eta, 5.0, norm) > third[0] * 0.0
    moved = 2.0 * (n_k * n * n + 58 + spread / eta + 2 * 2 * (2 * n + 3) * np.sqrt(n) + 2 * (1 / eta + 1 / T) * 1e-15 / u) * norm ** 2 / (4 * T * eta) * u
    assert np.isclose(optics_model.tolerance(n_k, n, T, eta, spread, norm, shift=1e-15), moved, rtol=1e-14)
    assert chi_model.ULP_EXP == 2.0 and chi_model.ULP_EXPM1 == 2.0 and chi_model.ULP_DIV == 2.0  # the 58 above


# ---- 6. the public interface ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("tbk_optical_conductivity", "tbk_optical_conductivity_multi", "tbk_optics_from_eigensystem", "tbk_optics_plan", "tbk_optics_timing",
               "tbk_hamilton_derivative_device")


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
    assert len(_lib.SIGNATURES["tbk_optics_from_eigensystem"][1]) == 15  # (device, dim, n_orb, nk, E, U, D, pos, mu, T, n_w, omega, eta, part_bytes, sigma)


def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    bare = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    omega = [0.0, 0.5]
    for kwargs in ({}, {"energy": 0.0, "n_electrons": 4}, {"energy": np.nan}, {"energy": "0"}, {"n_electrons": 0}, {"n_electrons": 8},
                   {"n_electrons": np.nan}, {"n_electrons": "4"}):
        with pytest.raises(ValueError):
            model.optical_conductivity((2, 2, 2), omega, eta=0.05, temperature=0.1, **kwargs)
    for bad in (None, "0.1", [], [[0.1, 0.2]], np.zeros((0,)), [0.1, np.nan], [np.inf], [-np.inf, 0.0], [0.1 + 0.2j], [True, False], ["0.1"],
                np.zeros((2, 2, 2)), [None], {"omega": 1.0}):
        with pytest.raises(ValueError):
            model.optical_conductivity((2, 2, 2), bad, eta=0.05, temperature=0.1, energy=0.0)
    for eta in (0.0, -0.1, np.nan, np.inf, "0.1", None, True, 1e-200, [0.05]):
        with pytest.raises(ValueError):
            model.optical_conductivity((2, 2, 2), omega, eta=eta, temperature=0.1, energy=0.0)
    for temperature in (0.0, -0.1, np.nan, np.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            model.optical_conductivity((2, 2, 2), omega, eta=0.05, temperature=temperature, energy=0.0)
    for mesh in ((4, 4), (4, 0, 4), (4.0, 4.0, 4.0), 4):
        with pytest.raises(ValueError):
            model.optical_conductivity(mesh, omega, eta=0.05, temperature=0.1, n_electrons=4)
    for kwargs in ({"convention": 0}, {"convention": 3}, {"convention": "2"}, {"cartesian": 1}, {"cartesian": None}):
        with pytest.raises(ValueError):
            model.optical_conductivity((2, 2, 2), omega, eta=0.05, temperature=0.1, energy=0.0, **kwargs)
    with pytest.raises(ValueError, match="cartesian=True needs the unit cell"):
        bare.optical_conductivity((2, 2, 2), omega, eta=0.05, temperature=0.1, energy=0.0, cartesian=True)
    with pytest.raises(TypeError):
        model.optical_conductivity((2, 2, 2), omega, 0.05, temperature=0.1, energy=0.0)  # keyword only
    with pytest.raises(TypeError):
        model.optical_conductivity((2, 2, 2), omega, temperature=0.1, energy=0.0)  # no default broadening
    with pytest.raises(TypeError):
        model.optical_conductivity((2, 2, 2), omega, eta=0.05, energy=0.0)  # no default temperature
    with pytest.raises(ValueError, match="needs a 2- or 3-dimensional model"):
        one_d.optical_conductivity((8,), omega, eta=0.05, temperature=0.1, energy=0.0)
    # the wording the methods share is the same text
    q = [[1, 0, 0]]
    for call in (lambda: model.dynamic_susceptibility((2, 2, 2), q, omega, eta=0.05, temperature=-1.0, energy=0.0),
                 lambda: model.optical_conductivity((2, 2, 2), omega, eta=0.05, temperature=-1.0, energy=0.0)):
        with pytest.raises(ValueError, match="temperature must be finite and positive, got -1.0"):
            call()
    for call in (lambda: model.dynamic_susceptibility((2, 2, 2), q, [np.nan], eta=0.05, temperature=0.1, energy=0.0),
                 lambda: model.optical_conductivity((2, 2, 2), [np.nan], eta=0.05, temperature=0.1, energy=0.0)):
        with pytest.raises(ValueError, match="omega must be finite"):
            call()
    for call in (lambda: model.dynamic_susceptibility((2, 2, 2), q, omega, eta=1e-200, temperature=0.1, energy=0.0),
                 lambda: model.optical_conductivity((2, 2, 2), omega, eta=1e-200, temperature=0.1, energy=0.0)):
        with pytest.raises(ValueError, match="its square underflows"):
            call()
    assert not hasattr(tbmodels_amd.KdotpModel, "optical_conductivity") and not hasattr(tbmodels_amd.Model, "velocity")
    assert tbmodels_amd.OpticalConductivity._fields == ("mu", "omega", "sigma")
