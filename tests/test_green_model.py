"""
tools/green_model.py, the NumPy statement of the lattice Green's function, against the properties that define
the quantity, and the argument checks of `Model.green_function`, which need no device.

Inputs: random Hermitian models (hoppings to 0 and two further cells) on the meshes 2 x 3 x 2, 3 x 4, 1 x 5 and 1 x 1 x 1 with 1, 3
and 9 orbitals; eigensystems of numpy.linalg.eigh; energies of both signs of Im z with |Im z| >= 0.05, one inside the spectrum's real
range.  Bounds (u = 2^-53, eta = min |Im z|), none taken from the code under test:

  tol_g = green_tolerance(NK, n, eta) = 4 (NK n + 32) u / eta: an element of G is a sum of NK n terms whose moduli add up to at
          most 1 / eta.
  against the direct resolvent: 2 max_k (||U U^H - 1|| + ||H U - U E|| ||U|| / eta) / eta + tol_g + 4 n u ||G_ref||
          (green_model.whole_call_tolerance), which must stay below 1e-9 for these inputs.
  the torus Dyson equation: (z - H) U g U^H - 1 = (U U^H - 1) - (H U - U E) g U^H per mesh point, eta times the eigensystem bound;
          plus the error of G (tol_g per element) and the roundings of the cell sum, each at most tol_g times the largest absolute
          row sum of z - H_torus.
  |z| = 10^6: z G(k) - 1 = H (z - H)^-1, at most ||H|| / (|z| - ||H||), plus |z| tol_g at eta = |Im z|.
"""

import ctypes
import itertools
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
import dm_model  # noqa: E402  pylint: disable=wrong-import-position
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import green_model  # noqa: E402  pylint: disable=wrong-import-position

MESHES = [(2, 3, 2), (3, 4), (1, 5), (1, 1, 1)]
ORBITALS = [1, 3, 9]
Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 4.0 + 0.5j, -0.05j, 2.5j])  # 0.3 and -1.1: inside the spectrum's real range
ETA = 0.05
_CACHE = {}


def _system(mesh, n):
    """(R, hop) of the stored half, H(k) (NK, n, n), eigenvalues (NK, n), eigenvectors (NK, n, n): computed once, never written."""
    key = (mesh, n)
    if key not in _CACHE:
        dim = len(mesh)
        rng = np.random.default_rng(900 + 11 * int(np.prod(mesh)) + n)
        R = np.zeros((3, dim), dtype=np.int64)
        R[1, 0], R[2, -1], R[2, 0] = 1, 1, -1
        hop = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
        hop[0] = (hop[0] + hop[0].conj().T) / 4  # the stored half of a Hermitian on-site block
        kpts = dos_model.mesh_kpoints(mesh)
        ham = np.einsum("kr,rij->kij", np.exp(2j * np.pi * (kpts @ R.T)), hop)
        ham = ham + np.conj(np.transpose(ham, (0, 2, 1)))
        eig, vec = np.linalg.eigh(ham)
        for array in (R, hop, ham, eig, vec):
            array.setflags(write=False)
        _CACHE[key] = (R, hop, ham, eig, vec)
    return _CACHE[key]


def _cell(mesh):
    return np.array(list(itertools.product(*[range(x) for x in mesh])), dtype=np.int64)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_the_model_is_the_direct_resolvent(mesh, n):
    _, _, ham, eig, vec = _system(mesh, n)
    R = np.concatenate([_cell(mesh), -_cell(mesh)[-2:], np.array([[5, -7, 3][:len(mesh)]])])
    got = green_model.green_function(eig, vec, mesh, Z, R)
    want = green_model.resolvent(ham, mesh, Z, R)
    bound = green_model.whole_call_tolerance(ham, eig, vec, ETA, want)
    err = np.abs(got - want).max()
    print("mesh %s n = %d: max|model - resolvent| = %.3e (bound %.3e)" % (mesh, n, err, bound))
    assert got.shape == (len(R), len(Z), n, n) and bound < 1e-9 and err <= bound


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_dyson_equation_on_the_mesh_torus(mesh, n):
    R, hop, ham, eig, vec = _system(mesh, n)
    n_k, cell = int(np.prod(mesh)), _cell(mesh)
    h_torus = green_model.torus_hoppings(mesh, R, hop)
    # H(k) is the transform of the folded hoppings: the folding itself
    back = np.einsum("kr,rij->kij", np.conj(dm_model.phases(mesh, cell)).T, h_torus)
    assert np.abs(back - ham).max() <= 1e-12 * max(1.0, np.abs(ham).max())
    G = green_model.green_function(eig, vec, mesh, Z, cell)
    strides = [int(np.prod(mesh[d + 1:])) for d in range(len(mesh))]
    row_sum = float(np.abs(h_torus).sum(axis=(0, 2)).max())
    eb = green_model.eigensystem_bound(ham, eig, vec, ETA)
    for iz, z in enumerate(Z):
        bound = ETA * eb + 2.0 * green_model.green_tolerance(n_k, n, ETA) * (abs(z) + row_sum)
        for r, vec_r in enumerate(cell):
            total = z * G[r, iz]
            for rp, vec_p in enumerate(cell):
                diff = sum(int(np.mod(a - b, m)) * s for a, b, m, s in zip(vec_r, vec_p, mesh, strides))
                total = total - h_torus[rp] @ G[diff, iz]
            want = np.eye(n) if r == 0 else np.zeros((n, n))
            assert np.abs(total - want).max() <= bound, (mesh, n, z, tuple(vec_r), np.abs(total - want).max(), bound)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_conjugate_energy_and_spectral_sum(mesh, n):
    _, _, _, eig, vec = _system(mesh, n)
    n_k, tol = int(np.prod(mesh)), green_model.green_tolerance(int(np.prod(mesh)), n, ETA)
    R = np.random.default_rng(6).integers(-3, 4, size=(6, len(mesh)))
    R[0] = 0
    G, mirror = green_model.green_function(eig, vec, mesh, Z, R), green_model.green_function(eig, vec, mesh, np.conj(Z), -R)
    assert np.abs(mirror - np.conj(np.transpose(G, (0, 1, 3, 2)))).max() <= 2 * tol
    for iz, z in enumerate(Z):
        eta = abs(z.imag)
        lorentz = float(np.sum((eta / np.pi) / ((z.real - eig) ** 2 + eta ** 2))) / n_k
        got = -np.sign(z.imag) * np.trace(G[0, iz]).imag / np.pi
        assert abs(got - lorentz) <= n * tol, (mesh, n, z)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_far_from_the_spectrum_z_times_g_is_the_identity(mesh, n):
    _, _, ham, eig, vec = _system(mesh, n)
    n_k = int(np.prod(mesh))
    R = np.array([[0] * len(mesh), list(mesh), [1] * len(mesh), [-2 * x for x in mesh], [0] * (len(mesh) - 1) + [2]], dtype=np.int64)
    h_norm = float(np.abs(eig).max())
    for z in (1e6j, 6e5 - 8e5j):
        G = green_model.green_function(eig, vec, mesh, [z], R)[:, 0]
        bound = h_norm / (abs(z) - h_norm) + abs(z) * green_model.green_tolerance(n_k, n, abs(z.imag))
        for vector, mat in zip(R, G):
            want = np.eye(n) if np.all(vector % np.array(mesh) == 0) else np.zeros((n, n))
            assert np.abs(z * mat - want).max() <= bound, (mesh, n, z, vector)


@pytest.mark.parametrize("mesh", MESHES)
def test_a_whole_mesh_period_changes_no_bit(mesh):
    dim = len(mesh)
    _, _, _, eig, vec = _system(mesh, 3)
    rng = np.random.default_rng(78)
    R = rng.integers(-5, 6, size=(8, dim)).astype(np.int64)
    R[-1] = [2 ** 31 - 3, -(2 ** 31) + 5, 2 ** 31 - 1][:dim]  # |R_d| near 2^31
    R[-2] = [-(2 ** 31), 2 ** 31 - 1, -(2 ** 31) + 1][:dim]
    base = green_model.green_function(eig, vec, mesh, Z, R)
    for d, n_d in enumerate(mesh):
        for periods in (1, -1, 7, -(2 ** 31) // n_d):
            moved = R.copy()
            moved[:, d] += periods * n_d
            assert np.array_equal(green_model.green_function(eig, vec, mesh, Z, moved), base), (mesh, d, periods)


def test_weights_are_the_reciprocal():
    eig = np.array([[-1.0, 0.25, 3.0]])
    g = green_model.weights(eig, Z)
    assert g.shape == (1, len(Z), 3)
    assert np.abs(g * (Z[None, :, None] - eig[:, None, :]) - 1.0).max() <= 8 * 2.0 ** -53
    assert green_model.green_tolerance(12, 9, 0.05) == 4.0 * (12 * 9 + 32) * 2.0 ** -53 / 0.05


def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    for z in (0.5, 0.5 + 0j, [1j, 2.0], np.nan + 1j, [1j, complex(np.inf, 1.0)], complex(0.0, np.nan), [], [[1j, 2j]], "1j", None):
        with pytest.raises(ValueError):
            model.green_function((2, 2, 2), z)
    with pytest.raises(ValueError):
        model.green_function((2, 2, 2), [1j] * 4097)
    with pytest.raises(ValueError):
        one_d.green_function((4,), 1j)
    for mesh in ((2, 2), (2, 0, 2), (2, 2, 2.5)):
        with pytest.raises(ValueError):
            model.green_function(mesh, 1j)
    for vectors in ([[0, 0]], [[0.5, 0, 0]], np.zeros((0, 3), dtype=int)):
        with pytest.raises(ValueError):
            model.green_function((2, 2, 2), 1j, R=vectors)
    assert not hasattr(tbmodels_amd.KdotpModel, "green_function")
    assert tbmodels_amd.GreenFunction._fields == ("z", "R", "G") and "GreenFunction" in tbmodels_amd.__all__


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_green_from_eigensystem": 13, "tbk_green_function": 7, "tbk_green_function_multi": 8, "tbk_green_plan": 7, "tbk_green_timing": 4}
    for name, count in counts.items():
        found = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert found, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        declared = [" ".join(part.split()) for part in found.group(1).split(",")]
        assert len(declared) == len(argtypes) == count, (name, declared)
        for text, ctype in zip(declared, argtypes):
            if "*" in text:
                assert ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer), (name, text)
            else:
                assert ctype is kinds[text.rsplit(" ", 1)[0]], (name, text)
