"""
tools/chi_model.py `susceptibility_tensor`, the NumPy statement of the four-index bare static susceptibility chi_0[i, l; j, m](q)
(DESIGN.md section 29), against the properties that define the quantity, the factorised form the kernels use, the orbital-resolved
and scalar models of the same file, the formula as written, and the argument checks of `Model.susceptibility_tensor`, which need no
device.

Inputs: random ascending bands with a flat band and an exact degenerate pair in every k-point, random unitary U, on the meshes
2 x 3 x 2, 3 x 4, 1 x 5 and 1 x 1 x 1 with 1, 3 and 9 orbitals, mu inside the bands, T in {0.05, 0.5}.  Bound: chi_model.tensor_tolerance
 per component of an entry for every comparison of two evaluations; the model hands the n^2 m^4 part to BLAS, so among
the identities of bits only those that repeat the same products (properties 6, 7, duplicates, exact Hermiticity) are asserted as such
on it, and property 10 within the bound -- the kernels' test asserts it bit for bit.
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
_CHI = {}


def _eigensystem(mesh, n):
    """As `_eigensystem` of tests/test_gpu_chi.py: band 0 flat, bands 1 and 2 an exact degenerate pair, random unitary U; and random
    positions.  Computed once, never written."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(7300 + 41 * n_k + n)
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


def _chi(mesh, n, T, q=None, mu=MU, U=None, orbitals=None):
    eig, vec, _ = _eigensystem(mesh, n)
    q = _vectors(mesh)[0] if q is None else q
    return chi_model.susceptibility_tensor(eig, vec if U is None else U, mesh, q, mu, T, orbitals)


def _shared(mesh, n, T):
    """The model on the case's vectors: computed once, shared by the tests and never written."""
    key = (mesh, n, T)
    if key not in _CHI:
        _CHI[key] = _chi(mesh, n, T)
        _CHI[key].setflags(write=False)
    return _CHI[key]


def _parts(z):
    z = np.asarray(z)
    return max(np.abs(z.real).max(), np.abs(z.imag).max())


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _matrix(chi):
    m = chi.shape[-1]
    return np.ascontiguousarray(chi).reshape(chi.shape[:-4] + (m * m, m * m))


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_hermitian_psd_blocks_inversion_and_high_temperature(mesh, n):
    eig, vec, _ = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    worst = [0.0, 0.0, 0.0, 0.0, np.inf]
    for T in TEMPERATURES:
        tol, tol_orb, tol_scalar = chi_model.tensor_tolerance(n_k, n, T), chi_model.orbital_tolerance(n_k, n, T), chi_model.tolerance(n_k, n, T)
        chi = _shared(mesh, n, T)
        assert chi.shape == (len(q), n, n, n, n) and chi.dtype == np.complex128 and np.all(np.isfinite(_bits(chi)))
        # property 1, and the form of the output: exactly Hermitian as a matrix (i, l) x (j, m), the diagonal's imaginary part +0, no -0
        matrix = _matrix(chi)
        assert np.array_equal(matrix, np.conj(np.swapaxes(matrix, 1, 2)))
        assert np.array_equal(chi, np.conj(chi.transpose(0, 3, 4, 1, 2)))
        diagonal = np.ascontiguousarray(np.diagonal(matrix, axis1=1, axis2=2).imag)
        assert np.all(diagonal == 0.0) and not np.any(np.signbit(_bits(chi)) & (_bits(chi) == 0.0))
        lowest = np.linalg.eigvalsh(matrix).min()
        worst[4] = min(worst[4], lowest)
        assert lowest >= -tol * n * n, (mesh, n, T, lowest)
        # property 2: the density-density block is the orbital-resolved chi_0[i, j]
        block = np.einsum("qiijj->qij", chi)
        gap = _parts(block - chi_model.orbital_susceptibility(eig, vec, mesh, q, MU, T))
        worst[0] = max(worst[0], gap / (tol + tol_orb))
        assert gap <= tol + tol_orb, (mesh, n, T, gap)
        # property 3: its sum over (i, j) is the scalar chi_0(q)
        total = block.sum(axis=(1, 2))
        scalar = chi_model.susceptibility(eig, vec, mesh, q, MU, T)
        worst[1] = max(worst[1], np.abs(total.real - scalar).max() / (n * n * tol + tol_scalar))
        assert np.all(np.abs(total.real - scalar) <= n * n * tol + tol_scalar) and np.all(np.abs(total.imag) <= n * n * tol)
        # property 4: chi(-q)[i, l; j, m] = chi(q)[m, j; l, i]; q = 0 is its own partner
        for a, b in zip(at["plus"] + [0], at["minus"] + [0]):
            gap = _parts(chi[b] - chi[a].transpose(3, 2, 1, 0))
            worst[2] = max(worst[2], gap / tol)
            assert gap <= tol, (mesh, n, T, a, b, gap)
    hot = 1e9 * max(float(np.ptp(eig)), 1.0)
    unit = np.einsum("ij,lm->iljm", np.eye(n), np.eye(n))[None]
    gap = _parts(4.0 * hot * _chi(mesh, n, hot) - unit)  # property 5
    worst[3] = gap
    assert gap <= 4.0 * hot * chi_model.tensor_tolerance(n_k, n, hot) + 1e-8  # (h(y) - 1 and 4 f (1 - f) - 1 are of the order 1 / hot)
    print("mesh %s n = %d: density block %.2e, sum rule %.2e and inversion %.2e of the bound, |4 T chi - 1| %.2e, lowest eigenvalue %.3e"
          % ((mesh, n) + tuple(worst)))


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_far_outside_the_spectrum_every_bit_is_zero(mesh, n):
    eig, _, _ = _eigensystem(mesh, n)
    q = _vectors(mesh)[0][:4]
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):
            for function in (chi_model.susceptibility_tensor, chi_model.susceptibility_tensor_factored):
                flat = _bits(function(eig, _eigensystem(mesh, n)[1], mesh, q, mu, T))
                assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (mesh, n, T, mu)  # property 6


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
        gap = _parts(_shared(mesh, n, T) - _chi(mesh, n, T, U=turned))  # property 8
        # the turned eigenvectors are another input, each of its entries off by a few u: twice the bound covers both evaluations
        assert gap <= 2.0 * chi_model.tensor_tolerance(n_k, n, T) + 16 * n * 2.0 ** -53 / T, (mesh, n, T, gap)


# selections for property 10 that fit n: a single orbital, a shuffled subset with the last orbital, a pair, all of them reversed
SELECTIONS = {1: ([0],), 3: ([1], [2, 0], [2, 1, 0]), 9: ([4], [8, 0, 3], [2, 1], list(range(8, -1, -1)))}


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_bits_do_not_depend_on_the_list_and_selections_agree(mesh, n):
    n_k = int(np.prod(mesh))
    q, at = _vectors(mesh)
    T = TEMPERATURES[0]
    tol = chi_model.tensor_tolerance(n_k, n, T)
    chi = _shared(mesh, n, T)
    assert np.array_equal(_bits(chi[at["duplicate"][0]]), _bits(chi[at["duplicate"][1]]))  # property 9
    assert np.array_equal(_bits(chi[at["full"]]), _bits(chi[at["shifted"]]))  # property 7
    order = np.random.default_rng(3).permutation(len(q))
    assert np.array_equal(_bits(chi[order]), _bits(_chi(mesh, n, T, q=np.ascontiguousarray(q[order]))))
    for chosen in SELECTIONS[n]:  # property 10 (the model: within the bound)
        part = _chi(mesh, n, T, orbitals=chosen)
        assert part.shape == (len(q),) + (len(chosen),) * 4
        assert _parts(part - chi[:, chosen][:, :, chosen][:, :, :, chosen][:, :, :, :, chosen]) <= tol, (mesh, n, T, chosen)
    eig, vec, _ = _eigensystem(mesh, n)
    for function in (chi_model.susceptibility_tensor, chi_model.susceptibility_tensor_factored, chi_model.susceptibility_tensor_naive):
        for bad in ([], [0, 0], [n], [-1], [0.0], [[0]]):
            with pytest.raises(ValueError):
                function(eig, vec, mesh, q, MU, T, bad)
        with pytest.raises(ValueError):
            function(eig, vec, mesh, q.astype(float), MU, T)


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_the_definition_against_the_factored_form(mesh, n):
    """The einsum over (k, b, b') all at once against P Q, the kernels' algebra: two evaluations of the same numbers."""
    eig, vec, _ = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, _ = _vectors(mesh)
    for T in TEMPERATURES:
        tol = chi_model.tensor_tolerance(n_k, n, T)
        for chosen in (None, SELECTIONS[n][-1], SELECTIONS[n][0]):
            want = _shared(mesh, n, T) if chosen is None else _chi(mesh, n, T, orbitals=chosen)
            got = chi_model.susceptibility_tensor_factored(eig, vec, mesh, q, MU, T, chosen)
            assert got.shape == want.shape and _parts(got - want) <= tol, (mesh, n, T, chosen, _parts(got - want), tol)
    print("mesh %s n = %d: max |definition - factored| / bound = %.3e" % (mesh, n, _parts(got - want) / tol))


@pytest.mark.parametrize("n", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_model_against_the_formula_as_written(mesh, n):
    """F as the quotient (f(a) - f(b)) / (a - b), f' on the diagonal, in one einsum over (k, b, b').  Condition and allowance as in
    tests/test_chi_orbital_model.py: |E - mu| / T < 709, and the difference as written is off by under 17 u in absolute terms, which
    the division by a - b makes 17 u / gap per unit of the moduli, gap the smallest non-zero level difference of the case."""
    eig, vec, _ = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, _ = _vectors(mesh)
    worst = 0.0
    assert np.abs(eig - MU).max() / min(TEMPERATURES) < 709.0
    diffs = np.abs(eig.reshape(-1)[:, None] - eig.reshape(-1)[None, :])
    gap = diffs[diffs > 0.0].min() if np.any(diffs > 0.0) else 1.0
    for T in TEMPERATURES:
        want = chi_model.susceptibility_tensor_naive(eig, vec, mesh, q, MU, T)
        allowance = chi_model.tensor_tolerance(n_k, n, T) + 17.0 * 2.0 ** -53 / gap
        worst = max(worst, _parts(_shared(mesh, n, T) - want) / allowance)
        assert _parts(_shared(mesh, n, T) - want) <= allowance, (mesh, n, T, allowance)
    print("mesh %s n = %d: max |model - formula as written| / allowance = %.3e" % (mesh, n, worst))


def test_the_index_order_is_that_of_graser_and_the_convention_1_block():
    """chi_{l1 l2 l3 l4} of Graser et al. (2009) has the numerator a_mu^{l4}(k) a_mu^{l2 *}(k) a_nu^{l1}(k+q) a_nu^{l3 *}(k+q), mu a band of
    k and nu one of k+q: written out with explicit loops and compared with chi[q, l2, l1, l4, l3].  And on the block i = l, j = m the
    convention-1 orbital susceptibility is D_i conj(D_j) chi[i, i, j, j]."""
    mesh, n, T = (3, 4), 3, 0.05
    eig, vec, pos = _eigensystem(mesh, n)
    q = np.array([[1, 2], [-1, 1]], dtype=np.int64)
    chi = chi_model.susceptibility_tensor(eig, vec, mesh, q, MU, T)
    tol = chi_model.tensor_tolerance(12, n, T)
    for index, vector in enumerate(q):
        to = chi_model.shifted_points(mesh, vector)
        graser = np.zeros((n, n, n, n), dtype=complex)
        for k in range(12):
            factor = chi_model.pair_factor(eig[k][:, None], eig[to[k]][None, :], MU, T)  # [mu, nu]
            a_k, a_kq = vec[k], vec[to[k]]  # a^l_band = [l, band]
            for l1 in range(n):
                for l2 in range(n):
                    for l3 in range(n):
                        for l4 in range(n):
                            numerator = (a_k[l4, :, None] * a_k[l2, :, None].conj()) * (a_kq[l1, None, :] * a_kq[l3, None, :].conj())
                            graser[l1, l2, l3, l4] -= (factor * numerator).sum() / 12
        assert _parts(graser - chi[index].transpose(1, 0, 3, 2)) <= tol
        assert _parts(graser - np.transpose(chi, (0, 2, 1, 4, 3))[index]) <= tol
    first = chi_model.orbital_susceptibility(eig, vec, mesh, q, MU, T, chi_model.phase_table(mesh, q, pos))
    table = chi_model.phase_table(mesh, q, pos)
    block = np.einsum("qiijj->qij", chi) * table[:, :, None] * table[:, None, :].conj()
    assert _parts(first - block) <= tol + chi_model.orbital_tolerance(12, n, T)


def test_the_tolerance_is_the_documented_formula():
    u = 2.0 ** -53
    n_k, n, T = 12, 9, 0.05
    c_e = c_m = 2
    c_t = 10  # two complex products of two eigenvector factors (three roundings per component each), the scale by t, the product of the pairs (three)
    assert chi_model.ROUNDINGS_TENSOR == c_t and chi_model.ULP_EXP == c_e and chi_model.ULP_EXPM1 == c_m
    want = 2 * ((n_k * n * n + 4 * c_e + c_m + 15 + c_t) / 4 + 4) * u / T
    assert np.isclose(chi_model.tensor_tolerance(n_k, n, T), want, rtol=1e-14)
    assert np.isclose(want, (n_k * n * n / 2 + 25.5) * u / T, rtol=1e-14)
    for n_k, n in ((1, 1), (1, 2), (12, 9), (4096, 64)):  # the two-level sum of the factorised form has fewer additions than the flat one
        assert (n - 1) + (n_k * n - 1) <= n_k * n * n


# ---- the public interface -----------------------------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)
    big = tbmodels_amd.Model(hop={(0, 0, 0): np.eye(17, dtype=complex) / 2}, size=17, dim=3, contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    q = [[1, 0, 0]]
    for kwargs in ({}, {"energy": 0.0, "n_electrons": 4}, {"energy": np.nan}, {"n_electrons": 0}, {"n_electrons": 8}):
        with pytest.raises(ValueError):
            model.susceptibility_tensor((2, 2, 2), q, temperature=0.1, **kwargs)
    for bad in (None, np.zeros((2, 3)), [[0.5, 0, 0]], [0, 1], "000"):
        with pytest.raises(ValueError):
            model.susceptibility_tensor((2, 2, 2), bad, temperature=0.1, energy=0.0)
    for bad in ([], [0, 0], [8], [-1], [0.0, 1.0], [[0, 1]], "01", [True, False], [None], np.zeros((0,), dtype=int), [2 ** 70], {"orbitals": 1},
                np.array([1], dtype=np.uint64)):  # the checks of orbital_susceptibility, by the same helper
        with pytest.raises(ValueError):
            model.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=bad)
    with pytest.raises(ValueError, match="up to 16 selected orbitals, got 17"):
        big.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0)
    with pytest.raises(ValueError, match="up to 16 selected orbitals, got 17"):
        big.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=list(range(16, -1, -1)))
    for temperature in (0.0, -0.1, np.nan, "0.1", None):
        with pytest.raises(ValueError):
            model.susceptibility_tensor((2, 2, 2), q, temperature=temperature, energy=0.0)
    for mesh in ((4, 4), (4, 0, 4), 4):
        with pytest.raises(ValueError):
            model.susceptibility_tensor(mesh, q, temperature=0.1, n_electrons=4)
    for kwargs in ({"convention": 2}, {"convention": 1}, {"matrix_elements": True}):  # convention 2 only: there is no such argument
        with pytest.raises(TypeError):
            model.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, **kwargs)
    with pytest.raises(TypeError):
        model.susceptibility_tensor((2, 2, 2), q, 0.1, energy=0.0)  # keyword only
    with pytest.raises(ValueError):
        one_d.susceptibility_tensor((8,), [[1]], temperature=0.1, energy=0.0)
    for call in (lambda: model.orbital_susceptibility((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=[1, 1]),
                 lambda: model.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=[1, 1])):
        with pytest.raises(ValueError, match=r"orbitals must be distinct, got \[1, 1\]"):  # one helper, one wording
            call()
    assert not hasattr(tbmodels_amd.KdotpModel, "susceptibility_tensor")
    assert tbmodels_amd.SusceptibilityTensor._fields == ("mu", "q", "orbitals", "chi") and "SusceptibilityTensor" in tbmodels_amd.__all__


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in ("tbk_chi_tensor_from_eigensystem", "tbk_susceptibility_tensor", "tbk_susceptibility_tensor_multi", "tbk_chi_tensor_plan"):
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
    assert "phases" not in re.search(r"\bint tbk_chi_tensor_from_eigensystem\(([^;]*)\);", header).group(1)
