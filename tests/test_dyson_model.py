"""
tools/dyson_model.py, the NumPy statement of the dressed lattice Green's function, against numpy.linalg.inv
and against the properties that define the quantity.  No GPU.

Bounds (u = 2^-53), none measured on the code under test: dyson_model.tolerance, i.e. per energy
max_k 8 n u rho kappa_2(A) ||A^-1||_2 + 4 (NK + 32) u max_k ||A^-1||_2 with rho the growth factor of the model's own elimination; a
comparison of two calls is bounded by the sum of their bounds.  The inputs are causal (dyson_model.causal_case), so with
|Im z| >= 0.05 the bound stays below 1e-9, which is asserted.  Every case prints its measured maximum.
"""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dm_model  # noqa: E402  pylint: disable=wrong-import-position
import dyson_model  # noqa: E402  pylint: disable=wrong-import-position
import green_model  # noqa: E402  pylint: disable=wrong-import-position

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])
MESH = (2, 3)
R = np.array([[0, 0], [1, 0], [-1, 0], [2, -1], [1 + 2, 0 - 3]], dtype=np.int64)


def _within(got, want, bound, what):
    err = np.abs(got - want).max(axis=(0, 2, 3))
    print("%s: max|difference| per energy %s (bounds %s)" % (what, " ".join("%.2e" % e for e in err), " ".join("%.2e" % b for b in bound)))
    assert np.all(bound < 1e-9), bound
    assert np.all(err <= bound), (what, err, bound)


@pytest.mark.parametrize("n", [1, 3, 16, 17, 64])
def test_model_matches_the_direct_inverse(n):
    H, sigma = dyson_model.causal_case(n, 6, Z, 4100 + n)
    G, rho = dyson_model.dressed_green_function(H, MESH, Z, sigma, R)
    assert G.shape == (len(R), len(Z), n, n) and rho.shape == (6, len(Z)) and rho.min() >= 1.0
    print("n = %d: growth factor <= %.3f" % (n, rho.max()))
    _within(G, dyson_model.direct(H, MESH, Z, sigma, R), dyson_model.tolerance(H, Z, sigma, rho), "n = %d against direct" % n)
    assert np.array_equal(G[4], G[1])  # R + whole mesh periods: the bits of R


def test_single_inverse_and_its_permutations():
    rng = np.random.default_rng(4200)
    for n in (1, 2, 15, 16, 18, 40):
        A = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
        inverse, rho, prow = dyson_model.invert(A)
        assert sorted(prow) == list(range(n)) and rho >= 1.0
        kappa = np.linalg.cond(A)
        err = np.abs(inverse - np.linalg.inv(A)).max()
        bound = 8 * n * dyson_model.U_ROUND * rho * kappa * np.linalg.norm(np.linalg.inv(A), 2)
        print("n = %d: max|A^-1 - numpy| = %.2e (bound %.2e)" % (n, err, bound))
        assert err <= bound


def test_zero_self_energy_is_the_resolvent():
    n = 5
    H, sigma = dyson_model.causal_case(n, 6, Z, 4300)
    G, rho = dyson_model.dressed_green_function(H, MESH, Z, 0 * sigma, R)
    eig, vec = np.linalg.eigh(H)
    undressed = green_model.green_function(eig, vec, MESH, Z, R)
    bound = dyson_model.tolerance(H, Z, 0 * sigma, rho) + green_model.whole_call_tolerance(H, eig, vec, 0.05, undressed)
    _within(G, undressed, bound, "Sigma = 0 against the undressed model")


def test_scalar_and_hermitian_self_energies_shift_the_problem():
    n = 4
    H, _ = dyson_model.causal_case(n, 6, Z, 4400)
    s = np.array([0.2 - 0.1j, -0.3 + 0.2j, 0.1 - 0.3j, 0.4 + 0.01j, -0.2j])  # causal with Z: Im s of the sign opposite to Im z
    sigma = s[:, None, None] * np.eye(n)[None]
    G, rho = dyson_model.dressed_green_function(H, MESH, Z, sigma, R)
    zero = np.zeros_like(sigma)
    G0, rho0 = dyson_model.dressed_green_function(H, MESH, Z - s, zero, R)
    bound = dyson_model.tolerance(H, Z, sigma, rho) + dyson_model.tolerance(H, Z - s, zero, rho0)
    _within(G, G0, bound, "Sigma = s 1 against z - s")
    rng = np.random.default_rng(4401)
    S = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    S = 0.3 * (S + S.conj().T)
    const = np.broadcast_to(S, (len(Z), n, n))
    G1, rho1 = dyson_model.dressed_green_function(H, MESH, Z, const, R)
    G2, rho2 = dyson_model.dressed_green_function(H + S[None], MESH, Z, zero, R)
    bound = dyson_model.tolerance(H, Z, const, rho1) + dyson_model.tolerance(H + S[None], Z, zero, rho2)
    _within(G1, G2, bound, "Sigma = S against H + S")


def test_conjugation_symmetry():
    n = 6
    H, sigma = dyson_model.causal_case(n, 6, Z, 4500)
    G, rho = dyson_model.dressed_green_function(H, MESH, Z, sigma, R)
    sigma_h = np.conj(np.transpose(sigma, (0, 2, 1)))
    mirror, rho_m = dyson_model.dressed_green_function(H, MESH, np.conj(Z), sigma_h, -R)
    bound = dyson_model.tolerance(H, Z, sigma, rho) + dyson_model.tolerance(H, np.conj(Z), sigma_h, rho_m)
    _within(mirror, np.conj(np.transpose(G, (0, 1, 3, 2))), bound, "G(R, conj z; Sigma^H) against G(-R, z; Sigma)^H")


def test_dyson_equation_on_the_mesh_torus():
    n, mesh = 3, (4, 4)
    rng = np.random.default_rng(4600)
    vectors = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [2, -1]])
    hop = 0.3 * (rng.normal(size=(5, n, n)) + 1j * rng.normal(size=(5, n, n)))
    hop[0] = (hop[0] + hop[0].conj().T) / 4
    torus = green_model.torus_hoppings(mesh, vectors, hop)  # H_torus[cell point]
    cell = np.array([[i, j] for i in range(4) for j in range(4)], dtype=np.int64)
    H = np.einsum("kr,rij->kij", np.conj(dm_model.phases(mesh, cell)).T, torus)  # H(k) = sum_R' exp(+2 pi i k . R') H_torus(R')
    assert np.abs(H - np.conj(np.transpose(H, (0, 2, 1)))).max() < 1e-14
    _, sigma = dyson_model.causal_case(n, 1, Z, 4601)
    G, rho = dyson_model.dressed_green_function(H, mesh, Z, sigma, cell)
    bound = dyson_model.tolerance(H, Z, sigma, rho)
    worst = 0.0
    for zi, z in enumerate(Z):
        for r, vec in enumerate(cell):
            total = np.zeros((n, n), dtype=complex)
            for rp, vecp in enumerate(cell):
                diff = np.mod(vec - vecp, mesh)
                kernel = -torus[rp] + ((z * np.eye(n) - sigma[zi]) if not vecp.any() else 0)
                total += kernel @ G[diff[0] * 4 + diff[1], zi]
            worst = max(worst, np.abs(total - (np.eye(n) if not vec.any() else 0)).max())
    # the residual of 16 n products of (z - Sigma, H_torus) with G, each within its bound
    norm = sum(np.linalg.norm(t, 2) for t in torus) + np.abs(Z).max() + max(np.linalg.norm(s, 2) for s in sigma)
    limit = norm * n * bound.max()
    print("Dyson equation on the torus: max residual %.2e (bound %.2e)" % (worst, limit))
    assert worst <= limit < 1e-8


def test_a_singular_matrix_raises():
    with pytest.raises(np.linalg.LinAlgError):
        dyson_model.invert(np.zeros((3, 3)))
    with pytest.raises(np.linalg.LinAlgError):
        dyson_model.invert(np.array([[1.0, 2.0], [2.0, 4.0]]))  # the second pivot is exactly zero
    H = np.diag([0.5, -0.25]).astype(complex)[None]
    z = np.array([0.1 + 0.1j, 0.3 + 0j])
    sigma = np.array([np.zeros((2, 2)), 0.3 * np.eye(2) - H[0]], dtype=complex)
    with pytest.raises(np.linalg.LinAlgError):
        dyson_model.dressed_green_function(H, (1, 1), z, sigma, np.zeros((1, 2), dtype=np.int64))


def test_pivot_ties_take_the_lowest_row():
    A = np.array([[1.0, 2.0, 0.0], [-1.0, 0.0, 3.0], [1j, 1.0, 1.0]])  # |re| + |im| = 1 in every row of column 0
    inverse, _, prow = dyson_model.invert(A)
    assert prow[0] == 0
    assert np.abs(inverse @ A - np.eye(3)).max() < 1e-14
    # |re| + |im|, not the modulus: 0.6 + 0.6i (modulus 0.85) wins over 1.0
    B = np.array([[1.0, 1.0], [0.6 + 0.6j, 2.0]])
    assert dyson_model.invert(B)[2][0] == 1
    # a taken row is never taken again, and without pivoting the order is the natural one
    C = np.array([[0.0, 1.0], [1.0, 0.0]])
    assert list(dyson_model.invert(C)[2]) == [1, 0]
    with pytest.raises(np.linalg.LinAlgError):
        dyson_model.invert(C, pivoting=False)
