"""
The NumPy model of the projected density-of-states kernels (tools/pdos_model.py) is what the GPU tests compare csrc/tbk_pdos.hip
with.  Here (CPU) the model is held to facts that do not depend on it: the corner weights against their definition -- the integral
of theta(E - eps) lambda_c over the simplex, by seeded barycentric sampling -- the sum rule against dos_model's filled fraction,
invariance under the order of the corners, and for whole meshes unit weights, partitions, a flat band and the eigenvector weights.
"""

import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import pdos_model as model  # noqa: E402  pylint: disable=wrong-import-position

N_SAMPLES = 4 * 10 ** 6
# sampling error of a mean of N numbers in [0, 1]: sigma <= 0.5 / sqrt(N) = 2.5e-4; 6 sigma.  A wrong formula is off by 1e-2 or more.
SAMPLING_TOL = 1.5e-3


@pytest.mark.parametrize("corners", [(-0.7, -0.1, 0.35, 1.2), (-0.4, 0.25, 0.9)])
def test_corner_weights_are_the_integral_they_stand_for(corners):
    e = np.array(corners)
    n_c = len(e)
    rng = np.random.default_rng(20 + n_c)
    lam = rng.standard_exponential((N_SAMPLES, n_c))
    lam /= lam.sum(axis=1, keepdims=True)  # Dirichlet(1, ..., 1): uniform on the simplex
    eps = lam @ e
    # E in every range: below, inside every interval (two points each), on a corner, above
    inner = [e[i] + f * (e[i + 1] - e[i]) for i in range(n_c - 1) for f in (0.3, 0.8)]
    energies = np.array([e[0] - 0.5] + inner + [e[1], e[-1] + 0.5])
    got = model.corner_weights(e, energies)
    worst = 0.0
    for j, energy in enumerate(energies):
        want = (lam * (eps <= energy)[:, None]).mean(axis=0)
        worst = max(worst, np.abs(got[j] - want).max())
    print("%d corners: max|w - sampled integral| = %.3e" % (n_c, worst))
    assert worst <= SAMPLING_TOL
    assert np.array_equal(got[0], np.zeros(n_c)) and np.array_equal(got[-1], np.full(n_c, 1.0 / n_c))


def _corner_sets(n_c, seed):
    """Random corners, and ones with 2, 3 and all corners tied (in every position once sorted)."""
    rng = np.random.default_rng(seed)
    out = [rng.uniform(-2.0, 3.0, n_c) for _ in range(100)]
    for _ in range(40):
        c = rng.uniform(-2.0, 3.0, n_c)
        i, j = rng.choice(n_c, 2, replace=False)
        c[j] = c[i]
        out.append(c)
    for _ in range(20):
        c = rng.uniform(-2.0, 3.0, n_c)
        idx = rng.choice(n_c, 3, replace=False)
        c[idx] = c[idx[0]]
        out.append(c)
    out.append(np.full(n_c, 0.4))
    if n_c == 4:
        for _ in range(10):
            c = rng.uniform(-2.0, 3.0, 4)
            c[1], c[3] = c[0], c[2]
            out.append(c)
    return out


def _energies(e):
    width = max(e[-1] - e[0], 1.0)
    return np.union1d(np.linspace(e[0] - 0.1 * width, e[-1] + 0.1 * width, 61), e)


@pytest.mark.parametrize("n_c", [3, 4])
def test_corner_weights_sum_to_the_filled_fraction(n_c):
    for corners in _corner_sets(n_c, 300 + n_c):
        e = np.sort(corners)
        grid = _energies(e)
        w = model.corner_weights(e, grid)
        assert w.min() >= -1e-15
        assert np.abs(w.sum(axis=-1) - dos_model.simplex_fraction(e, grid)).max() <= 1e-14, corners


def test_weighted_sum_does_not_depend_on_the_order_of_the_corners():
    rng = np.random.default_rng(41)
    for corners in _corner_sets(4, 304)[::4]:
        a = rng.uniform(0.0, 1.0, 4)
        grid = _energies(np.sort(corners))
        results = []
        for perm in itertools.permutations(range(4)):  # the 24 input orders
            e, w = corners[list(perm)], a[list(perm)]
            order = np.argsort(e, kind="stable")
            results.append(model.corner_weights(e[order], grid) @ w[order])
        assert np.abs(np.array(results) - results[0]).max() <= 1e-14, corners


def _mesh_inputs(mesh, n_orb, n_groups, seed):
    rng = np.random.default_rng(seed)
    eig = np.sort(rng.uniform(-1.0, 1.0, tuple(mesh) + (n_orb,)), axis=-1)
    weights = rng.uniform(0.0, 1.0, tuple(mesh) + (n_groups, n_orb))
    return eig, weights


@pytest.mark.parametrize("mesh", [(3, 2, 4), (5, 4), (1, 1, 1)])
def test_unit_weights_and_partitions_give_the_total(mesh):
    n_orb = 5
    eig, weights = _mesh_inputs(mesh, n_orb, 3, 50 + len(mesh))
    grid = np.linspace(-1.2, 1.2, 49)
    total = dos_model.nos(eig, grid)
    ones = model.pnos(eig, np.ones(tuple(mesh) + (1, n_orb)), grid)
    assert ones.shape == (1, 49)
    assert np.abs(ones[0] - total).max() <= 1e-12 * n_orb
    weights /= weights.sum(axis=-2, keepdims=True)  # every (k, b) spread over the groups: rows sum to 1 over g
    parts = model.pnos(eig, weights, grid)
    assert parts.shape == (3, 49) and parts.min() >= 0.0
    assert np.abs(parts.sum(axis=0) - total).max() <= 1e-12 * n_orb
    assert np.all(np.diff(parts, axis=1) >= -1e-14)


@pytest.mark.parametrize("mesh", [(3, 2, 2), (4, 3)])
def test_flat_band_is_a_clean_step_of_the_mean_weight(mesh):
    rng = np.random.default_rng(60 + len(mesh))
    eig = np.full(tuple(mesh) + (1,), 0.25)
    weights = rng.uniform(0.0, 1.0, tuple(mesh) + (2, 1))
    grid = np.array([-1.0, 0.2499, 0.25, 0.2501, 1.0])
    got = model.pnos(eig, weights, grid)
    mean = weights.reshape(-1, 2).mean(axis=0)
    assert np.array_equal(got[:, :2], np.zeros((2, 2)))
    assert np.abs(got[:, 2:] - mean[:, None]).max() <= 1e-15


def test_band_weights_of_a_unitary_sum_to_one_over_a_partition():
    rng = np.random.default_rng(70)
    mat = rng.standard_normal((6, 7, 7)) + 1j * rng.standard_normal((6, 7, 7))
    unitary = np.linalg.qr(mat)[0]
    groups = [[0, 3], [1], [2, 4, 5, 6]]
    w = model.band_weights(unitary, groups)
    assert w.shape == (6, 3, 7)
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-14
    assert np.abs(w[:, 1, :] - np.abs(unitary[:, 1, :]) ** 2).max() == 0.0
    overlap = model.band_weights(unitary, [[0, 1], [1, 2]])  # an orbital in two groups counts in both
    assert np.abs(overlap.sum(axis=1) - (np.abs(unitary[:, [0, 1, 1, 2], :]) ** 2).sum(axis=1)).max() <= 1e-15
