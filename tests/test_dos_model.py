"""
The NumPy model of the density-of-states kernel (tools/dos_model.py) is what the GPU tests compare csrc/tbk_dos.hip with.
Here (CPU) the model itself is held to facts that do not depend on it: limits, monotonicity and continuity of the filled fraction
of one simplex, the mean-value identity of its integral, and for whole meshes the state count, the step function of a constant
model and the particle-hole symmetry of the cubic cosine band.
"""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model as model  # noqa: E402  pylint: disable=wrong-import-position


def _simplices(n_corners, seed):
    """A few hundred corner sets: generic ones, and ones with 2, 3 and all corners equal (in every position)."""
    rng = np.random.default_rng(seed)
    out = [rng.uniform(-2.0, 3.0, n_corners) for _ in range(200)]
    for _ in range(40):
        c = rng.uniform(-2.0, 3.0, n_corners)
        i, j = rng.choice(n_corners, 2, replace=False)
        c[j] = c[i]  # two equal: lowest, inner or highest pair once sorted
        out.append(c)
    for _ in range(40):
        c = rng.uniform(-2.0, 3.0, n_corners)
        idx = rng.choice(n_corners, 3, replace=False)
        c[idx] = c[idx[0]]  # three equal (a triangle: all)
        out.append(c)
    for _ in range(10):
        out.append(np.full(n_corners, rng.uniform(-2.0, 3.0)))  # a flat band
    if n_corners == 4:
        for _ in range(20):
            c = rng.uniform(-2.0, 3.0, 4)
            c[1], c[3] = c[0], c[2]  # two pairs
            out.append(c)
    return [rng.permutation(c) for c in out]


@pytest.mark.parametrize("n_corners", [3, 4])
def test_simplex_limits_monotonicity_and_continuity(n_corners):
    for corners in _simplices(n_corners, 100 + n_corners):
        e = np.sort(corners)
        width = max(e[-1] - e[0], 1.0)
        below = np.array([e[0] - width, np.nextafter(e[0], -np.inf)])
        assert np.array_equal(model.simplex_fraction(corners, below), [0.0, 0.0])
        above = np.array([e[-1], np.nextafter(e[-1], np.inf), e[-1] + width])
        assert np.array_equal(model.simplex_fraction(corners, above), [1.0, 1.0, 1.0])
        grid = np.union1d(np.linspace(e[0] - 0.1 * width, e[-1] + 0.1 * width, 301), e)
        n = model.simplex_fraction(corners, grid)
        assert np.all(np.diff(n) >= -1e-14) and n.min() >= 0.0 and n.max() <= 1.0 + 1e-14
        if e[-1] > e[0]:  # continuity at every corner that is not a clean step: from just below to the corner itself
            for corner in e:
                left = model.simplex_fraction(corners, np.array([np.nextafter(corner, -np.inf)]))[0]
                at = model.simplex_fraction(corners, np.array([corner]))[0]
                assert abs(at - left) <= 1e-13, (corners, corner, left, at)


@pytest.mark.parametrize("n_corners", [3, 4])
def test_simplex_integral_is_the_corner_mean(n_corners):
    """int_{e1}^{e_top} (1 - n_T) dE = mean(corners) - e1: the mean of a linear function over a simplex is its corner mean.
    Gauss-Legendre with 4 points per polynomial piece is exact for the cubics."""
    x, wq = np.polynomial.legendre.leggauss(4)
    for corners in _simplices(n_corners, 200 + n_corners):
        e = np.sort(corners)
        if e[-1] == e[0]:
            continue
        integral = 0.0
        for lo, hi in zip(e[:-1], e[1:]):
            if hi > lo:
                # nodes are strictly inside the piece: its own branch is the one evaluated
                pts = 0.5 * (hi + lo) + 0.5 * (hi - lo) * x
                integral += 0.5 * (hi - lo) * np.dot(wq, 1.0 - model.simplex_fraction(corners, pts))
        assert abs(integral - (e.mean() - e[0])) <= 1e-12 * (e[-1] - e[0]), (corners, integral, e.mean() - e[0])


@pytest.mark.parametrize("mesh, n_orb", [((3, 4, 5), 3), ((1, 1, 1), 2), ((2, 1, 3), 1), ((5, 4), 3), ((1, 3), 2)])
def test_mesh_counts_every_state_once(mesh, n_orb):
    rng = np.random.default_rng(7)
    eig = np.sort(rng.uniform(-1.0, 1.0, tuple(mesh) + (n_orb,)), axis=-1)
    grid = np.linspace(-1.5, 1.5, 31)
    nos = model.nos(eig, grid)
    assert abs(nos[0]) <= 1e-13 and abs(nos[-1] - n_orb) <= 1e-13
    assert np.all(np.diff(nos) >= -1e-13)
    assert np.allclose(model.dos(eig, grid), np.diff(nos) / (grid[1] - grid[0]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("mesh", [(3, 2, 4), (4, 3)])
def test_constant_model_gives_the_step_function_of_its_levels(mesh):
    levels = np.array([-0.75, 0.25, 0.25, 1.5])  # a doubly degenerate level among them
    eig = np.broadcast_to(levels, tuple(mesh) + (4,))
    grid = np.linspace(-1.0, 2.0, 25)  # multiples of 0.125: -0.75, 0.25 and 1.5 are grid points...
    grid = grid + 0.03                 # ... so the grid is moved away from the levels
    want = (levels[None, :] <= grid[:, None]).sum(axis=1).astype(float)
    assert np.array_equal(model.nos(eig, grid), want)
    # a level ON a grid point counts from that point on (n_T = 1 at and above the top corner)
    on = np.array([0.0, 0.25, 0.5])
    assert np.array_equal(model.nos(eig, on), [1.0, 3.0, 3.0])


@pytest.mark.parametrize("n", [4, 6])
def test_cubic_cosine_band_is_particle_hole_symmetric(n):
    """E = 2 t sum_d cos 2 pi k_d on an even mesh: the half-period shift maps simplices to simplices with negated energies, so
    nos(E) + nos(-E) = 1 on a grid symmetric about 0 that does not contain 0."""
    t = 0.7
    k = model.mesh_kpoints((n, n, n))
    eig = (2.0 * t * np.cos(2 * np.pi * k).sum(axis=1)).reshape(n, n, n, 1)
    grid = np.linspace(-4.5, 4.5, 40)
    assert 0.0 not in grid and np.allclose(grid, -grid[::-1], rtol=0, atol=1e-15)
    nos = model.nos(eig, grid)
    assert np.abs(nos + nos[::-1] - 1.0).max() <= 1e-12
    assert abs(nos[0]) <= 1e-13 and abs(nos[-1] - 1.0) <= 1e-13


def test_mesh_kpoints_are_in_meshgrid_order():
    k = model.mesh_kpoints((2, 3, 4))
    assert k.shape == (24, 3)
    assert np.array_equal(k[1], [0.0, 0.0, 0.25]) and np.array_equal(k[4], [0.0, 1.0 / 3.0, 0.0]) and np.array_equal(k[12], [0.5, 0.0, 0.0])
