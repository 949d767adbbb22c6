"""
The exact rational reference of the tetrahedron method (tools/tetra_exact.py), and the two NumPy models held to it (CPU).

1. The reference against values worked by hand, as Fraction equalities.  The hand values of (0, 1, 2, 3) come from the geometry
   (E = 1: the simplex cut off at corner 1 has edge parameters 1, 1/2, 1/3, volume 1/6, and the mean of lambda_1 over its
   vertices is (1 + 0 + 1/2 + 2/3) / 4), from Bloechl's closed form evaluated on paper (E = 3/2) and from the mirror symmetry
   w_c(E) = 1/4 - w_{5-c}(3 - E) (E = 2).
2. `pdos_model.corner_weights`, PER CORNER, and `dos_model.simplex_fraction` against the reference: all 8 tetrahedron and all 4
   triangle tie patterns, every tie also widened to one ulp, E on every corner rank, strictly inside every interval, below and
   above; and corners whose gaps are subnormal or so small that products of three of them underflow.
3. `pdos_model.pnos` and `dos_model.nos` against the reference on the seeded tie-rich meshes of tests/test_gpu_dos_exact.py.

Bounds.  Per corner and filled fraction: 1e-14, the bound tests/test_pdos_model.py holds the sum rule to; a weight is a polynomial
of a dozen roundings in ratios in [0, 1].  Whole meshes: 1e-14 n_orb -- a bin averages the simplices of a band (the error of a
mean is at most that of its terms) and adds the n_orb bands.  Measured maxima: DESIGN.md 10.5.
"""

import itertools
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import pdos_model  # noqa: E402  pylint: disable=wrong-import-position
import tetra_exact as exact  # noqa: E402  pylint: disable=wrong-import-position

TOL = 1e-14
TINY = 5e-324  # the smallest positive double


# ---- 1. the reference against values worked by hand ----------------------------------------------------------------------------
def test_filled_fractions_worked_by_hand():
    assert exact.filled_fraction((0, 0, 0, 1), F(1, 2)) == F(7, 8)
    assert exact.filled_fraction((0, 1, 1, 1), F(1, 2)) == F(1, 8)
    assert exact.filled_fraction((0, 0, 1, 1), F(1, 2)) == F(1, 2)
    assert exact.filled_fraction((0, 0, 0, 0), 0) == 1 and exact.filled_fraction((0, 0, 0, 0), F(-1, 2)) == 0
    assert exact.filled_fraction((0, 1, 2), F(1, 2)) == F(1, 8) and exact.filled_fraction((0, 0, 1), F(1, 2)) == F(3, 4)


def test_corner_weights_worked_by_hand():
    assert exact.corner_weights((0, 1, 2, 3), 1) == (F(13, 144), F(1, 24), F(1, 48), F(1, 72))
    assert exact.corner_weights((0, 1, 2, 3), F(3, 2)) == (F(47, 256), F(39, 256), F(25, 256), F(17, 256))
    assert exact.corner_weights((0, 1, 2, 3), 2) == (F(17, 72), F(11, 48), F(5, 24), F(23, 144))
    assert exact.corner_weights((0, 1, 2), 1) == (F(1, 4), F(1, 6), F(1, 12))
    assert exact.corner_weights((0, 1, 2, 3), 3) == (F(1, 4),) * 4 and exact.corner_weights((0, 1, 2, 3), F(-1, 10)) == (0,) * 4
    # (0, 0, 1, 1) at 1/2, the wedge: s = lambda_3 + lambda_4 has the density 6 s (1 - s) on the simplex and lambda_1 the mean
    # (1 - s) / 2 given s, so w_1 = 3 int_0^1/2 s (1 - s)^2 ds = 11/64; likewise w_3 = 3 int_0^1/2 s^2 (1 - s) ds = 5/64
    assert exact.corner_weights((0, 0, 1, 1), F(1, 2)) == (F(11, 64), F(11, 64), F(5, 64), F(5, 64))
    assert exact.corner_weights((1, 0, 1, 0), F(1, 2)) == (F(5, 64), F(11, 64), F(5, 64), F(11, 64))
    assert sum(exact.corner_weights((0, 0, 1, 1), F(1, 2))) == F(1, 2)


def test_unit_weights_give_the_filled_fraction_and_the_corner_order_does_not_matter():
    corners = (F(-1, 2), F(1, 16), F(1, 16) + F(1, 2 ** 56), F(1, 2))
    a = (F(3, 7), F(1, 5), F(2, 3), F(1, 11))
    for energy in (F(-1, 2), F(0), F(1, 16), F(1, 16) + F(1, 2 ** 57), F(1, 16) + F(1, 2 ** 56), F(1, 4), F(1, 2)):
        w = exact.corner_weights(corners, energy)
        assert sum(x * 1 for x in w) == exact.filled_fraction(corners, energy)
        want = sum(x * y for x, y in zip(w, a))
        for perm in itertools.permutations(range(4)):  # all 24 orders: the same Fraction
            got = sum(x * a[c] for x, c in zip(exact.corner_weights(tuple(corners[c] for c in perm), energy), perm))
            assert got == want
    # the filled fraction of a tetrahedron without ties against the textbook cubic, exactly
    e1, e2, e3, e4 = (F(x) for x in (-0.7, -0.1, 0.35, 1.2))
    x = F(-0.3) - e1
    assert exact.filled_fraction((-0.7, -0.1, 0.35, 1.2), -0.3) == x ** 3 / ((e2 - e1) * (e3 - e1) * (e4 - e1))
    y = e4 - F(0.8)
    assert exact.filled_fraction((1.2, -0.1, -0.7, 0.35), 0.8) == 1 - y ** 3 / ((e4 - e1) * (e4 - e2) * (e4 - e3))


# ---- 2. the models against the reference, per corner -----------------------------------------------------------------------------
def _tied_corner_sets(n_c):
    """Ascending corners for every tie pattern from levels of magnitude 2^-4 ... 2^-1, of both signs, every subset of the ties
    widened to one ulp: [(pattern, corners)]."""
    out = []
    for levels in ([2.0 ** -4, 2.0 ** -3, 2.0 ** -2, 2.0 ** -1], [-2.0 ** -1, -2.0 ** -2, -2.0 ** -3, -2.0 ** -4],
                   [-2.0 ** -2, -2.0 ** -4, 2.0 ** -3, 2.0 ** -1]):
        for pattern in sorted(exact.all_tie_patterns(n_c)):
            ties = [i for i, tied in enumerate(pattern) if tied]
            for widened in itertools.chain.from_iterable(itertools.combinations(ties, k) for k in range(len(ties) + 1)):
                corners, level = [levels[0]], 0
                for i, tied in enumerate(pattern):
                    if not tied:
                        level += 1
                        corners.append(levels[level])
                    elif i in widened:
                        corners.append(np.nextafter(corners[-1], np.inf))
                    else:
                        corners.append(corners[-1])
                out.append((pattern, np.array(corners)))
    return out


def _small_gap_corner_sets(n_c):
    """Gaps whose reciprocal overflows (subnormal) and gaps whose products underflow, beside gaps of order one."""
    if n_c == 4:
        sets = [(-0.5, 0.0, TINY, 0.5), (-0.5, -TINY, 0.0, 0.5), (0.0, TINY, 0.25, 0.5), (-0.5, -0.25, 0.0, TINY), (0.0, TINY, 2 * TINY, 3 * TINY),
                (0.0, 1e-110, 2e-110, 3e-110), (0.0, 1e-160, 0.5, 0.5 + 1e-16), (-1e-200, 0.0, 1e-200, 1.0), (0.0, 0.0, TINY, 0.5),
                (0.0, TINY, TINY, 0.5), (1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51, 1.0 + 2.0 ** -50)]
    else:
        sets = [(-0.5, 0.0, TINY), (0.0, TINY, 0.5), (0.0, TINY, 2 * TINY), (0.0, 1e-160, 2e-160), (-0.5, -TINY, 0.0), (0.0, 0.0, TINY),
                (1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51)]
    return [np.array(s) for s in sets]


def _probe_energies(corners):
    """E on every corner, strictly inside every interval (where a double lies there: the midpoint and both neighbours of the
    ends), below and above."""
    points = [corners[0] - 0.25, corners[-1] + 0.25]
    for lo, hi in zip(corners[:-1], corners[1:]):
        if hi > lo:
            points += [lo + 0.5 * (hi - lo), lo + 0.3 * (hi - lo), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf)]
    inner = [p for p in points if not np.isin(p, corners)]
    return np.unique(np.concatenate([corners, inner])), len(inner) > 2


def _check_models_on(corners):
    """max|model - exact| over the probe energies: (per corner, filled fraction); the models must be finite."""
    n_c = len(corners)
    energies, _ = _probe_energies(corners)
    got_w = pdos_model.corner_weights(corners, energies)
    got_n = dos_model.simplex_fraction(corners, energies)
    assert np.isfinite(got_w).all() and np.isfinite(got_n).all(), corners
    worst_w = worst_n = 0.0
    for j, energy in enumerate(energies):
        want = exact.corner_weights(tuple(float(x) for x in corners), float(energy))
        worst_w = max(worst_w, max(abs(F(float(got_w[j, c])) - want[c]) for c in range(n_c)))
        worst_n = max(worst_n, abs(F(float(got_n[j])) - sum(want)))
    return float(worst_w), float(worst_n)


@pytest.mark.parametrize("n_c", [4, 3])
def test_models_match_the_reference_per_corner_under_every_tie(n_c):
    sets = _tied_corner_sets(n_c)
    assert {pattern for pattern, _ in sets} == exact.all_tie_patterns(n_c)
    # the unwidened sets show every pattern to the models as an exact tie; every rank is probed (the corners are probe energies)
    assert {exact.tie_pattern(c) for _, c in sets} == exact.all_tie_patterns(n_c)
    worst_w = worst_n = 0.0
    for _, corners in sets:
        w, n = _check_models_on(corners)
        worst_w, worst_n = max(worst_w, w), max(worst_n, n)
    print("%d corners, %d sets: max|w_c - exact| = %.3e, max|n_T - exact| = %.3e" % (n_c, len(sets), worst_w, worst_n))
    assert worst_w <= TOL and worst_n <= TOL


@pytest.mark.parametrize("n_c", [4, 3])
def test_models_match_the_reference_at_subnormal_and_underflowing_gaps(n_c):
    worst_w = worst_n = 0.0
    for corners in _small_gap_corner_sets(n_c):
        w, n = _check_models_on(corners)
        worst_w, worst_n = max(worst_w, w), max(worst_n, n)
    print("%d corners, small gaps: max|w_c - exact| = %.3e, max|n_T - exact| = %.3e" % (n_c, worst_w, worst_n))
    assert worst_w <= TOL and worst_n <= TOL


def test_subnormal_gap_with_the_grid_on_its_lower_corner():
    """(-0.5, 0, 5e-324, 0.5) at E = 0: the middle branch, x2 = 0 against a gap whose reciprocal is inf.  The tetrahedron is half
    full there (the plane eps = 0 through two corners, up to 5e-324)."""
    corners = np.array([-0.5, 0.0, TINY, 0.5])
    want = exact.corner_weights(tuple(corners), 0.0)
    assert abs(sum(want) - F(1, 2)) < F(1, 10 ** 300)
    got = pdos_model.corner_weights(corners, np.array([0.0]))[0]
    assert np.abs(got - np.array([float(x) for x in want])).max() <= TOL
    assert abs(dos_model.simplex_fraction(corners, np.array([0.0]))[0] - 0.5) <= TOL
    tri = np.array([-0.5, 0.0, TINY])
    want = exact.corner_weights(tuple(tri), 0.0)
    assert np.abs(pdos_model.corner_weights(tri, np.array([0.0]))[0] - np.array([float(x) for x in want])).max() <= TOL
    assert abs(dos_model.simplex_fraction(tri, np.array([0.0]))[0] - float(sum(want))) <= TOL


# ---- 3. whole meshes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh, n_orb", [((2, 2, 2), 3), ((2, 2, 2), 1), ((3, 2, 1), 3), ((3, 2), 3), ((3, 2), 1), ((1, 1, 1), 3)])
def test_models_match_the_reference_on_tie_rich_meshes(mesh, n_orb):
    eig, weights = exact.tie_rich_inputs(mesh, n_orb, 2)
    e_min, step, n_e = exact.ALIGNED_GRID
    for name, grid in (("aligned", e_min + np.arange(n_e) * step), ("unaligned", -0.7 + np.arange(13) * 0.11)):
        want = exact.pnos(eig, weights, grid)
        if name == "aligned":  # coverage is a condition of the test
            assert want.patterns_met == exact.possible_tie_patterns(mesh), (mesh, n_orb, want.patterns_met)
            assert all(want.rank_hit), want.rank_hit
        err_p = np.abs(pdos_model.pnos(eig, weights, grid) - want.nos).max()
        err_n = np.abs(dos_model.nos(eig, grid) - exact.nos(eig, grid).nos).max()
        print("%s x %d %s: max|pnos - exact| = %.3e, max|nos - exact| = %.3e" % (mesh, n_orb, name, err_p, err_n))
        assert err_p <= TOL * n_orb and err_n <= TOL * n_orb


def test_the_bins_argument_selects_columns():
    eig, weights = exact.tie_rich_inputs((3, 2), 3, 2)
    grid = -0.75 + np.arange(22) / 16.0
    whole, part = exact.pnos(eig, weights, grid), exact.pnos(eig, weights, grid, bins=[4, 13, 21])
    assert part.bins == [4, 13, 21] and np.array_equal(part.nos, whole.nos[:, [4, 13, 21]])
