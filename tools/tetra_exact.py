#!/usr/bin/env python3
"""
Exact reference of the (projected) number of states of tools/dos_model.py and tools/pdos_model.py, in rational arithmetic.

    nos[g][j] = 1 / (S NK) * sum over (cell, band, simplex T) of  int_T theta(E_j - eps(k)) A_g(k) dk / |T|

for the doubles it is given: every input is converted with Fraction(float), which is exact, every operation is exact, and the
result is rounded to double once, at the end.  It shares the simplex list with the models (`dos_model.simplex_corners`: the mesh
topology) and nothing else: it does not use Bloechl's closed forms, it does not sort the corners and it has no branch per energy
range.  The region eps <= E of a simplex is integrated geometrically (`corner_weights`):

    corners with e_c <= E are "below"
    none below            0;  all below: 1 / n per corner
    one below             the small simplex cut off at that corner: its vertices are the corner b and the points at parameter
                          t_d = (E - e_b) / (e_d - e_b) on the edges to the others, its volume is the product of the t_d
    one above             the whole simplex minus the small simplex at that corner, t_d = (e_a - E) / (e_a - e_d)
    two below, two above  (tetrahedron) a wedge between the triangles (b1, p11, p12) and (b2, p21, p22), p_ij on the edge from
                          below corner i to above corner j: three tetrahedra whose volumes are determinants of barycentric coordinates
    the integral of a linear function over a simplex = its volume times the mean of the function's values at its vertices

A cut edge always joins a corner with e <= E to one with e > E, so no denominator is zero under any tie of the corners.

Besides the values it keeps the books the tests assert their coverage from: which tie patterns of the sorted corners occurred, which
of them met an evaluated grid point inside their range, and for every corner rank whether an evaluated grid point equalled a corner
of that rank exactly.  It is design tooling: nothing in the product imports it.
"""

import functools
import itertools
from fractions import Fraction

import numpy as np

import dos_model


def _det(rows):
    """Determinant of a small square matrix of Fractions (Laplace expansion along the first row)."""
    n = len(rows)
    if n == 1:
        return rows[0][0]
    total = Fraction(0)
    for col, value in enumerate(rows[0]):
        if value != 0:
            minor = [row[:col] + row[col + 1:] for row in rows[1:]]
            total += (-1 if col % 2 else 1) * value * _det(minor)
    return total


def _piece(vertices, volume=None):
    """int lambda_c over the simplex whose vertices are given in barycentric coordinates of T, in units of |T|: one Fraction per
    corner.  ``volume`` (in units of |T|) if it is known, else |det| of the coordinates."""
    n = len(vertices)
    if volume is None:
        volume = abs(_det([list(v) for v in vertices]))
    return [volume * sum(v[c] for v in vertices) / n for c in range(n)]


def _unit(n, c):
    return tuple(Fraction(int(i == c)) for i in range(n))


def _cut(n, e, lo, hi, energy):
    """The point eps = energy on the edge from corner lo (e <= energy) to corner hi (e > energy), and its parameter from lo."""
    t = (energy - e[lo]) / (e[hi] - e[lo])
    point = [Fraction(0)] * n
    point[lo], point[hi] = 1 - t, t
    return tuple(point), t


@functools.lru_cache(maxsize=None)
def _weights(e, energy):
    n = len(e)
    below = [c for c in range(n) if e[c] <= energy]
    above = [c for c in range(n) if e[c] > energy]
    if not below:
        return (Fraction(0),) * n
    if not above:
        return (Fraction(1, n),) * n
    if len(below) == 1:
        b = below[0]
        cuts = [_cut(n, e, b, a, energy) for a in above]
        volume = Fraction(1)
        for _, t in cuts:
            volume *= t
        return tuple(_piece([_unit(n, b)] + [p for p, _ in cuts], volume))
    if len(above) == 1:
        a = above[0]
        cuts = [_cut(n, e, b, a, energy) for b in below]
        volume = Fraction(1)
        for _, t in cuts:
            volume *= 1 - t  # the parameter from the corner above
        empty = _piece([_unit(n, a)] + [p for p, _ in cuts], volume)
        return tuple(Fraction(1, n) - x for x in empty)
    # the wedge of a tetrahedron
    (b1, b2), (a1, a2) = below, above
    first = [_unit(n, b1), _cut(n, e, b1, a1, energy)[0], _cut(n, e, b1, a2, energy)[0]]
    second = [_unit(n, b2), _cut(n, e, b2, a1, energy)[0], _cut(n, e, b2, a2, energy)[0]]
    total = [Fraction(0)] * n
    for i in range(3):  # the staircase triangulation of a prism
        for c, x in enumerate(_piece(first[i:] + second[:i + 1])):
            total[c] += x
    return tuple(total)


def corner_weights(corners, energy):
    """The exact w_c(E) = int_T theta(E - eps) lambda_c / |T| for the corner energies ``corners`` (3 or 4 numbers, ANY order;
    floats or Fractions): a tuple of Fractions in the order of ``corners``."""
    e = tuple(Fraction(x) for x in corners)
    if len(e) not in (3, 4):
        raise ValueError("a simplex has 3 or 4 corners")
    return _weights(e, Fraction(energy))


def filled_fraction(corners, energy):
    """The exact filled fraction n_T(E): the sum of the corner weights."""
    return sum(corner_weights(corners, energy))


def tie_pattern(corners):
    """Which neighbours among the SORTED corners are equal: (e1 == e2, e2 == e3[, e3 == e4])."""
    s = sorted(corners)
    return tuple(s[i] == s[i + 1] for i in range(len(s) - 1))


def all_tie_patterns(n_corners):
    return set(itertools.product((False, True), repeat=n_corners - 1))


class Exact:
    """nos: (G, len(bins)) doubles.  bins: the evaluated bin indices.  patterns, patterns_met, rank_hit: the books of `coverage`."""

    def __init__(self, nos, bins, patterns, patterns_met, rank_hit):
        self.nos, self.bins, self.patterns, self.patterns_met, self.rank_hit = nos, bins, patterns, patterns_met, rank_hit


def coverage(eig, energies):
    """
    The books of a mesh and the grid points ``energies`` (comparisons of doubles are exact):
    patterns      the tie patterns of the sorted corners that occur among the simplices;
    patterns_met  those for which some simplex has a grid point inside its range e1 <= E < e_top (all corners equal: a grid
                  point ON the step, E == e1);
    rank_hit[r]   some grid point equals the corner of rank r + 1 of some simplex exactly.
    """
    eig = np.asarray(eig, dtype=float)
    energies = np.asarray(energies, dtype=float)
    corners = np.concatenate([c.reshape(-1, c.shape[-1]) for c in dos_model.simplex_corners(eig)])
    corners = np.unique(np.sort(corners, axis=-1), axis=0)
    patterns, met = set(), set()
    rank_hit = [bool(np.isin(corners[:, r], energies).any()) for r in range(corners.shape[-1])]
    for s in corners:
        pattern = tuple(bool(x) for x in s[:-1] == s[1:])
        patterns.add(pattern)
        inside = (energies >= s[0]) & ((energies < s[-1]) | (s[0] == s[-1]) & (energies == s[0]))
        if inside.any():
            met.add(pattern)
    return patterns, met, rank_hit


def possible_tie_patterns(mesh):
    """The tie patterns a mesh can show at all.  One point: every corner is that point.  An axis of a single point: the step
    along it returns to the same point, so two corners of every simplex are equal and the pattern without a tie cannot occur."""
    n_c = len(mesh) + 1
    if all(n == 1 for n in mesh):
        return {(True,) * (n_c - 1)}
    every = all_tie_patterns(n_c)
    if any(n == 1 for n in mesh):
        every.discard((False,) * (n_c - 1))
    return every


LEVELS = (-0.5, -0.25, 0.0625, 0.125, 0.5)  # dyadic: every level sits on the grid -0.75 + j / 16


ALIGNED_GRID = (-0.75, 2.0 ** -4, 22)  # e_min, step, n_e: every E_j is exact, the levels are bins 4, 8, 13, 14 and 20
# seeds (searched once, on the CPU) with which the aligned grid meets every tie pattern the mesh can show and hits a corner of
# every rank, for every number of bands used: {(mesh, n_orb): seed}
TIE_RICH_SEEDS = {
    ((2, 2, 2), 1): 319, ((2, 2, 2), 3): 1, ((2, 2, 2), 4): 1,
    ((3, 2, 1), 1): 6, ((3, 2, 1), 3): 2, ((3, 2, 1), 4): 1,
    ((3, 3, 2), 1): 9, ((3, 3, 2), 3): 1, ((3, 3, 2), 4): 1,
    ((3, 2), 1): 6, ((3, 2), 3): 2, ((3, 2), 4): 1,
}


def tie_rich_inputs(mesh, n_orb, n_groups, seed=None):
    """Seeded inputs in which corners tie: eigenvalues drawn from LEVELS, about 30 % of them moved up by one ulp (a tie widened
    to the smallest gap there is), every row ascending; weights uniform in [0, 1].  (mesh + (n_orb,), mesh + (n_groups, n_orb))"""
    if seed is None:
        seed = TIE_RICH_SEEDS.get((tuple(mesh), n_orb), 1)
    rng = np.random.default_rng(seed)
    shape = tuple(mesh) + (n_orb,)
    eig = rng.choice(np.array(LEVELS), size=shape)
    eig = np.where(rng.random(shape) < 0.3, np.nextafter(eig, np.inf), eig)
    eig = np.sort(eig, axis=-1)
    weights = rng.uniform(0.0, 1.0, tuple(mesh) + (n_groups, n_orb))
    return eig, weights


def pnos(eig, weights, grid, bins=None):
    """The exact nos[g][j] of `pdos_model.pnos(eig, weights, grid)` for j in ``bins`` (default: every bin), with the books."""
    eig = np.asarray(eig, dtype=float)
    weights = np.asarray(weights, dtype=float)
    grid = np.asarray(grid, dtype=float)
    mesh, n_orb = eig.shape[:-1], eig.shape[-1]
    if weights.ndim != eig.ndim + 1 or weights.shape[:-2] != mesh or weights.shape[-1] != n_orb:
        raise ValueError("weights must have shape mesh + (G, n_orb)")
    n_groups = weights.shape[-2]
    n_k = int(np.prod(mesh))
    bins = list(range(len(grid))) if bins is None else [int(j) for j in bins]
    energies = [Fraction(float(grid[j])) for j in bins]
    corners_e = dos_model.simplex_corners(eig)
    corners_a = dos_model.simplex_corners(weights.reshape(mesh + (n_groups * n_orb,)))
    n_c = corners_e[0].shape[-1]
    # A is dyadic: integers over one power of two, so that the sums over simplices with the same weights are integer sums
    scale = max(Fraction(float(x)).denominator for x in np.unique(weights))
    # simplices with the same corner energies (in corner order) share their weights at every bin: add up their A first
    pooled = {}
    for c_e, c_a in zip(corners_e, corners_a):
        flat_e = c_e.reshape(n_k * n_orb, n_c)
        flat_a = np.moveaxis(c_a.reshape(n_k, n_groups, n_orb, n_c), 1, 2).reshape(n_k * n_orb, n_groups, n_c)
        for e_row, a_row in zip(flat_e, flat_a):
            key = tuple(float(x) for x in e_row)
            ints = [[int(Fraction(float(x)) * scale) for x in a_g] for a_g in a_row]
            if key in pooled:
                pooled[key] = [[p + q for p, q in zip(pg, ig)] for pg, ig in zip(pooled[key], ints)]
            else:
                pooled[key] = ints
    total = [[Fraction(0)] * len(bins) for _ in range(n_groups)]
    for key, a_sum in pooled.items():
        e = tuple(Fraction(x) for x in key)
        for j, energy in enumerate(energies):
            w = _weights(e, energy)
            if any(w):
                for g in range(n_groups):
                    total[g][j] += sum(w_c * a for w_c, a in zip(w, a_sum[g]))
    denom = scale * len(corners_e) * n_k
    values = np.array([[float(x / denom) for x in row] for row in total]).reshape(n_groups, len(bins))
    patterns, met, rank_hit = coverage(eig, grid[bins])
    return Exact(values, bins, patterns, met, rank_hit)


def nos(eig, grid, bins=None):
    """The exact nos[j] of `dos_model.nos(eig, grid)`: `pnos` with unit weights; ``.nos`` has shape (len(bins),)."""
    eig = np.asarray(eig, dtype=float)
    result = pnos(eig, np.ones(eig.shape[:-1] + (1, eig.shape[-1])), grid, bins)
    result.nos = result.nos[0]
    return result


def main():
    print("tetrahedron (0, 1, 2, 3): the exact corner weights")
    for energy in (Fraction(1, 2), 1, Fraction(3, 2), 2, Fraction(5, 2)):
        w = corner_weights((0, 1, 2, 3), energy)
        print("E = %-4s w = %-40s n_T = %s" % (energy, ", ".join(str(x) for x in w), sum(w)))


if __name__ == "__main__":
    main()
