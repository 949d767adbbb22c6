#!/usr/bin/env python3
"""
Exact statement of the band edges and the Fermi level of csrc/tbk_fermi.hip, in NumPy and rational arithmetic.

    eig            (n_1, ..., n_dim, n_orb), dim in {2, 3}: eig[..., b] = the b-th ascending eigenvalue at every mesh point
    band_edges     emin[b] = min over the mesh of eig[..., b], emax[b] = max: doubles of the array
    nos_exact(E)   N(E) = 1 / (S NK) sum over (cell, band, simplex) of n_T(E) as a Fraction, n_T from tetra_exact.filled_fraction
                   (simplices wholly below or above E are counted by comparisons of doubles, which are exact)
    fermi_level    n an integer m with emax[m - 1] < emin[m]: (midpoint, emax[m - 1], emin[m]); otherwise the smallest double mu
                   with N_exact(mu) >= n, found by bisection over the ordered doubles (N_exact is monotone, so the bisection finds
                   THE smallest one), returned as (mu, mu, mu)

The comparison N_exact(E) >= n is made in Fractions: n is the rational number the float holds.  It is design tooling: nothing in
the product imports it.  `python tools/fermi_model.py` prints the closed-form check of tests/test_fermi_model.py.
"""

import struct
from fractions import Fraction

import numpy as np

import dos_model
import tetra_exact


def band_edges(eig):
    """(emin, emax): two (n_orb,) arrays."""
    eig = np.asarray(eig, dtype=float)
    flat = eig.reshape(-1, eig.shape[-1])
    return flat.min(axis=0), flat.max(axis=0)


def sorted_simplices(eig):
    """Every simplex of the mesh with its corners ascending: (S NK n_orb, dim + 1)."""
    corners = dos_model.simplex_corners(np.asarray(eig, dtype=float))
    return np.sort(np.concatenate([c.reshape(-1, c.shape[-1]) for c in corners]), axis=-1)


def nos_exact(eig, energy, simplices=None):
    """N(energy) as a Fraction.  ``simplices``: `sorted_simplices(eig)` if the caller has it."""
    s = sorted_simplices(eig) if simplices is None else simplices
    energy = float(energy)
    full = int(np.count_nonzero(s[:, -1] <= energy))
    total = Fraction(full)
    cut = s[(s[:, 0] <= energy) & (s[:, -1] > energy)]
    if len(cut):
        rows, counts = np.unique(cut, axis=0, return_counts=True)
        for row, count in zip(rows, counts):
            total += int(count) * tetra_exact.filled_fraction(tuple(float(x) for x in row), energy)
    return total / len(s) * np.asarray(eig).shape[-1]


def key(x):
    """The ordered-integer image of a double: x < y  <=>  key(x) < key(y); -0.0 sits in front of +0.0."""
    (bits,) = struct.unpack("<Q", struct.pack("<d", x))
    return (~bits) & (2 ** 64 - 1) if bits >> 63 else bits | (1 << 63)


def unkey(k):
    bits = k & ~(1 << 63) if k >> 63 else (~k) & (2 ** 64 - 1)
    (x,) = struct.unpack("<d", struct.pack("<Q", bits))
    return x


def fermi_level(eig, n_electrons):
    """(mu, lower, upper) for 0 < n_electrons < n_orb; lower < upper exactly in the gap case."""
    eig = np.asarray(eig, dtype=float)
    n_orb = eig.shape[-1]
    n = float(n_electrons)
    if not 0.0 < n < n_orb:
        raise ValueError("n_electrons must lie inside (0, n_orb)")
    emin, emax = band_edges(eig)
    if n == int(n):
        m = int(n)
        if emax[m - 1] < emin[m]:
            lower, upper = float(emax[m - 1]), float(emin[m])
            return lower + (upper - lower) / 2, lower, upper
    target = Fraction(n)
    simplices = sorted_simplices(eig)
    lo, hi = key(np.nextafter(emin[0], -np.inf)), key(float(emax[-1]))  # N(lo) = 0 < n <= N(hi) = n_orb
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if nos_exact(eig, unkey(mid), simplices) >= target:
            hi = mid
        else:
            lo = mid
    mu = unkey(hi)
    mu = 0.0 if mu == 0.0 else mu  # -0.0 and +0.0 are one energy
    return mu, mu, mu


def main():
    # one band, E = i + j on a 4 x 4 mesh (periodic): the closed form of tests/test_fermi_model.py
    i, j = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    eig = (i + j).astype(float)[..., None]
    print("E     N_exact")
    for energy in (0.0, 0.5, 1.0, 2.5, 3.0, 6.0):
        print("%4.1f  %s" % (energy, nos_exact(eig, energy)))
    for n in (0.25, 0.5, 0.75):
        print("n = %.2f  mu = %.17g" % (n, fermi_level(eig, n)[0]))


if __name__ == "__main__":
    main()
