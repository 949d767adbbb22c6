#!/usr/bin/env python3
"""
NumPy model of the density-of-states kernel of csrc/tbk_dos.hip: the number of states nos(E) of a uniform, periodic k mesh by
the linear tetrahedron method (triangles in two dimensions).

    mesh (n_1, ..., n_dim), dim in {2, 3}; E has shape (n_1, ..., n_dim, n_orb), E[..., b] = the b-th ascending eigenvalue
    dim = 3   every cell is cut into the 6 tetrahedra that share its main diagonal: for every order (a, b, c) of the axes the
              corners 0, e_a, e_a + e_b, e_a + e_b + e_c; weight 1 / (6 NK) each
    dim = 2   2 triangles per cell: for both orders (a, b) the corners 0, e_a, e_a + e_b; weight 1 / (2 NK) each
    nos[j]    = sum over (cell, band, simplex) of weight * n_T(E_j), n_T = the filled fraction of the simplex for the band
              interpolated linearly between its corners (`simplex_fraction`)

The neighbours of a cell are taken with np.roll: the mesh is periodic.  This file is the executable statement of DESIGN.md
section 10.1; the GPU tests compare the kernel with it on identical inputs.  `python tools/dos_model.py` prints the free-electron
like check of tests/test_dos_model.py.  It is design tooling: nothing in the product imports it.
"""

import itertools

import numpy as np


def simplex_fraction(corners, energies):
    """
    Filled fraction n_T(E) of simplices whose corner energies are ``corners[..., :]`` (3 corners: triangle, 4: tetrahedron) for
    every E of the 1-D array ``energies``: shape ``corners.shape[:-1] + (len(energies),)``.  The ranges are half-open as in
    DESIGN 10.1, the comparisons select the branch, and a branch is evaluated only where it was selected (so a zero denominator
    is never divided by; a fully degenerate simplex is a clean step at its energy).  Every branch is a polynomial in ratios
    (E - e_i) / (e_j - e_i) or (e_j - E) / (e_j - e_i) that lie in [0, 1] and are formed one by one: no product of differences can
    underflow to 0 against an overflowing product of reciprocals, however small a gap is.
    """
    corners = np.sort(np.asarray(corners, dtype=float), axis=-1)
    energies = np.asarray(energies, dtype=float)
    n_c = corners.shape[-1]
    if n_c not in (3, 4):
        raise ValueError("a simplex has 3 or 4 corners")
    lead = corners.shape[:-1]
    shape = lead + energies.shape
    en = np.broadcast_to(energies, shape)
    e = [np.broadcast_to(corners[..., i, None], shape) for i in range(n_c)]
    out = np.zeros(shape)
    out[en >= e[-1]] = 1.0
    if n_c == 4:
        e1, e2, e3, e4 = e
        sel = (en >= e1) & (en < e2)
        a1, a2, a3, a4, x = e1[sel], e2[sel], e3[sel], e4[sel], en[sel] - e1[sel]
        out[sel] = (x / (a2 - a1)) * (x / (a3 - a1)) * (x / (a4 - a1))
        sel = (en >= e2) & (en < e3)
        a1, a2, a3, a4, x = e1[sel], e2[sel], e3[sel], e4[sel], en[sel]
        x1, x2, y3, y4 = x - a1, x - a2, a3 - x, a4 - x
        q41, q32 = x1 / (a4 - a1), x2 / (a3 - a2)
        out[sel] = q41 * (x1 / (a3 - a1) + q32 * (y3 / (a3 - a1))) + (x2 / (a4 - a2)) * q32 * (y4 / (a4 - a1))
        sel = (en >= e3) & (en < e4)
        a1, a2, a3, a4, y = e1[sel], e2[sel], e3[sel], e4[sel], e4[sel] - en[sel]
        out[sel] = 1.0 - (y / (a4 - a1)) * (y / (a4 - a2)) * (y / (a4 - a3))
    else:
        e1, e2, e3 = e
        sel = (en >= e1) & (en < e2)
        a1, a2, a3, x = e1[sel], e2[sel], e3[sel], en[sel] - e1[sel]
        out[sel] = (x / (a2 - a1)) * (x / (a3 - a1))
        sel = (en >= e2) & (en < e3)
        a1, a2, a3, y = e1[sel], e2[sel], e3[sel], e3[sel] - en[sel]
        out[sel] = 1.0 - (y / (a3 - a1)) * (y / (a3 - a2))
    return out


def simplex_corners(eig):
    """
    The corner energies of every simplex of the mesh: a list of S = dim! arrays of shape ``eig.shape + (dim + 1,)``, one per
    order of the axes.  ``eig``: (n_1, ..., n_dim, n_orb).
    """
    eig = np.asarray(eig, dtype=float)
    dim = eig.ndim - 1
    if dim not in (2, 3):
        raise ValueError("the mesh must have 2 or 3 dimensions")
    simplices = []
    for order in itertools.permutations(range(dim)):
        corners, shifted = [eig], eig
        for axis in order:
            shifted = np.roll(shifted, -1, axis=axis)  # the neighbour at +1 along `axis`, periodic
            corners.append(shifted)
        simplices.append(np.stack(corners, axis=-1))
    return simplices


def nos(eig, energies, chunk=64):
    """nos[j] for ``eig`` of shape (n_1, ..., n_dim, n_orb) and the 1-D array ``energies`` (any ascending grid)."""
    eig = np.asarray(eig, dtype=float)
    energies = np.asarray(energies, dtype=float)
    simplices = simplex_corners(eig)
    n_k = int(np.prod(eig.shape[:-1]))
    total = np.zeros(len(energies))
    for corners in simplices:  # the loop over the simplices of a cell
        flat = corners.reshape(-1, corners.shape[-1])
        for j0 in range(0, len(energies), chunk):
            total[j0:j0 + chunk] += simplex_fraction(flat, energies[j0:j0 + chunk]).sum(axis=0)
    return total / (len(simplices) * n_k)


def dos(eig, energies):
    """The difference quotient of ``nos`` on a uniform grid: values at the bin midpoints."""
    energies = np.asarray(energies, dtype=float)
    return np.diff(nos(eig, energies)) / np.diff(energies)


def mesh_kpoints(mesh):
    """The k list of a mesh, (NK, dim) in np.meshgrid(..., indexing="ij") order: k_d = i_d / n_d."""
    axes = [np.arange(n) / n for n in mesh]
    return np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], axis=1)


def main():
    # one cosine band on a cubic mesh: nos(E) + nos(-E) = 1 on an even mesh, nos runs from 0 to 1
    n = 12
    k = mesh_kpoints((n, n, n))
    eig = (2.0 * np.cos(2 * np.pi * k).sum(axis=1)).reshape(n, n, n, 1)
    grid = np.linspace(-6.5, 6.5, 14)
    states = nos(eig, grid)
    print("E      nos      nos(E) + nos(-E)")
    for e, s, t in zip(grid, states, states[::-1]):
        print("%6.2f  %.6f  %.15f" % (e, s, s + t))


if __name__ == "__main__":
    main()
