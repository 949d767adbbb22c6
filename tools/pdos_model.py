#!/usr/bin/env python3
"""
NumPy model of the projected density-of-states kernels of csrc/tbk_pdos.hip: the number of states nos_g(E) of a uniform, periodic
k mesh by the linear tetrahedron method (triangles in two dimensions), every state (k, b) weighted by A_g(k, b) in [0, 1].

    eig      (n_1, ..., n_dim, n_orb)       E[..., b] = the b-th ascending eigenvalue
    weights  (n_1, ..., n_dim, G, n_orb)    A_g(k, b), e.g. `band_weights(U, groups)` = sum_{i in g} |U[k][i][b]|^2
    nos[g][j] = 1 / (S NK) * sum over (cell, band, simplex T) of  int_T theta(E_j - eps(k)) A_g(k) dk / |T|,
                eps and A_g interpolated linearly between the corners of T  =  sum_c w_c(E_j) A_g,c   (`corner_weights`)

The simplices are those of tools/dos_model.py (`simplex_corners`: the 6 tetrahedra that share the main diagonal of a cell, the 2
triangles in two dimensions), the corners of a simplex are sorted by energy with a STABLE sort (ties keep corner order) and each
corner's weights travel with its energy.  With A = 1 the sum of the corner weights is the filled fraction n_T of dos_model, so
`pnos` is `dos_model.nos`.  This file is the executable statement of DESIGN.md section 11; the GPU tests compare the kernels with
it on identical inputs.  It is design tooling: nothing in the product imports it.
"""

import numpy as np

import dos_model


def corner_weights(e_sorted, energies):
    """
    Bloechl's corner weights w_c(E) of simplices whose ASCENDING corner energies are ``e_sorted[..., :]`` (3 corners: triangle,
    4: tetrahedron) for every E of the 1-D array ``energies``: shape ``e_sorted.shape[:-1] + (len(energies), n_corners)``.
    w_c(E) = int_T theta(E - eps) lambda_c / |T| for the linear interpolant eps = sum_c lambda_c e_c; sum_c w_c = n_T(E).  The
    ranges are half-open, the comparisons select the branch and a branch is evaluated only where it was selected, so a zero
    denominator is never divided by.
    """
    corners = np.asarray(e_sorted, dtype=float)
    energies = np.asarray(energies, dtype=float)
    n_c = corners.shape[-1]
    if n_c not in (3, 4):
        raise ValueError("a simplex has 3 or 4 corners")
    if np.any(np.diff(corners, axis=-1) < 0):
        raise ValueError("the corner energies must be ascending")
    shape = corners.shape[:-1] + energies.shape
    en = np.broadcast_to(energies, shape)
    e = [np.broadcast_to(corners[..., i, None], shape) for i in range(n_c)]
    out = np.zeros(shape + (n_c,))
    out[en >= e[-1]] = 1.0 / n_c
    if n_c == 4:
        e1, e2, e3, e4 = e
        sel = (en >= e1) & (en < e2)
        a1, a2, a3, a4, en_s = e1[sel], e2[sel], e3[sel], e4[sel], en[sel]
        e21, e31, e41 = a2 - a1, a3 - a1, a4 - a1
        x = en_s - a1
        c = x ** 3 / (4.0 * e21 * e31 * e41)
        out[sel] = np.stack([c * (4.0 - x * (1.0 / e21 + 1.0 / e31 + 1.0 / e41)), c * x / e21, c * x / e31, c * x / e41], axis=-1)
        sel = (en >= e2) & (en < e3)
        a1, a2, a3, a4, en_s = e1[sel], e2[sel], e3[sel], e4[sel], en[sel]
        e31, e41, e32, e42 = a3 - a1, a4 - a1, a3 - a2, a4 - a2
        x1, x2, y3, y4 = en_s - a1, en_s - a2, a3 - en_s, a4 - en_s
        c1 = x1 * x1 / (4.0 * e41 * e31)
        c2 = x1 * x2 * y3 / (4.0 * e41 * e32 * e31)
        c3 = x2 * x2 * y4 / (4.0 * e42 * e32 * e41)
        out[sel] = np.stack([
            c1 + (c1 + c2) * y3 / e31 + (c1 + c2 + c3) * y4 / e41,
            c1 + c2 + c3 + (c2 + c3) * y3 / e32 + c3 * y4 / e42,
            (c1 + c2) * x1 / e31 + (c2 + c3) * x2 / e32,
            (c1 + c2 + c3) * x1 / e41 + c3 * x2 / e42,
        ], axis=-1)
        sel = (en >= e3) & (en < e4)
        a1, a2, a3, a4, en_s = e1[sel], e2[sel], e3[sel], e4[sel], en[sel]
        e41, e42, e43 = a4 - a1, a4 - a2, a4 - a3
        y = a4 - en_s
        c = y ** 3 / (4.0 * e41 * e42 * e43)
        out[sel] = np.stack([0.25 - c * y / e41, 0.25 - c * y / e42, 0.25 - c * y / e43,
                             0.25 - c * (4.0 - y * (1.0 / e41 + 1.0 / e42 + 1.0 / e43))], axis=-1)
    else:
        e1, e2, e3 = e
        third = 1.0 / 3.0
        sel = (en >= e1) & (en < e2)
        a1, a2, a3, en_s = e1[sel], e2[sel], e3[sel], en[sel]
        e21, e31 = a2 - a1, a3 - a1
        x = en_s - a1
        c = x * x / (3.0 * e21 * e31)
        out[sel] = np.stack([c * (3.0 - x * (1.0 / e21 + 1.0 / e31)), c * x / e21, c * x / e31], axis=-1)
        sel = (en >= e2) & (en < e3)
        a1, a2, a3, en_s = e1[sel], e2[sel], e3[sel], en[sel]
        e31, e32 = a3 - a1, a3 - a2
        y = a3 - en_s
        c = y * y / (3.0 * e31 * e32)
        out[sel] = np.stack([third - c * y / e31, third - c * y / e32, third - c * (3.0 - y * (1.0 / e31 + 1.0 / e32))], axis=-1)
    return out


def pnos(eig, weights, grid, chunk=64):
    """nos[g][j] for ``eig`` (n_1, ..., n_dim, n_orb), ``weights`` (n_1, ..., n_dim, G, n_orb) and the 1-D ascending ``grid``."""
    eig = np.asarray(eig, dtype=float)
    weights = np.asarray(weights, dtype=float)
    grid = np.asarray(grid, dtype=float)
    mesh, n_orb = eig.shape[:-1], eig.shape[-1]
    if weights.ndim != eig.ndim + 1 or weights.shape[:-2] != mesh or weights.shape[-1] != n_orb:
        raise ValueError("weights must have shape mesh + (G, n_orb)")
    n_groups = weights.shape[-2]
    n_k = int(np.prod(mesh))
    corners_e = dos_model.simplex_corners(eig)  # S arrays mesh + (n_orb, dim + 1)
    corners_a = dos_model.simplex_corners(weights.reshape(mesh + (n_groups * n_orb,)))  # the same list on the weights
    total = np.zeros((n_groups, len(grid)))
    for c_e, c_a in zip(corners_e, corners_a):
        n_c = c_e.shape[-1]
        flat_e = c_e.reshape(n_k * n_orb, n_c)
        flat_a = np.moveaxis(c_a.reshape(n_k, n_groups, n_orb, n_c), 1, 2).reshape(n_k * n_orb, n_groups, n_c)
        order = np.argsort(flat_e, axis=-1, kind="stable")  # ties keep corner order; the weights travel with the energies
        flat_e = np.take_along_axis(flat_e, order, axis=-1)
        flat_a = np.take_along_axis(flat_a, order[:, None, :], axis=-1)
        for j0 in range(0, len(grid), chunk):
            w = corner_weights(flat_e, grid[j0:j0 + chunk])  # (items, bins, corners)
            total[:, j0:j0 + chunk] += np.einsum("mjc,mgc->gj", w, flat_a)
    return total / (len(corners_e) * n_k)


def band_weights(U, groups):
    """A[..., g, b] = sum_{i in groups[g]} |U[..., i, b]|^2 for eigenvectors in the columns of ``U`` (..., n_orb, n_orb)."""
    prob = np.abs(np.asarray(U)) ** 2
    return np.stack([prob[..., list(group), :].sum(axis=-2) for group in groups], axis=-2)


def main():
    # two cosine bands that trade their orbital character across the zone: the projections add up to the total
    n = 10
    k = dos_model.mesh_kpoints((n, n, n))
    band = 2.0 * np.cos(2 * np.pi * k).sum(axis=1)
    eig = np.stack([band - 7.0, band + 7.0], axis=1).reshape(n, n, n, 2)
    mix = (0.5 + 0.5 * np.cos(2 * np.pi * k[:, 0])).reshape(n, n, n)
    weights = np.stack([np.stack([mix, 1.0 - mix], axis=-1), np.stack([1.0 - mix, mix], axis=-1)], axis=-2)
    grid = np.linspace(-13.5, 13.5, 10)
    states = pnos(eig, weights, grid)
    print("E       nos_0     nos_1     sum       dos_model.nos")
    for e, a, b, t in zip(grid, states[0], states[1], dos_model.nos(eig, grid)):
        print("%6.2f  %.6f  %.6f  %.6f  %.6f" % (e, a, b, a + b, t))


if __name__ == "__main__":
    main()
