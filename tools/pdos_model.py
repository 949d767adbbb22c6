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
    denominator is never divided by.  As in dos_model every branch is built from ratios in [0, 1] that are formed one by one, so
    a gap too small for its reciprocal (a subnormal one) never meets a zero: there is no 0 * inf and no 0 / 0 in a selected branch.
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
        a1, a2, a3, a4, x = e1[sel], e2[sel], e3[sel], e4[sel], en[sel] - e1[sel]
        q21, q31, q41 = x / (a2 - a1), x / (a3 - a1), x / (a4 - a1)
        c = 0.25 * q21 * q31 * q41
        out[sel] = np.stack([c * (4.0 - (q21 + q31 + q41)), c * q21, c * q31, c * q41], axis=-1)
        sel = (en >= e2) & (en < e3)
        a1, a2, a3, a4, en_s = e1[sel], e2[sel], e3[sel], e4[sel], en[sel]
        e31, e41, e32, e42 = a3 - a1, a4 - a1, a3 - a2, a4 - a2
        x1, x2, y3, y4 = en_s - a1, en_s - a2, a3 - en_s, a4 - en_s
        p31, p41, p32, p42 = x1 / e31, x1 / e41, x2 / e32, x2 / e42  # from below
        m31, m32, m41, m42 = y3 / e31, y3 / e32, y4 / e41, y4 / e42  # from above
        t = 0.25 * p41
        c1 = t * p31
        c2 = t * p32 * m31
        c3 = 0.25 * p42 * p32 * m41
        c12, c23 = c1 + c2, c2 + c3
        c123 = c12 + c3
        out[sel] = np.stack([
            c1 + c12 * m31 + c123 * m41,
            c123 + c23 * m32 + c3 * m42,
            c12 * p31 + c23 * p32,
            c123 * p41 + c3 * p42,
        ], axis=-1)
        sel = (en >= e3) & (en < e4)
        a1, a2, a3, a4, y = e1[sel], e2[sel], e3[sel], e4[sel], e4[sel] - en[sel]
        q41, q42, q43 = y / (a4 - a1), y / (a4 - a2), y / (a4 - a3)
        c = 0.25 * q41 * q42 * q43
        out[sel] = np.stack([0.25 - c * q41, 0.25 - c * q42, 0.25 - c * q43, 0.25 - c * (4.0 - (q41 + q42 + q43))], axis=-1)
    else:
        e1, e2, e3 = e
        third = 1.0 / 3.0
        sel = (en >= e1) & (en < e2)
        a1, a2, a3, x = e1[sel], e2[sel], e3[sel], en[sel] - e1[sel]
        q21, q31 = x / (a2 - a1), x / (a3 - a1)
        c = third * q21 * q31
        out[sel] = np.stack([c * (3.0 - (q21 + q31)), c * q21, c * q31], axis=-1)
        sel = (en >= e2) & (en < e3)
        a1, a2, a3, y = e1[sel], e2[sel], e3[sel], e3[sel] - en[sel]
        q31, q32 = y / (a3 - a1), y / (a3 - a2)
        c = third * q31 * q32
        out[sel] = np.stack([third - c * q31, third - c * q32, third - c * (3.0 - (q31 + q32))], axis=-1)
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
