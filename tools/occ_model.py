#!/usr/bin/env python3
"""
NumPy and exact-rational model of csrc/tbk_occ.hip: the tetrahedron integration weight of every state of a uniform, periodic k mesh
at one energy, and the band occupations, band energies and orbital occupations made from it.

    w[k][b] = 1 / (S NK) * sum over the simplices T that contain mesh point k of Bloechl's corner weight of k in T

Mesh point v is corner p of the simplex with axis order sigma of the cell at v - (e_sigma1 + ... + e_sigmap): 24 tetrahedra over 15
mesh points in three dimensions, 6 triangles over 7 in two.  `gather_table` lists them in the kernel's summation order
(s = (dim + 1) sigma + p, sigma in itertools.permutations order); `point_weights` is the kernel's arithmetic in NumPy by that
gather, `point_weights_scatter` the same quantity scattered from the simplices of `dos_model.simplex_corners`, and
`point_weights_exact` the exact rational value (corner weights of tools/tetra_exact.py), rounded once.  The triangle weights are
carried times three and the divisor is 3 S NK, as in the kernel: a full corner is then exactly 1.

`python tools/occ_model.py` prints a small worked case.  Design tooling: nothing in the product imports it.
"""

import itertools
from fractions import Fraction

import numpy as np

import dos_model
import tetra_exact

GAP_SCALE = 2.0 ** 54  # DOS_GAP_SCALE of csrc/tbk_tetra.h


def gather_table(dim):
    """[(sigma, p, offsets)] in the kernel's order: the simplex with axis order ``sigma`` in which the point is corner ``p``;
    ``offsets`` are its dim + 1 corners relative to the point, in simplex order (offsets[p] is the zero vector)."""
    if dim not in (2, 3):
        raise ValueError("the mesh must have 2 or 3 dimensions")
    table = []
    for sigma in itertools.permutations(range(dim)):
        steps = [np.zeros(dim, dtype=int)]
        for axis in sigma:
            step = steps[-1].copy()
            step[axis] += 1
            steps.append(step)
        for p in range(dim + 1):
            table.append((sigma, p, tuple(tuple(int(x) for x in step - steps[p]) for step in steps)))
    return table


def _stable_sort(corners):
    """Ascending along the last axis, ties in corner order; returns (sorted, order) with order[..., r] = the corner of rank r."""
    order = np.argsort(corners, axis=-1, kind="stable")
    return np.take_along_axis(corners, order, axis=-1), order


def corner_weights(e_sorted, energy):
    """The kernel's corner weights of simplices whose SORTED corner energies are ``e_sorted[..., :]`` at one energy: shape of
    ``e_sorted``; tetrahedra in units of 1 (a full corner is 1/4), triangles TIMES THREE (a full corner is 1)."""
    e = np.asarray(e_sorted, dtype=float)
    n_c = e.shape[-1]
    mu = float(energy)
    out = np.zeros(e.shape)
    full = 0.25 if n_c == 4 else 1.0
    out[mu >= e[..., -1]] = full
    s = e * GAP_SCALE
    es = mu * GAP_SCALE
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if n_c == 4:
            s1, s2, s3, s4 = (s[..., i] for i in range(4))
            r21, r31, r41, r32, r42, r43 = 1.0 / (s2 - s1), 1.0 / (s3 - s1), 1.0 / (s4 - s1), 1.0 / (s3 - s2), 1.0 / (s4 - s2), 1.0 / (s4 - s3)
            sel = (mu >= e[..., 0]) & (mu < e[..., 1])
            x = es - s1
            q21, q31, q41 = x * r21, x * r31, x * r41
            c = 0.25 * q21 * q31 * q41
            first = np.stack([c * (4.0 - (q21 + q31 + q41)), c * q21, c * q31, c * q41], axis=-1)
            out[sel] = first[sel]
            sel = (mu >= e[..., 1]) & (mu < e[..., 2])
            x1, x2, y3, y4 = es - s1, es - s2, s3 - es, s4 - es
            p31, p41, p32, p42 = x1 * r31, x1 * r41, x2 * r32, x2 * r42
            m31, m32, m41, m42 = y3 * r31, y3 * r32, y4 * r41, y4 * r42
            t = 0.25 * p41
            c1 = t * p31
            c2 = t * p32 * m31
            c3 = 0.25 * p42 * p32 * m41
            c12, c23 = c1 + c2, c2 + c3
            c123 = c12 + c3
            second = np.stack([c1 + c12 * m31 + c123 * m41, c123 + c23 * m32 + c3 * m42, c12 * p31 + c23 * p32, c123 * p41 + c3 * p42], axis=-1)
            out[sel] = second[sel]
            sel = (mu >= e[..., 2]) & (mu < e[..., 3])
            y = s4 - es
            q41, q42, q43 = y * r41, y * r42, y * r43
            c = 0.25 * q41 * q42 * q43
            third = np.stack([0.25 - c * q41, 0.25 - c * q42, 0.25 - c * q43, 0.25 - c * (4.0 - (q41 + q42 + q43))], axis=-1)
            out[sel] = third[sel]
        else:
            s1, s2, s3 = (s[..., i] for i in range(3))
            r21, r31, r32 = 1.0 / (s2 - s1), 1.0 / (s3 - s1), 1.0 / (s3 - s2)
            sel = (mu >= e[..., 0]) & (mu < e[..., 1])
            x = es - s1
            q21, q31 = x * r21, x * r31
            c = q21 * q31
            first = np.stack([c * (3.0 - (q21 + q31)), c * q21, c * q31], axis=-1)
            out[sel] = first[sel]
            sel = (mu >= e[..., 1]) & (mu < e[..., 2])
            y = s3 - es
            q31, q32 = y * r31, y * r32
            c = q31 * q32
            second = np.stack([1.0 - c * q31, 1.0 - c * q32, 1.0 - c * (3.0 - (q31 + q32))], axis=-1)
            out[sel] = second[sel]
    return np.clip(out, 0.0, full)


def _simplex_weights(corners, energy):
    """Corner weights in CORNER order (not sorted order) of simplices with corner energies ``corners[..., :]``."""
    e_sorted, order = _stable_sort(corners)
    sorted_w = corner_weights(e_sorted, energy)
    out = np.empty_like(sorted_w)
    np.put_along_axis(out, order, sorted_w, axis=-1)
    return out


def _shift(eig, offset):
    """eig at mesh point v + offset for every v (periodic)."""
    out = eig
    for axis, step in enumerate(offset):
        if step:
            out = np.roll(out, -step, axis=axis)
    return out


def point_weights(eig, energy):
    """w[mesh + (n_orb,)] by the gather, in the kernel's summation order and with its one division."""
    eig = np.asarray(eig, dtype=float)
    dim = eig.ndim - 1
    n_k = int(np.prod(eig.shape[:-1]))
    acc = np.zeros(eig.shape)
    for _, p, offsets in gather_table(dim):
        corners = np.stack([_shift(eig, off) for off in offsets], axis=-1)
        acc = acc + _simplex_weights(corners, energy)[..., p]
    return acc / (6.0 * n_k)


def point_weights_scatter(eig, energy):
    """The same quantity scattered from the simplices of every cell (`dos_model.simplex_corners`): corner c of the simplex with
    axis order sigma of cell v is mesh point v + e_sigma1 + ... + e_sigmac."""
    eig = np.asarray(eig, dtype=float)
    dim = eig.ndim - 1
    n_k = int(np.prod(eig.shape[:-1]))
    acc = np.zeros(eig.shape)
    for sigma, corners in zip(itertools.permutations(range(dim)), dos_model.simplex_corners(eig)):
        weights = _simplex_weights(corners, energy)
        for c in range(dim + 1):
            moved = weights[..., c]
            for axis in sigma[:c]:
                moved = np.roll(moved, 1, axis=axis)  # the weight of cell v belongs to point v + e_axis
            acc = acc + moved
    return acc / (6.0 * n_k)


def point_weights_exact(eig, energy, as_fractions=False):
    """The exact rational w (corner weights of `tetra_exact.corner_weights`), rounded once to doubles (or as Fractions)."""
    eig = np.asarray(eig, dtype=float)
    dim = eig.ndim - 1
    mesh, n_orb = eig.shape[:-1], eig.shape[-1]
    n_k = int(np.prod(mesh))
    n_s = 6 if dim == 3 else 2
    total = np.zeros(eig.shape, dtype=object)
    total[...] = Fraction(0)
    orders = list(itertools.permutations(range(dim)))
    for cell in itertools.product(*[range(n) for n in mesh]):
        for sigma in orders:
            points = [cell]
            for axis in sigma:
                nxt = list(points[-1])
                nxt[axis] = (nxt[axis] + 1) % mesh[axis]
                points.append(tuple(nxt))
            for b in range(n_orb):
                weights = tetra_exact.corner_weights([eig[pt + (b,)] for pt in points], energy)
                for pt, x in zip(points, weights):
                    total[pt + (b,)] += x
    total = total / Fraction(n_s * n_k)
    if as_fractions:
        return total
    return np.array([float(x) for x in total.reshape(-1)]).reshape(eig.shape)


def occupations(w, eig, U):
    """(q[n_orb], f[n_orb], eb[n_orb]) from weights ``w`` and eigenvalues ``eig`` of shape mesh + (n_orb,) and eigenvectors ``U`` of
    shape mesh + (n_orb, n_orb) or (NK, n_orb, n_orb), U[k][i][b] = component i of band b (None: q is None)."""
    w = np.asarray(w, dtype=float)
    n = w.shape[-1]
    flat_w, flat_e = w.reshape(-1, n), np.asarray(eig, dtype=float).reshape(-1, n)
    f = flat_w.sum(axis=0)
    eb = (flat_w * flat_e).sum(axis=0)
    q = None
    if U is not None:
        flat_u = np.asarray(U).reshape(-1, n, n)
        q = np.einsum("kb,kib->i", flat_w, np.abs(flat_u) ** 2)
    return q, f, eb


def main():
    # one band on the mesh (2, 2) with the corner values 0, 1, 2, 3, half filled at mu = 1.5
    eig = np.array([[0.0, 1.0], [2.0, 3.0]]).reshape(2, 2, 1)
    mu = 1.5
    print("gather table (2-D): sigma, own position, corner offsets")
    for sigma, p, offsets in gather_table(2):
        print("   ", sigma, p, offsets)
    gather, scatter = point_weights(eig, mu), point_weights_scatter(eig, mu)
    exact = point_weights_exact(eig, mu, as_fractions=True)
    print("mesh (2, 2), E = 0, 1, 2, 3, mu = %.2f" % mu)
    for idx in itertools.product(range(2), range(2)):
        print("    point %s: gather %.17g  scatter %.17g  exact %s" % (idx, gather[idx + (0,)], scatter[idx + (0,)], exact[idx + (0,)]))
    print("    sum w = %.17g   N(mu) = %.17g" % (gather.sum(), dos_model.nos(eig, [mu])[0]))
    _, f, eb = occupations(gather, eig, None)
    print("    band occupation %.17g, band energy %.17g" % (f[0], eb[0]))


if __name__ == "__main__":
    main()
