#!/usr/bin/env python3
"""
NumPy model of csrc/tbk_tdf.hip: the transport distribution of a uniform, periodic k mesh by the linear tetrahedron method (DESIGN.md
section 30), the statement every test compares with.

Mesh points k = (i_1 / n_1, ..., i_dim / n_dim), ``E, U`` of ``eigh(k, convention=2)``, ``D^a`` and ``V^a = U^H D^a U`` those of
tools/optics_model.py; reduced coordinates, e = hbar = 1, per unit cell, no spin factor::

    w[a,c](k,b) = Re sum_{b' : |E_kb - E_kb'| <= delta}  V^a[b,b'] conj(V^c[b,b'])          delta = degeneracy >= 0
    N[a,c](E)   = 1 / (S NK) sum_simplices sum_b sum_corners  w_corner(E) w[a,c](corner, b)     the cumulative  int^E Sigma[a,c]
    Sigma[a,c]  = diff(N[a,c]) / step                                                          at the bin midpoints

The pair criterion is the plain comparison ``abs(E_b - E_b') <= delta`` on the doubles, not chained into clusters.  For an isolated
band w = v_a v_c; inside a degenerate set the diagonal of V depends on the basis the eigensolver returned, the sum of w over the set,
Re tr(P V^a P V^c), does not.

The kernels integrate G = dim (dim + 1) / 2 NON-NEGATIVE channels (`channels`: the dim diagonals sum |V^a|^2, then sum |V^a + V^c|^2 for
the pairs a < c in the order (0, 1), (0, 2), (1, 2)), each divided by a power of two from `scales`, through the fixed point of the
projected density of states; `from_channels` is the polarization step N[a,c] = (N+[a,c] - N[a,a] - N[c,c]) / 2.  `tolerance` is the
bound of DESIGN.md 30.4: derived, nothing measured on the kernels enters it.

`python tools/tdf_model.py` prints Sigma_xx of the square lattice against a fine sum.  Design tooling: nothing in the product imports it.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optics_model  # noqa: E402  pylint: disable=wrong-import-position
import pdos_model  # noqa: E402  pylint: disable=wrong-import-position

U_ROUND = 2.0 ** -53


def pairs(dim):
    """The pairs a < c in channel order."""
    return [(a, c) for a in range(dim) for c in range(a + 1, dim)]


def mask(E, degeneracy):
    """[NK][n][n]: the pairs (b, b') that enter, ``abs(E_b - E_b') <= degeneracy`` as the kernel writes it."""
    E = np.asarray(E, dtype=float)
    return np.abs(E[:, :, None] - E[:, None, :]) <= degeneracy


def weights(E, U, D, degeneracy=1e-8):
    """w[NK][dim][dim][n] from E [NK][n], U [NK][n][n], D [NK][dim][n][n] (`optics_model.derivatives`)."""
    V = optics_model.velocities(E, U, D)
    keep = mask(E, degeneracy)
    return np.einsum("kabq,kcbq,kbq->kacb", V, V.conj(), keep.astype(float)).real


def channels(E, U, D, degeneracy=1e-8):
    """The G non-negative channels [NK][G][n], unscaled."""
    V = optics_model.velocities(E, U, D)
    keep = mask(E, degeneracy)[:, None]
    dim = V.shape[1]
    diagonal = (np.abs(V) ** 2 * keep).sum(axis=-1)
    mixed = [(np.abs(V[:, a] + V[:, c]) ** 2 * keep[:, 0]).sum(axis=-1) for a, c in pairs(dim)]
    return np.concatenate([diagonal] + [m[:, None] for m in mixed], axis=1) if mixed else diagonal


def from_channels(ch, axis):
    """The polarization step along ``axis`` (of length G): the symmetric [dim][dim] in its place (two axes)."""
    ch = np.moveaxis(np.asarray(ch, dtype=float), axis, 0)
    G = ch.shape[0]
    dim = 2 if G == 3 else 3
    if G != dim * (dim + 1) // 2:
        raise ValueError("3 or 6 channels")
    out = np.empty((dim, dim) + ch.shape[1:])
    for a in range(dim):
        out[a, a] = ch[a]
    for p, (a, c) in enumerate(pairs(dim)):
        out[a, c] = (ch[dim + p] - ch[a] - ch[c]) / 2.0
        out[c, a] = out[a, c]
    return np.moveaxis(out, (0, 1), (axis, axis + 1))


def power_of_two_above(x):
    """The power of two s with x < s <= 2 x (1 for x = 0)."""
    if x == 0.0:
        return 1.0
    return float(np.ldexp(1.0, np.frexp(x)[1]))


def velocity_bounds(r_vec, hop):
    """B_a = sum_R |R_a| ||hop[R]||_F over both halves of the lattice (the packed half is listed: D^a = X + X^H with X the listed sum, so
    twice it): ||D^a(k)||_2 <= B_a for every k."""
    r_vec = np.asarray(r_vec)
    norms = np.sqrt((np.abs(np.asarray(hop)) ** 2).sum(axis=(1, 2)))
    return np.array([2.0 * float((np.abs(r_vec[:, a]).astype(float) * norms).sum()) for a in range(r_vec.shape[1])])


def scales(r_vec, hop):
    """s_g [G]: the power of two above 1.0000001 times the bound of channel g -- B_a^2 for a diagonal (every row sum of |V^a|^2 is a
    diagonal element of V^a V^a^H, at most ||V^a||_2^2 = ||D^a||_2^2), (B_a + B_c)^2 for a pair.  A function of the model alone."""
    B = velocity_bounds(r_vec, hop)
    dim = len(B)
    bounds = [B[a] ** 2 for a in range(dim)] + [(B[a] + B[c]) ** 2 for a, c in pairs(dim)]
    return np.array([power_of_two_above(1.0000001 * b) for b in bounds])


def cumulative(eig, per_state, grid):
    """``pdos_model.pnos`` on any per-state quantity: eig mesh + (n,), per_state mesh + (M, n) -> [M][NE]."""
    return pdos_model.pnos(eig, per_state, grid)


def transport_distribution(E, U, D, mesh, grid, degeneracy=1e-8):
    """(cumulative [dim][dim][NE], tdf [dim][dim][NE - 1]) from the eigensystem of the mesh points in mesh order, through the channels
    as the kernels go."""
    E = np.asarray(E, dtype=float)
    mesh = tuple(int(n) for n in mesh)
    grid = np.asarray(grid, dtype=float)
    ch = channels(E, U, D, degeneracy)
    total = cumulative(E.reshape(mesh + E.shape[1:]), ch.reshape(mesh + ch.shape[1:]), grid)
    N = from_channels(total, 0)
    step = (grid[-1] - grid[0]) / (len(grid) - 1)
    return N, np.diff(N, axis=-1) / step


def weight_tolerance(n, norm, extra=0.0):
    """tol_w of DESIGN.md 30.4 for ONE evaluation of a row sum of n products of two elements of V (or of V^a + V^c), ``norm`` a bound
    on the Frobenius norm of that matrix: 27.4 gives ||dV||_F <= 2 (2 n + 3) sqrt(n) norm u for the two products behind V (+ extra
    norm u for a D^a that is itself rounded, `extra` in units of u); the row sum moves by at most 2 ||dV||_F norm (Cauchy-Schwarz, V
    enters twice), its n products and n - 1 additions by (n + 2) norm^2 u."""
    return (4.0 * (2 * n + 3) * np.sqrt(n) + 2.0 * extra + n + 2.0) * norm * norm * U_ROUND


def tolerance(n, norms, scale, extra=0.0):
    """The bounds of kernel against model on the same (E, U, D), per channel and per tensor element.  ``norms`` [dim]: G_a = max_k
    ||D^a(k)||_F; ``scale`` [G]: `scales`.  Returns a dict:

    ``channel_weights`` [G]     2 tol_w (two evaluations), with norm G_a, or G_a + G_c for a pair;
    ``channel_fixed`` [G]       the accumulate stage alone on the same scaled weights: the last two terms of the next line;
    ``channel_cumulative`` [G]  n times ``channel_weights`` (the corner weights of a band add up to at most 1 per bin, n bands), plus the fixed point,
                                scale 2 n 2^-41 (fractions and steps are both rounded to 2^-40), plus the corner weights' own rounding,
                                fewer than 32 operations on either side: 64 u n scale;
    ``weights``, ``cumulative`` [dim][dim]   the polarization step: the three channels' bounds added and halved off the diagonal."""
    norms = np.asarray(norms, dtype=float)
    scale = np.asarray(scale, dtype=float)
    dim = len(norms)
    channel_norm = np.array([norms[a] for a in range(dim)] + [norms[a] + norms[c] for a, c in pairs(dim)])
    cw = 2.0 * weight_tolerance(n, channel_norm, extra)
    fixed = scale * n * (2.0 ** -40 + 64.0 * U_ROUND)
    cc = n * cw + fixed

    def tensor(ch):
        out = np.empty((dim, dim))
        for a in range(dim):
            out[a, a] = ch[a]
        for p, (a, c) in enumerate(pairs(dim)):
            out[a, c] = out[c, a] = (ch[dim + p] + ch[a] + ch[c]) / 2.0
        return out

    return {"channel_weights": cw, "channel_fixed": fixed, "channel_cumulative": cc, "weights": tensor(cw), "cumulative": tensor(cc)}


def square_lattice(t=1.0):
    """One band, E = 2 t (cos 2 pi k_x + cos 2 pi k_y): packed half-space hoppings."""
    return np.array([[1, 0], [0, 1]], dtype=np.int64), np.full((2, 1, 1), t, dtype=np.complex128)


def square_lattice_sigma(mesh, grid, t=1.0):
    """(N_xx, Sigma_xx) of the square lattice on ``mesh`` by the tetrahedron method."""
    r_vec, hop = square_lattice(t)
    k = optics_model.mesh_kpoints(mesh)
    E = (2.0 * t * np.cos(2.0 * np.pi * k).sum(axis=1))[:, None]
    U = np.ones((len(k), 1, 1), dtype=complex)
    D = optics_model.derivatives(r_vec, hop, k)
    N, sigma = transport_distribution(E, U, D, mesh, grid, 0.0)
    return N[0, 0], sigma[0, 0]


def square_lattice_reference(grid, fine=1024, t=1.0):
    """N_xx at the grid energies from a plain sum over a fine x fine mesh shifted off the symmetry points: (1 / NK) sum v_x^2 theta(E - E_k)."""
    x = (np.arange(fine) + 0.5) / fine
    cx = np.cos(2.0 * np.pi * x)
    E = 2.0 * t * (cx[:, None] + cx[None, :])
    v2 = np.broadcast_to(((2.0 * t * np.sin(2.0 * np.pi * x)) ** 2)[:, None], E.shape)
    order = np.argsort(E, axis=None)
    running = np.cumsum(v2.reshape(-1)[order]) / E.size
    idx = np.searchsorted(E.reshape(-1)[order], np.asarray(grid, dtype=float), side="right")
    return np.where(idx > 0, running[np.maximum(idx, 1) - 1], 0.0)


def main():
    grid = np.linspace(-4.5, 4.5, 37)
    want = square_lattice_reference(grid)
    for n in (16, 32, 64):
        got, _ = square_lattice_sigma((n, n), grid)
        print("square lattice %3d x %3d: max|N_xx - fine sum| = %.3e (h^2 = %.3e), N_xx(top) = %.6f" % (n, n, np.abs(got - want).max(), 1.0 / n ** 2, got[-1]))


if __name__ == "__main__":
    main()
