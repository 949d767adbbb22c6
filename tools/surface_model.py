#!/usr/bin/env python3
"""
NumPy model of the surface Green's function of csrc/tbk_surface.hip: the iterative decimation of Lopez
Sancho, Lopez Sancho and Rubio (J. Phys. F 15, 851 (1985)) on principal layers of a tight-binding model.

With a the stacking axis, n the orbitals of a cell and hop_full[R] the full hopping matrices (hamilton(k, convention=2) =
sum_R exp(2 pi i k.R) hop_full[R]), at an in-plane point kp (the reduced coordinates without component a):

    H_m(kp)   = sum_{R : R_a = m} exp(2 pi i kp.Rp) hop_full[R]          m = -L ... L,  H_{-m} = H_m^H
    L         = max |R_a|                                               cells in a principal layer;  N = n L  (n when L = 0)
    H00[p, q] = H_{q - p}                  p, q = 0 ... L - 1           blocks of n x n, cell p at position p along +a
    H01[p, q] = H_{L + q - p} if q <= p, else 0                         principal layer P to P + 1

and per (kp, z), Im z != 0, from es = et = e = H00, alpha = H01, beta = H01^H:

    repeat   g = (z 1 - e)^-1                                          `dyson_model.invert`: the kernel's elimination
             T = g alpha;  e = e + beta T;  et = et + beta T;  A' = alpha T
             T = g beta;   e = e + alpha T; es = es + alpha T; B' = beta T
             alpha, beta = A', B'
    until    max(|alpha|_inf, |beta|_inf) <= 2^-53 |H01|_inf            row sums of |re| + |im|, checked after every update
    G_bottom = (z - es)^-1    the crystal on principal layers P >= 0, its surface cell is block 0
    G_top    = (z - et)^-1    the crystal on principal layers P <= 0, its surface cell is block L - 1
    G_bulk   = (z - e)^-1     a principal layer deep inside

`layers_direct` is the definition of H_m; `layers_from_samples` is what the library does -- H(kp, k_a) = sum_m H_m exp(2 pi i m k_a)
is a trigonometric polynomial of degree L, sampled at k_a = j / (2 L + 1) and inverted by a discrete Fourier sum.

`python tools/surface_model.py` prints the chain against its closed form.  Design tooling: nothing in the product imports it.
"""

import numpy as np

import dyson_model

U_ROUND = 2.0 ** -53
MAX_ITERATIONS = 64


def full_hoppings(r_vec, hop):
    """{R: matrix} over both half spaces from the packed half-space arrays of `Model.from_packed` (H(k) = sum over the stored R of
    exp(2 pi i k.R) hop[R] + its Hermitian conjugate)."""
    full = {}
    for R, mat in zip(np.asarray(r_vec), np.asarray(hop, dtype=np.complex128)):
        key = tuple(int(x) for x in R)
        minus = tuple(-x for x in key)
        full[key] = full.get(key, 0) + mat
        full[minus] = full.get(minus, 0) + mat.conj().T
    return full


def layer_count(full, axis):
    """L = max |R_a| over the hoppings that are not identically zero keys of the model."""
    return max([abs(R[axis]) for R in full] or [0])


def layers_direct(full, axis, kpar, L):
    """H_m [2 L + 1][n][n] (index m + L) at the in-plane point kpar [dim - 1] by direct summation."""
    n = next(iter(full.values())).shape[0]
    out = np.zeros((2 * L + 1, n, n), dtype=np.complex128)
    kpar = np.asarray(kpar, dtype=float).reshape(-1)
    for R, mat in full.items():
        rest = [x for d, x in enumerate(R) if d != axis]
        out[R[axis] + L] += np.exp(2j * np.pi * float(np.dot(kpar, rest))) * mat
    return out


def sample_points(kpar, axis, L, dim):
    """The 2 L + 1 full k-points (kpar with k_a = j / (2 L + 1) inserted at `axis`) the extraction samples, [2 L + 1][dim]."""
    kpar = np.asarray(kpar, dtype=float).reshape(-1)
    pts = np.empty((2 * L + 1, dim))
    for j in range(2 * L + 1):
        pts[j] = np.insert(kpar, axis, j / (2 * L + 1.0))
    return pts


def twiddles(L):
    """(cos, sin) [2 L + 1][2 L + 1][2] of -2 pi ((m j) mod (2 L + 1)) / (2 L + 1), row m + L: the host table of the library."""
    M = 2 * L + 1
    m = np.arange(-L, L + 1)[:, None]
    j = np.arange(M)[None, :]
    angle = -2.0 * np.pi * ((m * j) % M) / M
    return np.stack([np.cos(angle), np.sin(angle)], axis=-1)


def layers_from_samples(samples):
    """H_m [2 L + 1][n][n] from H(kpar, j / (2 L + 1)) [2 L + 1][n][n]: (sum_j w[m][j] H_j) / (2 L + 1), j ascending."""
    samples = np.asarray(samples, dtype=np.complex128)
    M = samples.shape[0]
    L = (M - 1) // 2
    tw = twiddles(L)
    w = tw[..., 0] + 1j * tw[..., 1]
    out = np.zeros_like(samples)
    for j in range(M):
        out = out + w[:, j, None, None] * samples[j][None]
    return out / float(M)


def principal(layers):
    """(H00, H01) [N][N] from H_m [2 L + 1][n][n]; H01 is None for L = 0."""
    layers = np.asarray(layers, dtype=np.complex128)
    L = (layers.shape[0] - 1) // 2
    n = layers.shape[1]
    if L == 0:
        return layers[0].copy(), None
    H00 = np.zeros((L * n, L * n), dtype=np.complex128)
    H01 = np.zeros_like(H00)
    for p in range(L):
        for q in range(L):
            H00[p * n:(p + 1) * n, q * n:(q + 1) * n] = layers[(q - p) + L]
            if q <= p:
                H01[p * n:(p + 1) * n, q * n:(q + 1) * n] = layers[(L + q - p) + L]
    return H00, H01


def norm_inf(a):
    """max over rows of sum over columns of |re| + |im|."""
    a = np.asarray(a)
    return float((np.abs(a.real) + np.abs(a.imag)).sum(axis=1).max()) if a.size else 0.0


def _invert(a):
    """(inverse, rho) by `dyson_model.invert`.  Its growth factor counts the elements of the inverse, which appear in place while the
    elimination runs; rho here is the largest element of the elimination over the largest of input AND result, so that a large
    inverse (|g| up to 1 / eta) is not booked as growth."""
    g, growth, _ = dyson_model.invert(a)
    scale = float(np.abs(a).max())
    return g, max(1.0, growth * scale / max(scale, float(np.abs(g).max())))


def decimate_terms(H00, H01, z, *, max_iterations=MAX_ITERATIONS, to_zero=False):
    """(es, et, e, iterations, rho) of one (kpar, z): the loop of the decimation without its closing inversions -- what `decimate`
    inverts, and what tools/transport_model.py takes the lead self-energies es - H00 and et - H00 from."""
    H00 = np.asarray(H00, dtype=np.complex128)
    N = H00.shape[0]
    one = np.eye(N)
    es, et, e = H00.copy(), H00.copy(), H00.copy()
    iterations, rho = 0, 1.0
    if H01 is not None:
        alpha = np.asarray(H01, dtype=np.complex128).copy()
        beta = alpha.conj().T.copy()
        threshold = 0.0 if to_zero else U_ROUND * norm_inf(alpha)
        while True:
            g, growth = _invert(z * one - e)
            rho = max(rho, growth)
            with np.errstate(all="ignore"):
                t = g @ alpha
                p2 = beta @ t
                a_new = alpha @ t
                et = et + p2
                e = e + p2
                t = g @ beta
                p3 = alpha @ t
                b_new = beta @ t
                es = es + p3
                e = e + p3
            alpha, beta = a_new, b_new
            iterations += 1
            size = max(norm_inf(alpha), norm_inf(beta))
            if not np.isfinite(size):
                raise np.linalg.LinAlgError("Singular matrix")
            if size <= threshold:
                break
            if iterations >= max_iterations:
                raise np.linalg.LinAlgError("no convergence in %d iterations" % max_iterations)
    return es, et, e, iterations, rho


def decimate(H00, H01, z, *, max_iterations=MAX_ITERATIONS, to_zero=False):
    """(G_bottom, G_top, G_bulk, iterations, rho) of one (kpar, z).  rho: the largest growth factor of the inversions.  to_zero: run
    alpha and beta down to exact zero instead of the stopping rule (the rule's test).  numpy.linalg.LinAlgError when the cap is
    reached or an inversion is singular."""
    es, et, e, iterations, rho = decimate_terms(H00, H01, z, max_iterations=max_iterations, to_zero=to_zero)
    one = np.eye(es.shape[0])
    out = []
    for m in (es, et, e):
        g, growth = _invert(z * one - m)
        rho = max(rho, growth)
        out.append(g)
    return out[0], out[1], out[2], iterations, rho


def decimate_mp(H00, H01, z, *, digits=60):
    """(G_bottom, G_top, G_bulk) as complex128 arrays from the same iteration in mpmath at `digits` digits, run until alpha and beta
    are below 10^-(digits - 10) |H01|: the reference `tolerance` is checked against (N <= 24: mpmath's matrices are slow)."""
    import mpmath  # pylint: disable=import-outside-toplevel

    with mpmath.workdps(digits):
        def lift(a):
            a = np.asarray(a, dtype=np.complex128)
            return mpmath.matrix([[mpmath.mpc(float(x.real), float(x.imag)) for x in row] for row in a])

        N = np.shape(H00)[0]
        zz = mpmath.mpc(float(np.real(z)), float(np.imag(z))) * mpmath.eye(N)
        es, et, e = lift(H00), lift(H00), lift(H00)
        if H01 is not None:
            alpha = lift(H01)
            beta = alpha.H
            stop = mpmath.mpf(10) ** (10 - digits) * mpmath.mnorm(alpha, "inf")
            for _ in range(400):
                g = mpmath.inverse(zz - e)
                t = g * alpha
                p2 = beta * t
                a_new = alpha * t
                t = g * beta
                p3 = alpha * t
                b_new = beta * t
                et, es, e = et + p2, es + p3, e + p2 + p3
                alpha, beta = a_new, b_new
                if max(mpmath.mnorm(alpha, "inf"), mpmath.mnorm(beta, "inf")) <= stop:
                    break
            else:
                raise np.linalg.LinAlgError("the reference did not converge")
        out = []
        for m in (es, et, e):
            g = mpmath.inverse(zz - m)
            out.append(np.array([[complex(g[i, j]) for j in range(N)] for i in range(N)]))
    return out[0], out[1], out[2]


def surface_green_function(H00, H01, z, *, max_iterations=MAX_ITERATIONS):
    """(bottom, top, bulk [NK][NZ][N][N], iterations [NK][NZ], rho [NK][NZ]) from H00, H01 [NK][N][N] (H01 None: L = 0)."""
    H00 = np.asarray(H00, dtype=np.complex128)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    n_k, N = H00.shape[0], H00.shape[-1]
    G = np.empty((3, n_k, len(z), N, N), dtype=np.complex128)
    its = np.zeros((n_k, len(z)), dtype=np.int32)
    rho = np.ones((n_k, len(z)))
    for k in range(n_k):
        for i, zz in enumerate(z):
            b, t, m, its[k, i], rho[k, i] = decimate(H00[k], None if H01 is None else H01[k], complex(zz), max_iterations=max_iterations)
            G[0, k, i], G[1, k, i], G[2, k, i] = b, t, m
    return G[0], G[1], G[2], its, rho


def spectral(G):
    """-Im diag(G) / pi."""
    return -np.diagonal(G, axis1=-2, axis2=-1).imag / np.pi


def tolerance(H00, H01, z, iterations, rho):
    """The bound per component of the three functions, [NK][NZ], from what is known before the run:

        8 N u rho (|z| + |H|) / eta^2 (iterations + 1),      |H| = |H00|_2 + 2 |H01|_2,  eta = |Im z|

    Every step preserves causality (e, es, et are H00 plus self-energies with Im of the sign opposite to Im z), so |g|_2 <= 1 / eta
    and kappa_2(z - e) <= (|z| + |e|_2) / eta; one inversion then errs by 8 N u rho kappa_2 |g| (the form of dyson_model.tolerance)
    and the iterations + 1 inversions of a result are counted as if their errors added.  rho is the growth factor of the model's
    eliminations as `_invert` defines it, iterations the model's count (numbers or arrays [NK][NZ])."""
    H00 = np.asarray(H00, dtype=np.complex128)
    N = H00.shape[-1]
    H00 = H00.reshape(-1, N, N)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    size = np.linalg.norm(H00, 2, axis=(1, 2))
    if H01 is not None:
        size = size + 2.0 * np.linalg.norm(np.asarray(H01, dtype=np.complex128).reshape(-1, N, N), 2, axis=(1, 2))
    eta = np.abs(z.imag)[None, :]
    rho = np.broadcast_to(np.asarray(rho, dtype=float), (H00.shape[0], len(z)))
    iterations = np.broadcast_to(np.asarray(iterations, dtype=float), (H00.shape[0], len(z)))
    return 8.0 * N * U_ROUND * rho * (np.abs(z)[None, :] + size[:, None]) / eta ** 2 * (iterations + 1.0)


def random_case(n, L, n_k, seed):
    """Test inputs: H_m [NK][2 L + 1][n][n] with H_{-m} = H_m^H, scaled so that sum_m |H_m|_2 <= 2 (the bulk spectrum lies in
    [-2, 2]), and their (H00, H01) [NK][N][N] (H01 None for L = 0)."""
    rng = np.random.default_rng(seed)
    layers = np.zeros((n_k, 2 * L + 1, n, n), dtype=np.complex128)
    for k in range(n_k):
        for m in range(L + 1):
            a = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
            if m == 0:
                a = (a + a.conj().T) / 2
            layers[k, L + m] = a
            layers[k, L - m] = a.conj().T
        total = sum(np.linalg.norm(layers[k, j], 2) for j in range(2 * L + 1))
        layers[k] *= 2.0 / total
    pairs = [principal(layers[k]) for k in range(n_k)]
    H00 = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
    H01 = None if L == 0 else np.ascontiguousarray(np.stack([p[1] for p in pairs]))
    return layers, H00, H01


def chain_closed_form(z, t, t_plane, kpar):
    """(G_surface, G_bulk) of the chain: one orbital, hopping t along a and t_plane in the plane (2-D lattice, kpar a number)."""
    zeta = z - 2.0 * t_plane * np.cos(2.0 * np.pi * kpar)
    root = np.sqrt(zeta * zeta - 4.0 * t * t + 0j)
    g = (zeta - root) / (2.0 * t * t)
    if g.imag * z.imag > 0:  # the branch where Im G and Im z have opposite signs
        root = -root
        g = (zeta - root) / (2.0 * t * t)
    return g, 1.0 / root


def main():
    t, t_plane, kpar = 1.0, 0.3, 0.17
    full = {(0, 1): np.array([[t]]), (0, -1): np.array([[t]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    layers = layers_direct(full, 1, [kpar], 1)
    H00, H01 = principal(layers)
    print("the chain: t = %g along a, t' = %g in the plane, k = %g" % (t, t_plane, kpar))
    for z in (0.4 + 0.5j, 0.4 + 0.05j, 1.9 - 0.05j, 2.0 + 1e-3j):
        b, top, bulk, its, rho = decimate(H00, H01, z)
        gs, gb = chain_closed_form(z, t, t_plane, kpar)
        bound = tolerance(H00[None], H01[None], z, its, rho)[0, 0]
        print("    z = %-14s %2d iterations  |G_bottom - closed| = %.2e  |G_top - closed| = %.2e  |G_bulk - closed| = %.2e  (bound %.2e)"
              % (z, its, abs(b[0, 0] - gs), abs(top[0, 0] - gs), abs(bulk[0, 0] - gb), bound))


if __name__ == "__main__":
    main()
