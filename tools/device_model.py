#!/usr/bin/env python3
"""
NumPy model of the layer-resolved Green's functions of csrc/tbk_device_green.hip: the device of
tools/transport_model.py, its diagonal blocks G_pp, the blocks (p, 1) and (p, M), the local density of states per layer and orbital and
the parts of it injected from the two leads.

a, H00, H01, N = size L, V_p, the decimation, es, et, Gamma_R, Gamma_L, g_p, D_p and P_p are exactly those of transport_model (DESIGN.md
22.1); below Q_p is its P_p.  Per (kp, z), Im z != 0, after the forward sweep of transport_model.transmission, unchanged down to the
order of the operations:

    G_M = g_M                      C_M = g_M
    for p = M - 1 ... 1:   X = g_p H01          Y = H01^H g_p
                           G_p = g_p + (X G_{p+1}) Y            diagonal block (p, p) of the full resolvent
                           C_p = X C_{p+1}                      block (p, M)
    F_1 = G_1;   F_p = G_p (H01^H Q_{p-1})  (1 < p < M);   F_M = Q_M   (M > 1)      block (p, 1)
    ldos[p][i]  = -Im G_p[i][i] / pi
    left[p][i]  = Re sum_j (F_p Gamma_L)[i][j] conj(F_p[i][j]) / (2 pi)      injected from the left lead
    right[p][i] = Re sum_j (C_p Gamma_R)[i][j] conj(C_p[i][j]) / (2 pi)      injected from the right lead
    T = Re tr[(Gamma_R Q_M)(Gamma_L Q_M^H)]                                   transport_model's, unchanged

Products are formed as bracketed; the order is part of the definition.  The kernel differs from this file only in the summation order
inside a product and inside a row sum.

Properties.  (1) ldos - left - right = (Im z / pi) sum_q sum_j |G_pq[i][j]|^2: it has the sign of Im z and vanishes as eta -> 0.  (2)
With V = 0, G_p is the bulk Green's function of surface_model.decimate for every p.  (3) F_M and T have the bits of
transport_model.transmission.  (4) The bits of one (kp, z) depend on nothing else.

`device_dense` is an independent route: the blocks of the dense (M N) x (M N) inverse of transport_model.transmission_dense.
`device_mp` is the same sweep in mpmath.  `chain_closed_form` is the local G of the chain with one impurity.

`python tools/device_model.py` prints a small table; `--golden` writes tests/golden/device_mp.npz.  Design tooling: nothing in the
product imports it.
"""

import collections

import numpy as np

import surface_model as sm
import transport_model as tm

U_ROUND = sm.U_ROUND
MAX_ITERATIONS = sm.MAX_ITERATIONS

DeviceGreen = collections.namedtuple("DeviceGreen", ("T", "G", "F", "C", "ldos", "left", "right", "iterations", "rho", "g", "Q", "es", "et"))


def _row_sums(a, b):
    """Re sum_j a[i][j] conj(b[i][j]) / (2 pi), per row"""
    return (a.real * b.real + a.imag * b.imag).sum(axis=1) / (2.0 * np.pi)


def device_green(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """`DeviceGreen` of one (kp, z): T, the blocks G, F, C [M][N][N], ldos, left, right [M][N], the count of the decimation, the
    largest growth factor of all inversions, and what the forward sweep keeps (g, Q [M][N][N]; es, et).  The forward sweep is
    transport_model.transmission's, statement by statement.  numpy.linalg.LinAlgError when the cap is reached, an inversion is singular
    or a block is not finite."""
    H00 = np.asarray(H00, dtype=np.complex128)
    N = H00.shape[0]
    V = tm._device_argument(V, N)  # pylint: disable=protected-access
    M = V.shape[0]
    es, et, iterations, rho = tm.lead_terms(H00, H01, z, max_iterations=max_iterations)
    H01 = np.asarray(H01, dtype=np.complex128)
    H10 = H01.conj().T.copy()
    one = np.eye(N)
    g = np.empty((M, N, N), dtype=np.complex128)
    Q = np.empty((M, N, N), dtype=np.complex128)
    HQ = np.zeros((M, N, N), dtype=np.complex128)  # HQ[p] = H01^H Q_{p-1}
    D = et + V[0]
    P = None
    for p in range(M):
        if p == M - 1:
            D = D + (es - H00)
        g[p], growth = sm._invert(z * one - D)  # pylint: disable=protected-access
        rho = max(rho, growth)
        with np.errstate(all="ignore"):
            if p > 0:
                HQ[p] = H10 @ P
            P = g[p] if p == 0 else g[p] @ HQ[p]
            if p < M - 1:
                D = (H00 + V[p + 1]) + H10 @ (g[p] @ H01)
        Q[p] = P
    gamma_r, gamma_l = tm._broadening(es), tm._broadening(et)  # pylint: disable=protected-access
    T = tm._trace_of_product(gamma_r @ P, gamma_l @ P.conj().T)  # pylint: disable=protected-access
    G, F, C = np.empty_like(g), np.empty_like(g), np.empty_like(g)
    with np.errstate(all="ignore"):
        G[M - 1] = g[M - 1]
        C[M - 1] = g[M - 1]
        for p in range(M - 2, -1, -1):
            X = g[p] @ H01
            Y = H10 @ g[p]
            G[p] = g[p] + (X @ G[p + 1]) @ Y
            C[p] = X @ C[p + 1]
        for p in range(M):
            if p == M - 1:
                F[p] = Q[p]
            elif p == 0:
                F[p] = G[p]
            else:
                F[p] = G[p] @ HQ[p]
        ldos = np.array([-np.diagonal(G[p]).imag / np.pi for p in range(M)])
        left = np.array([_row_sums(F[p] @ gamma_l, F[p]) for p in range(M)])
        right = np.array([_row_sums(C[p] @ gamma_r, C[p]) for p in range(M)])
    for block in (g, G, F, C):
        if not np.all(np.isfinite(block.view(float))):
            raise np.linalg.LinAlgError("Singular matrix")
    return DeviceGreen(T, G, F, C, ldos, left, right, iterations, rho, g, Q, es, et)


def device_dense(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """(G, F, C [M][N][N], rows [M][N][M N]) from the dense inverse of transport_model.transmission_dense: the blocks (p, p), (p, 1),
    (p, M) and the full block rows."""
    N = np.shape(H00)[0]
    _, _, full = tm.transmission_dense(H00, H01, V, z, max_iterations=max_iterations)
    M = full.shape[0] // N
    blocks = full.reshape(M, N, M, N)
    G = np.array([blocks[p, :, p, :] for p in range(M)])
    F = np.array([blocks[p, :, 0, :] for p in range(M)])
    C = np.array([blocks[p, :, M - 1, :] for p in range(M)])
    return G, F, C, full.reshape(M, N, M * N)


def device_mp(H00, H01, V, z, *, digits=60):
    """(T, G, F, C, ldos, left, right) as floats and complex128 / float64 arrays from the same decimation and the same two sweeps in
    mpmath at `digits` digits, the decimation run as in transport_model.transmission_mp (N <= 24: mpmath's matrices are slow)."""
    import mpmath  # pylint: disable=import-outside-toplevel

    N = np.shape(H00)[0]
    V = tm._device_argument(V, N)  # pylint: disable=protected-access
    M = V.shape[0]
    with mpmath.workdps(digits):
        def lift(a):
            a = np.asarray(a, dtype=np.complex128)
            return mpmath.matrix([[mpmath.mpc(float(x.real), float(x.imag)) for x in row] for row in a])

        def lower(a):
            return np.array([[complex(a[i, j]) for j in range(N)] for i in range(N)])

        zz = mpmath.mpc(float(np.real(z)), float(np.imag(z))) * mpmath.eye(N)
        h00 = lift(H00)
        es, et, e = lift(H00), lift(H00), lift(H00)
        alpha = lift(H01)
        beta = alpha.H
        h01, h10 = alpha.copy(), beta.copy()
        stop = mpmath.mpf(10) ** (10 - digits) * mpmath.mnorm(alpha, "inf")
        for _ in range(400):
            gg = mpmath.inverse(zz - e)
            t = gg * alpha
            p2 = beta * t
            a_new = alpha * t
            t = gg * beta
            p3 = alpha * t
            b_new = beta * t
            et, es, e = et + p2, es + p3, e + p2 + p3
            alpha, beta = a_new, b_new
            if max(mpmath.mnorm(alpha, "inf"), mpmath.mnorm(beta, "inf")) <= stop:
                break
        else:
            raise np.linalg.LinAlgError("the reference did not converge")
        g, Q = [], []
        D = et + lift(V[0])
        for p in range(M):
            if p == M - 1:
                D = D + (es - h00)
            g.append(mpmath.inverse(zz - D))
            Q.append(g[p] if p == 0 else g[p] * (h10 * Q[p - 1]))
            if p < M - 1:
                D = h00 + lift(V[p + 1]) + h10 * (g[p] * h01)
        gamma_r = mpmath.mpc(0, 1) * (es - es.H)
        gamma_l = mpmath.mpc(0, 1) * (et - et.H)
        a = gamma_r * Q[M - 1]
        b = gamma_l * Q[M - 1].H
        total = mpmath.mpf(0)
        for i in range(N):
            for j in range(N):
                total += (a[i, j] * b[j, i]).real
        G, C = [None] * M, [None] * M
        G[M - 1] = C[M - 1] = g[M - 1]
        for p in range(M - 2, -1, -1):
            X = g[p] * h01
            G[p] = g[p] + (X * G[p + 1]) * (h10 * g[p])
            C[p] = X * C[p + 1]
        F = [Q[p] if p == M - 1 else G[p] if p == 0 else G[p] * (h10 * Q[p - 1]) for p in range(M)]

        def injected(B, gamma):
            A = B * gamma
            return [float(sum((A[i, j] * B[i, j].conjugate()).real for j in range(N)) / (2 * mpmath.pi)) for i in range(N)]

        ldos = np.array([[float(-G[p][i, i].imag / mpmath.pi) for i in range(N)] for p in range(M)])
        left = np.array([injected(F[p], gamma_l) for p in range(M)])
        right = np.array([injected(C[p], gamma_r) for p in range(M)])
        return (float(total), np.array([lower(x) for x in G]), np.array([lower(x) for x in F]), np.array([lower(x) for x in C]), ldos, left, right)


def chain_closed_form(z, t, t_plane, kpar, eps):
    """The local G of the chain of surface_model.chain_closed_form on its one impurity site (M = 1, V_1 = eps): with g_s the surface
    function of the clean half chain, G = 1 / (zeta - eps - 2 t^2 g_s).  Exact at any eta."""
    g_s, _ = sm.chain_closed_form(z, t, t_plane, kpar)
    zeta = z - 2.0 * t_plane * np.cos(2.0 * np.pi * kpar)
    return 1.0 / (zeta - eps - 2.0 * t * t * g_s)


Tolerance = collections.namedtuple("Tolerance", ("T", "G", "F", "C", "ldos", "left", "right", "sG", "sF", "sC", "sL", "sR"))


def tolerance(H00, H01, V, z, result):
    """The bounds of one (kp, z) from the model's own run `result` (a `DeviceGreen`): `Tolerance` with T a number, G, F, C, ldos, left,
    right [M] (per component of layer p's block or row) and the scales they are relative to.

    E = transport_model.relative_error: 8 N u rho kappa_2 (iterations + M + 1), kappa_2 <= (|z| + |H00| + 2 |H01| + max |V_p|) / eta,
    the normwise relative error of a factor that has all inversions of the forward sweep behind it, counted as if their errors added
    (DESIGN.md 22.5).  Every g_p and Q_p is such a factor (a product's own rounding, N u of the norms of its operands, is below one
    inversion's and is covered by the + 1).  A block B of the backward sweep is a sum of products of such factors and of the block of
    the layer above; with the errors again counted as if they added, relative to the 2-norms of the blocks that multiply them:

        |B - exact| <= E c(B) s(B)
        s(G_M) = |g_M|,  s(G_p) = |g_p| + |X_p| |G_{p+1}| |Y_p|        c(G_p) = 3 (M - p) + 1      (g_p, X_p, Y_p, and the layer above)
        s(C_M) = |g_M|,  s(C_p) = |X_p| |C_{p+1}|                      c(C_p) = (M - p) + 1
        s(F_1) = s(G_1), s(F_p) = |G_p| |H01^H Q_{p-1}|, s(F_M) = |Q_M|  c(F_p) = c(G_p) + p - 1,  c(F_M) = M

    The norms are those of the model's blocks themselves: no power of |H01| / eta per backward step enters.  ldos carries G's bound
    over pi.  left = sum_j (F Gamma_L) conj(F) / (2 pi) has two factors F and one Gamma_L, whose relative error is E against 2 |H01|^2
    |G_top| (22.5): (2 c(F_p) + 1) E s(F_p)^2 (2 |H01|^2 |G_top|) / (2 pi); right the same with C, es and G_bottom.  T: 22.5's."""
    H00 = np.asarray(H00, dtype=np.complex128)
    H01 = np.asarray(H01, dtype=np.complex128)
    N = H00.shape[0]
    M = result.G.shape[0]
    H10 = H01.conj().T
    E = tm.relative_error(H00, H01, V, z, result.iterations, result.rho)
    norm = lambda a: float(np.linalg.norm(a, 2))  # noqa: E731
    one = np.eye(N)
    b2 = norm(H01) ** 2
    gamma_l = 2.0 * b2 * norm(np.linalg.inv(z * one - result.et))
    gamma_r = 2.0 * b2 * norm(np.linalg.inv(z * one - result.es))
    sG, sF, sC = np.empty(M), np.empty(M), np.empty(M)
    cG, cF, cC = np.empty(M), np.empty(M), np.empty(M)
    for p in range(M - 1, -1, -1):  # p from 0: layer p + 1 of the docstring
        layer = p + 1
        if p == M - 1:
            sG[p] = sC[p] = norm(result.g[p])
        else:
            X, Y = result.g[p] @ H01, H10 @ result.g[p]
            sG[p] = norm(result.g[p]) + norm(X) * norm(result.G[p + 1]) * norm(Y)
            sC[p] = norm(X) * norm(result.C[p + 1])
        cG[p] = 3.0 * (M - layer) + 1.0
        cC[p] = (M - layer) + 1.0
        if p == M - 1:
            sF[p], cF[p] = norm(result.Q[p]), float(M)
        elif p == 0:
            sF[p], cF[p] = sG[p], cG[p]
        else:
            sF[p], cF[p] = norm(result.G[p]) * norm(H10 @ result.Q[p - 1]), cG[p] + layer - 1.0
    sL = sF ** 2 * gamma_l / (2.0 * np.pi)
    sR = sC ** 2 * gamma_r / (2.0 * np.pi)
    scale_T = float(N * gamma_r * gamma_l * norm(result.Q[M - 1]) ** 2)
    return Tolerance(4.0 * E * scale_T, E * cG * sG, E * cF * sF, E * cC * sC, E * cG * sG / np.pi, (2.0 * cF + 1.0) * E * sL, (2.0 * cC + 1.0) * E * sR,
                     sG, sF, sC, sL, sR)


#: (n, L, M) of tests/test_gpu_device_green.py: N = 1, 3, 16, 17, 32, 33 and 64; M = 1: no backward step; (5, 1, 6): a deep stack
GPU_CASES = [(1, 1, 1), (3, 1, 2), (8, 2, 3), (17, 1, 2), (8, 4, 2), (11, 3, 2), (16, 4, 3), (64, 1, 1), (64, 1, 2), (5, 1, 6)]
GPU_Z = tm.GPU_Z
GPU_NK = tm.GPU_NK
gpu_case = tm.gpu_case


def device_green_function(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """[NK][NZ] lists of `DeviceGreen` and of `Tolerance` from H00, H01 [NK][N][N] and V [M][N][N]."""
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    results, bounds = [], []
    for k in range(np.shape(H00)[0]):
        results.append([device_green(H00[k], H01[k], V, complex(zz), max_iterations=max_iterations) for zz in z])
        bounds.append([tolerance(H00[k], H01[k], V, complex(zz), r) for zz, r in zip(z, results[-1])])
    return results, bounds


def stack(items, name):
    """the field `name` of a [NK][NZ] list of named tuples as one array"""
    return np.array([[getattr(x, name) for x in row] for row in items])


def write_golden(path):
    """T, ldos, left, right of `device_mp` at 60 digits for the GPU cases with N <= 17, [3][5][M][N] each (T: [3][5])."""
    out = {"Z": GPU_Z}
    for n, L, M in GPU_CASES:
        if n * L > 17:
            continue
        H00, H01, V = gpu_case(n, L, M)
        rows = [[device_mp(H00[k], H01[k], V, complex(z)) for z in GPU_Z] for k in range(GPU_NK)]
        tag = "_%d_%d_%d" % (n, L, M)
        out["T" + tag] = np.array([[x[0] for x in row] for row in rows])
        out["ldos" + tag] = np.array([[x[4] for x in row] for row in rows])
        out["left" + tag] = np.array([[x[5] for x in row] for row in rows])
        out["right" + tag] = np.array([[x[6] for x in row] for row in rows])
        print("(n, L, M) = (%d, %d, %d) done" % (n, L, M), flush=True)
    np.savez(path, **out)


def main():
    print("the GPU cases: the model against the dense inverse, and the bounds")
    for n, L, M in GPU_CASES:
        if n * L > 33:
            continue
        H00, H01, V = gpu_case(n, L, M)
        worst, bound, excess = 0.0, 0.0, np.inf
        for z in GPU_Z:
            r = device_green(H00[0], H01[0], V, complex(z))
            tol = tolerance(H00[0], H01[0], V, complex(z), r)
            G, F, C, _ = device_dense(H00[0], H01[0], V, complex(z))
            for got, want, t in ((r.G, G, tol.G), (r.F, F, tol.F), (r.C, C, tol.C)):
                err = np.abs(got - want).reshape(M, -1).max(axis=1)
                worst, bound = max(worst, err.max()), max(bound, t.max())
            excess = min(excess, float(((r.ldos - r.left - r.right) * np.sign(z.imag)).min()))
        print("    (n, L, M) = (%2d, %d, %d): max|block - dense| = %.2e, largest bound %.2e, min (ldos - left - right) sign(Im z) = %.2e" % (n, L, M, worst, bound, excess))


if __name__ == "__main__":
    import os
    import sys

    if "--golden" in sys.argv:
        write_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "device_mp.npz"))
    else:
        main()
