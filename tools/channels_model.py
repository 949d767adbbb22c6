#!/usr/bin/env python3
"""
NumPy model of the transmission eigenvalues of csrc/tbk_channels.hip: the eigenvalues T_n in [0, 1] of the
matrix whose trace is the Landauer transmission of tools/transport_model.py, and the shot noise sum_n T_n (1 - T_n).

Per (kp, z, sample) the decimation and the sweep of `transport_model` give es, et and P_M.  With s = sign(Im z):

    B_R = s i (es - es^H),  B_L = s i (et - et^H)     element by element, as `transport_model._broadening`; Hermitian, positive
                                                      semidefinite up to rounding for either sign of Im z
    B = L L^H                                         `pivoted_cholesky`: diagonal pivoting, the largest remaining diagonal first
                                                      (ties: the lowest index, a NaN counts as +inf); it stops at rank r when the
                                                      largest remaining diagonal is <= N u d0, d0 the largest diagonal of B, u = 2^-53.
                                                      Step j writes its column of L into column perm[j], the pivot's own: the
                                                      factor is L up to a permutation of its columns kept in the table perm, the
                                                      r columns taken hold B = L L^H whatever their order, the others are zero.
    t = L_R^H (P_M L_L)                               two products, bracketed as written;  tr t^H t = tr[B_R P_M B_L P_M^H] = T
    `hestenes`                                        one-sided Jacobi on the columns of t when r_L <= r_R, on those of t^H
                                                      otherwise: the matrix with the fewer columns that are not exactly zero, so
                                                      that N - min(r_R, r_L) columns start as zeros and are never rotated
    T_n = the squared column norms, descending        the entries beyond min(r_R, r_L) are exactly 0.0

The Jacobi (`hestenes`): the columns are padded with zeros to NP = 16, 32 or 64 (the kernel's templates; the next even number above
64).  A sweep is NP - 1 rounds of NP / 2 disjoint pairs in the round-robin order of `round_pairs`.  For a pair p < q with
a = |t_p|^2, b = |t_q|^2, c = t_p^H t_q the pair is skipped when a == 0, b == 0 or not |c| > N u sqrt(a) sqrt(b) (a product of
square roots: a b underflows for tunnelling channels); otherwise

    zeta = (b - a) / (2 |c|),  tau = sign(zeta) / (|zeta| + sqrt(1 + zeta^2))  (sign(0) = 1),  cs = 1 / sqrt(1 + tau^2),  sn = cs tau
    w = sn c / |c|;     t_p' = cs t_p - conj(w) t_q,     t_q' = w t_p + cs t_q          |c| = hypot(Re c, Im c)

which makes the two columns orthogonal.  The iteration stops after the first sweep without a rotation; MAX_SWEEPS sweeps that all
rotate raise numpy.linalg.LinAlgError.

One-sided Jacobi on t, not an eigensolve of t^H t: small T_n keep a relative accuracy instead of drowning in u T_max.

`channels_dense` is an independent route -- eigvalsh of Gamma_L^(1/2) P^H Gamma_R P Gamma_L^(1/2), the root from eigh, P and the
self-energies from the dense inverse of `transport_model.transmission_dense` -- and `channels_mp` the same in mpmath on the sweep of
`transport_model.transmission_mp` (N <= 17).  `python tools/channels_model.py` prints the sweep counts and bounds of every GPU input;
`--golden` writes tests/golden/channels_mp.npz.  Design tooling: nothing in the product imports it.
"""

import numpy as np

import ensemble_model as em
import surface_model as sm
import transport_model as tm

U_ROUND = tm.U_ROUND
MAX_ITERATIONS = tm.MAX_ITERATIONS
#: the kernel's cap of the Jacobi sweeps (CHAN_MAX_SWEEPS of csrc/tbk_channels.hip): at least twice the largest count of `gpu_inputs`
MAX_SWEEPS = 48


def pivoted_cholesky(B):
    """(L, perm, rank) of a Hermitian positive semidefinite B [N][N]: B = L L^H up to rounding and the part dropped at `rank`.
    perm[j], j < rank, is the pivot of step j and the column of L that step wrote; the columns of L that no step took are exactly
    zero, and so is row perm[j] in the columns of later steps."""
    A = np.array(B, dtype=np.complex128)
    N = A.shape[0]
    L = np.zeros((N, N), dtype=np.complex128)
    perm = np.full(N, -1, dtype=np.int64)
    taken = np.zeros(N, dtype=bool)
    rank = 0
    threshold = 0.0
    for j in range(N):
        d = A.real.diagonal().copy()
        d[np.isnan(d)] = np.inf
        d[taken] = -np.inf
        p = int(np.argmax(d))  # (the first of equal maxima: the lowest index)
        if j == 0:
            threshold = N * U_ROUND * d[p]
        if d[p] <= threshold:
            break
        root = np.sqrt(d[p])
        with np.errstate(all="ignore"):
            col = A[:, p] * (1.0 / root)  # (one reciprocal per step, as the kernel)
        col[taken] = 0.0
        col[p] = root
        L[:, p] = col
        taken[p] = True
        perm[j] = p
        rank = j + 1
        rest = ~taken
        with np.errstate(all="ignore"):
            A[np.ix_(rest, rest)] -= np.outer(col[rest], col[rest].conj())
    return L, perm, rank


def padded_size(N):
    """The number of columns the Jacobi runs on: the kernel's NP up to 64 rows, the next even number above."""
    for NP in (16, 32, 64):
        if N <= NP:
            return NP
    return N + (N & 1)


def round_pairs(NP, r):
    """(p [NP / 2], q [NP / 2]), p < q: the pairs of round r = 0 ... NP - 2 of the round-robin order.  Pair 0 is (r, NP - 1), pair
    j >= 1 is ((r + j) mod (NP - 1), (r - j) mod (NP - 1)); a sweep meets every pair once."""
    j = np.arange(1, NP // 2)
    u = np.concatenate(([r], (r + j) % (NP - 1)))
    v = np.concatenate(([NP - 1], (r - j) % (NP - 1)))
    return np.minimum(u, v), np.maximum(u, v)


def hestenes(t, *, max_sweeps=MAX_SWEEPS):
    """(squared singular values [N] descending, sweeps) of t [N][N] by the one-sided Jacobi of the module's docstring."""
    t = np.asarray(t, dtype=np.complex128)
    N = t.shape[1]
    NP = padded_size(N)
    W = np.zeros((t.shape[0], NP), dtype=np.complex128)
    W[:, :N] = t
    limit = N * U_ROUND
    sweeps = 0
    while True:
        if sweeps >= max_sweeps:
            raise np.linalg.LinAlgError("the channel iteration did not converge in %d sweeps" % max_sweeps)
        sweeps += 1
        rotations = 0
        for r in range(NP - 1):
            p, q = round_pairs(NP, r)
            x, y = W[:, p], W[:, q]
            a = (x.real * x.real + x.imag * x.imag).sum(axis=0)
            b = (y.real * y.real + y.imag * y.imag).sum(axis=0)
            cr = (x.real * y.real + x.imag * y.imag).sum(axis=0)
            ci = (x.real * y.imag - x.imag * y.real).sum(axis=0)
            size = np.hypot(cr, ci)
            with np.errstate(all="ignore"):
                go = (a != 0.0) & (b != 0.0) & (size > limit * np.sqrt(a) * np.sqrt(b))
                zeta = (b - a) / (2.0 * size)
                tau = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + tau * tau)
                sn = cs * tau
                w = sn * (cr / size) + 1j * (sn * (ci / size))
                new_x = cs * x - np.conj(w) * y
                new_y = w * x + cs * y
            W[:, p] = np.where(go, new_x, x)
            W[:, q] = np.where(go, new_y, y)
            rotations += int(np.count_nonzero(go))
        if rotations == 0:
            break
    values = (W.real * W.real + W.imag * W.imag).sum(axis=0)
    return np.sort(values[:N], kind="stable")[::-1].copy(), sweeps


def _factors(es, et, z):
    sign = 1.0 if np.imag(z) > 0 else -1.0
    B_R = sign * tm._broadening(es)  # pylint: disable=protected-access
    B_L = sign * tm._broadening(et)  # pylint: disable=protected-access
    return pivoted_cholesky(B_R), pivoted_cholesky(B_L)


def channels_of(es, et, P, z, *, max_sweeps=MAX_SWEEPS):
    """(T_n [N] descending, sweeps, (r_R, r_L)) from the lead terms and P_M of one (kp, z, sample): steps 1 to 5."""
    (L_R, _, r_R), (L_L, _, r_L) = _factors(es, et, z)
    with np.errstate(all="ignore"):
        t = L_R.conj().T @ (P @ L_L)
    values, sweeps = hestenes(t if r_L <= r_R else t.conj().T, max_sweeps=max_sweeps)
    return values, sweeps, (r_R, r_L)


def channels(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS, max_sweeps=MAX_SWEEPS):
    """(T_n [N], T, iterations, rho, P_M, sweeps, (r_R, r_L)) of one (kp, z): `transport_model.transmission` and steps 1 to 5 on its
    lead terms and P_M."""
    T, P, iterations, rho = tm.transmission(H00, H01, V, z, max_iterations=max_iterations)
    es, et, _, _ = tm.lead_terms(H00, H01, z, max_iterations=max_iterations)
    values, sweeps, ranks = channels_of(es, et, P, z, max_sweeps=max_sweeps)
    return values, T, iterations, rho, P, sweeps, ranks


def noise(values):
    """sum_n T_n (1 - T_n) along the last axis."""
    values = np.asarray(values, dtype=np.float64)
    return (values * (1.0 - values)).sum(axis=-1)


def _root(gamma):
    w, U = np.linalg.eigh((gamma + gamma.conj().T) / 2)
    return (U * np.sqrt(np.clip(w, 0.0, None))) @ U.conj().T


def channels_dense(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """T_n [N] descending by an independent route: P and the self-energies as in `transport_model.transmission_dense`, the
    eigenvalues of Gamma_L^(1/2) P^H Gamma_R P Gamma_L^(1/2) by eigvalsh."""
    H00 = np.asarray(H00, dtype=np.complex128)
    H01 = np.asarray(H01, dtype=np.complex128)
    _, P, _ = tm.transmission_dense(H00, H01, V, z, max_iterations=max_iterations)
    bottom, top, _, _, _ = sm.decimate(H00, H01, z, max_iterations=max_iterations)
    sign = 1.0 if np.imag(z) > 0 else -1.0
    sigma_r = H01 @ bottom @ H01.conj().T
    sigma_l = H01.conj().T @ top @ H01
    gamma_r = sign * 1j * (sigma_r - sigma_r.conj().T)
    gamma_l = sign * 1j * (sigma_l - sigma_l.conj().T)
    half = _root(gamma_l)
    inner = half @ P.conj().T @ gamma_r @ P @ half
    return np.linalg.eigvalsh((inner + inner.conj().T) / 2)[::-1].copy()


def channels_mp(H00, H01, V, z, *, digits=60):
    """T_n [N] descending as floats from the decimation and the sweep of `transport_model.transmission_mp` in mpmath at `digits`
    digits and the Hermitian eigenvalues of Gamma_L^(1/2) P^H Gamma_R P Gamma_L^(1/2) (N <= 17: mpmath's matrices are slow)."""
    import mpmath  # pylint: disable=import-outside-toplevel

    N = np.shape(H00)[0]
    V = tm._device_argument(V, N)  # pylint: disable=protected-access
    M = V.shape[0]
    with mpmath.workdps(digits):
        def lift(a):
            a = np.asarray(a, dtype=np.complex128)
            return mpmath.matrix([[mpmath.mpc(float(x.real), float(x.imag)) for x in row] for row in a])

        zz = mpmath.mpc(float(np.real(z)), float(np.imag(z))) * mpmath.eye(N)
        h00 = lift(H00)
        es, et, e = lift(H00), lift(H00), lift(H00)
        alpha = lift(H01)
        beta = alpha.H
        h01, h10 = alpha.copy(), beta.copy()
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
        D = et + lift(V[0])
        P = None
        for p in range(M):
            if p == M - 1:
                D = D + (es - h00)
            g = mpmath.inverse(zz - D)
            P = g if p == 0 else g * (h10 * P)
            if p < M - 1:
                D = h00 + lift(V[p + 1]) + h10 * (g * h01)
        sign = 1 if np.imag(z) > 0 else -1
        gamma_r = sign * mpmath.mpc(0, 1) * (es - es.H)
        gamma_l = sign * mpmath.mpc(0, 1) * (et - et.H)
        w, U = mpmath.eighe((gamma_l + gamma_l.H) / 2)
        root = mpmath.diag([mpmath.sqrt(x) if x > 0 else mpmath.mpf(0) for x in w])
        half = U * root * U.H
        inner = half * P.H * gamma_r * P * half
        values = mpmath.eighe((inner + inner.H) / 2, eigvals_only=True)
        return np.array(sorted((float(x) for x in values), reverse=True))


def tolerance(H00, H01, V, z, iterations, rho, P, sweeps, *, max_iterations=MAX_ITERATIONS):
    """The bound on |T_n - exact| of every sorted T_n of one (kp, z), DESIGN.md 26.4.  With sigma2 = `transport_model.scale` / N, the
    bound on |t|_2^2, and eps = `transport_model.relative_error` it is the sum of
        4 eps sigma2                            Weyl: T_n are the eigenvalues of K^(1/2) Gamma K^(1/2) for either Gamma, K the rest of
                                                the product, so each of the four factors (two Gamma, P_M twice) moves them by eps sigma2
        2 (N + 1)^2 u sigma2                    the Cholesky factors: a backward error (N + 1) u |B| and the part dropped at the rank, a
                                                semidefinite remainder of trace <= N (N u d0), for each of the two B
        (8 N (sweeps + 2) + N^2) u sigma2       the Jacobi: 8 N u per sweep and for each of the two products of t, and the pairs left
                                                with |c| <= N u sqrt(a b), an off-diagonal part of the Gram matrix of norm <= N^2 u sigma2
    """
    N = np.shape(H00)[0]
    sigma2 = tm.scale(H00, H01, z, P, max_iterations=max_iterations) / N
    eps = tm.relative_error(H00, H01, V, z, iterations, rho)
    return float((4.0 * eps + (2.0 * (N + 1) ** 2 + 8.0 * N * (sweeps + 2) + N * N) * U_ROUND) * sigma2)


#: (n, L, M) of tests/test_gpu_channels.py: `transport_model.GPU_CASES` without N = 65 -- N = 1, 3, 16, 17, 32, 33, 64 (twice)
GPU_CASES = [case for case in tm.GPU_CASES if case[0] * case[1] <= 64]
GPU_Z = tm.GPU_Z
GPU_NK = tm.GPU_NK
GPU_S = em.GPU_S
#: (n, L, M) of the sample-grouping test: N = 3, 17, 33
GROUP_CASES = [(3, 1, 2), (17, 1, 2), (11, 3, 2)]
#: N of the rank-deficient inputs
DEFICIENT_N = (3, 17)
DEFICIENT_SHAPES = ("cross", "row", "column")

gpu_case = tm.gpu_case


def group_case(n, L, M):
    """(H00, H01 [3][N][N], onsite [S][M][N], matrices [S][M][N][N]) of the sample-grouping test: the leads of `gpu_case`,
    `ensemble_model.gpu_case`'s on-site energies and random Hermitian devices."""
    H00, H01, onsite = em.gpu_case(n, L, M)
    matrices = np.stack([tm.random_device(n * L, M, 9600 + 37 * n + s) for s in range(GPU_S)])
    return H00, H01, onsite, matrices


def deficient_case(N, shape):
    """(H00, H01 [3][N][N], V [2][N][N]): a 3-row crystal whose H01 has non-zero entries in row 0 and column 0 (shape "cross"), in
    row 0 alone (shape "row") or in column 0 alone (shape "column"), embedded for N > 3 in N rows whose other N - 3 have no hopping
    along the axis at all: those rows and columns of both broadenings are exactly zero, so at least N - 3 trailing T_n are exactly
    0.0 whatever the rounding.  The cross gives both broadenings rank 2 of 3 in exact arithmetic; in floating point each of r_R, r_L is
    2 or 3 as the last remaining diagonal, a rounding residue, falls against the threshold N u d0, and the third T_n is exactly 0.0
    whenever one of them is 2 -- two live columns are rotated beside a zero one, as t or as t^H.  A single row opens one row of the
    right lead's broadening and nothing else, exactly: r_R = 1 whatever the rounding, while r_L -- a rank-one matrix that is full -- is
    1 or 2; a single column is the mirror image.  min(r_R, r_L) = 1 either way."""
    _, h00, h01 = tm.random_case(3, 1, GPU_NK, 9700)
    H00 = np.zeros((GPU_NK, N, N), dtype=np.complex128)
    H01 = np.zeros_like(H00)
    if N > 3:
        _, big, _ = tm.random_case(N, 1, GPU_NK, 9701)
        H00[:] = big
        H00[:, :3, 3:] = 0.0
        H00[:, 3:, :3] = 0.0
    H00[:, :3, :3] = h00
    if shape not in DEFICIENT_SHAPES:
        raise ValueError("shape must be one of %r" % (DEFICIENT_SHAPES,))
    if shape in ("cross", "row"):
        H01[:, 0, :3] = h01[:, 0, :]
    if shape in ("cross", "column"):
        H01[:, :3, 0] = h01[:, :, 0]
    V = tm.random_device(N, 2, 9702)
    return H00, H01, V


def gpu_inputs():
    """(label, H00 [N][N], H01 [N][N], V [M][N][N], z) of every (kp, z, sample) the GPU tests run through the kernel."""
    for n, L, M in GPU_CASES:
        H00, H01, V = gpu_case(n, L, M)
        for k in range(GPU_NK):
            for z in GPU_Z:
                yield "case (%d, %d, %d)" % (n, L, M), H00[k], H01[k], V, complex(z)
    for n, L, M in GROUP_CASES:
        H00, H01, onsite, matrices = group_case(n, L, M)
        for devices in (em.expand(onsite), matrices):
            for s in range(GPU_S):
                for k in range(GPU_NK):
                    for z in GPU_Z:
                        yield "groups (%d, %d, %d)" % (n, L, M), H00[k], H01[k], devices[s], complex(z)
    for N in DEFICIENT_N:
        for shape in DEFICIENT_SHAPES:
            H00, H01, V = deficient_case(N, shape)
            for k in range(GPU_NK):
                for z in GPU_Z:
                    yield "deficient %d %s" % (N, shape), H00[k], H01[k], V, complex(z)


def channels_function(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """(T_n [NK][NZ][N], T [NK][NZ], iterations [NK][NZ], bound [NK][NZ], sweeps [NK][NZ], bound of T [NK][NZ]) from H00, H01
    [NK][N][N] and V [M][N][N]."""
    H00 = np.asarray(H00, dtype=np.complex128)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    n_k, N = H00.shape[0], H00.shape[-1]
    values = np.empty((n_k, len(z), N))
    T = np.empty((n_k, len(z)))
    bound = np.empty((n_k, len(z)))
    bound_t = np.empty((n_k, len(z)))
    its = np.zeros((n_k, len(z)), dtype=np.int32)
    sweeps = np.zeros((n_k, len(z)), dtype=np.int32)
    for k in range(n_k):
        for i, zz in enumerate(z):
            values[k, i], T[k, i], its[k, i], rho, P, sweeps[k, i], _ = channels(H00[k], H01[k], V, complex(zz), max_iterations=max_iterations)
            bound[k, i] = tolerance(H00[k], H01[k], V, complex(zz), its[k, i], rho, P, sweeps[k, i], max_iterations=max_iterations)
            bound_t[k, i] = tm.tolerance(H00[k], H01[k], V, complex(zz), its[k, i], rho, P, max_iterations=max_iterations)
    return values, T, its, bound, sweeps, bound_t


def write_golden(path):
    """T_n of `channels_mp` at 60 digits for the GPU cases with N <= 17, [3][5][N] each."""
    out = {"Z": GPU_Z}
    for n, L, M in GPU_CASES:
        if n * L > 17:
            continue
        H00, H01, V = gpu_case(n, L, M)
        out["Tn_%d_%d_%d" % (n, L, M)] = np.array([[channels_mp(H00[k], H01[k], V, complex(z)) for z in GPU_Z] for k in range(GPU_NK)])
        print("(n, L, M) = (%d, %d, %d) done" % (n, L, M), flush=True)
    np.savez(path, **out)


def main():
    print("every (kp, z, sample) of the GPU tests: the most sweeps, the largest bound, the smallest ranks")
    table = {}
    for label, H00, H01, V, z in gpu_inputs():
        values, _, its, rho, P, sweeps, ranks = channels(H00, H01, V, z)
        bound = tolerance(H00, H01, V, z, its, rho, P, sweeps)
        row = table.setdefault(label, [H00.shape[0], 0, 0.0, H00.shape[0], 0.0])
        row[1] = max(row[1], sweeps)
        row[2] = max(row[2], bound)
        row[3] = min(row[3], min(ranks))
        row[4] = max(row[4], float(np.abs(values - channels_dense(H00, H01, V, z)).max() / bound))
    for label, (N, sweeps, bound, rank, ratio) in table.items():
        print("    %-20s N = %2d  sweeps <= %2d  bound <= %.1e  rank >= %2d  |T_n - dense| <= %.1e bound" % (label, N, sweeps, bound, rank, ratio))
    print("the most sweeps: %d (the cap is %d)" % (max(row[1] for row in table.values()), MAX_SWEEPS))


if __name__ == "__main__":
    import os
    import sys

    if "--golden" in sys.argv:
        write_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "channels_mp.npz"))
    else:
        main()
