#!/usr/bin/env python3
"""
NumPy model of the bond currents of csrc/tbk_device_green.hip's CURRENT instantiation: the device of
tools/device_model.py and, from its blocks F_p = G_{p,1} and C_p = G_{p,M}, the currents of the states injected from each lead, per bond.

Everything in front of the new lines is device_model.device_green, unchanged down to the order of the operations.  Layers are numbered
p = 1 ... M; the device's blocks are H_{p,p+1} = H01, H_{p+1,p} = H01^H and H_pp = H00 + V_p.  Per (kp, z), Im z != 0:

    A^L_{p,q} = (F_p Gamma_L) F_q^H          A^R_{p,q} = (C_p Gamma_R) C_q^H          (brackets = order of the products)
    K^L_p[i][j] = 2 Im(conj(H01[i][j]) A^L_{p,p+1}[i][j])      p = 1 ... M - 1   from orbital i of layer p to orbital j of layer p + 1
    J^L_p[i][j] = 2 Im(conj(H_pp[i][j]) A^L_{p,p}[i][j])       p = 1 ... M       from orbital i to orbital j inside layer p
    K^R, J^R: the same with A^R
    current_left[p][i]  = sum_j K^L_p[i][j]        current_right[p][i] = sum_j K^R_p[i][j]

in e / h per unit energy.  K^L flows towards the right lead (positive totals), K^R towards the left (negative totals).  The kernel
differs from this file only in the summation order inside a product and inside a row sum.

Properties, with the signed eta = Im z (`identities` returns their residuals):
(1) for 1 < p < M: sum K^L_{p-1} - sum K^L_p = 4 pi eta sum_i left[p][i];  sum K^L_{M-1} - T = 4 pi eta sum_i left[M][i].
(2) per orbital, 1 < p < M: sum_i K^L_{p-1}[i][j] - sum_k K^L_p[j][k] - sum_k J^L_p[j][k] = 4 pi eta left[p][j]; R and right the same.
(3) for 1 < p < M: sum K^R_{p-1} - sum K^R_p = 4 pi eta sum_i right[p][i];  -sum K^R_1 - T' = 4 pi eta sum_i right[1][i] with T' = Re
    tr[Gamma_L C_1 Gamma_R C_1^H], which is T only as eta -> 0.
(4) K is exactly 0 where H01 is, J where H_pp is; J is antisymmetric up to rounding.
(5) T, ldos, left, right and iterations are device_green's.  (6) The bits of one (kp, z) depend on nothing else.

`current_dense` is an independent route: the blocks of the dense (M N) x (M N) inverse of transport_model.transmission_dense and
self-energies formed as products.  `current_mp` is the sweep and the new lines in mpmath.

`python tools/current_model.py` prints a small table; `--golden` writes tests/golden/current_mp.npz.  Design tooling: nothing in the
product imports it.
"""

import collections

import numpy as np

import device_model as dm
import surface_model as sm
import transport_model as tm

U_ROUND = sm.U_ROUND
MAX_ITERATIONS = sm.MAX_ITERATIONS

DeviceCurrent = collections.namedtuple("DeviceCurrent", ("T", "ldos", "left", "right", "current_left", "current_right", "inter_left", "inter_right",
                                                         "intra_left", "intra_right", "iterations", "green"))
NAMES = ("current_left", "current_right", "inter_left", "inter_right", "intra_left", "intra_right")


def _bond(H, A):
    """2 Im(conj(H) o A), element by element"""
    return 2.0 * (H.real * A.imag - H.imag * A.real)


def currents_of_blocks(H00, H01, V, F, C, gamma_l, gamma_r):
    """(current_left, current_right [M - 1][N], K^L, K^R [M - 1][N][N], J^L, J^R [M][N][N]) from the blocks F, C [M][N][N] and the
    broadenings, by the lines of the docstring."""
    H00 = np.asarray(H00, dtype=np.complex128)
    H01 = np.asarray(H01, dtype=np.complex128)
    M, N = F.shape[0], F.shape[1]
    inter = [np.zeros((M - 1, N, N)), np.zeros((M - 1, N, N))]
    intra = [np.zeros((M, N, N)), np.zeros((M, N, N))]
    with np.errstate(all="ignore"):
        for side, (B, gamma) in enumerate(((F, gamma_l), (C, gamma_r))):
            for p in range(M):
                X = B[p] @ gamma
                intra[side][p] = _bond(H00 + V[p], X @ B[p].conj().T)
                if p + 1 < M:
                    inter[side][p] = _bond(H01, X @ B[p + 1].conj().T)
    return inter[0].sum(axis=2), inter[1].sum(axis=2), inter[0], inter[1], intra[0], intra[1]


def device_current(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """`DeviceCurrent` of one (kp, z): T, ldos, left, right and iterations of device_model.device_green (its `DeviceGreen` is the field
    `green`), current_left, current_right [M - 1][N], inter_left, inter_right [M - 1][N][N] (K) and intra_left, intra_right [M][N][N]
    (J).  numpy.linalg.LinAlgError as device_green, and when an element of K or J is not finite."""
    r = dm.device_green(H00, H01, V, z, max_iterations=max_iterations)
    N = r.G.shape[1]
    VV = tm._device_argument(V, N)  # pylint: disable=protected-access
    gamma_r, gamma_l = tm._broadening(r.es), tm._broadening(r.et)  # pylint: disable=protected-access
    out = currents_of_blocks(H00, H01, VV, r.F, r.C, gamma_l, gamma_r)
    if not all(np.all(np.isfinite(x)) for x in out):
        raise np.linalg.LinAlgError("Singular matrix")
    return DeviceCurrent(r.T, r.ldos, r.left, r.right, *out, r.iterations, r)


def current_dense(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """The six arrays of `currents_of_blocks` by an independent route: F_p and C_p are the blocks (p, 1) and (p, M) of the dense inverse
    of transport_model.transmission_dense, Gamma = i (Sigma - Sigma^H) of self-energies formed as products of the decimation's surface
    functions."""
    H00 = np.asarray(H00, dtype=np.complex128)
    H01 = np.asarray(H01, dtype=np.complex128)
    N = H00.shape[0]
    VV = tm._device_argument(V, N)  # pylint: disable=protected-access
    _, _, full = tm.transmission_dense(H00, H01, VV, z, max_iterations=max_iterations)
    M = full.shape[0] // N
    blocks = full.reshape(M, N, M, N)
    F = np.array([blocks[p, :, 0, :] for p in range(M)])
    C = np.array([blocks[p, :, M - 1, :] for p in range(M)])
    bottom, top, _, _, _ = sm.decimate(H00, H01, z, max_iterations=max_iterations)
    sigma_r = H01 @ bottom @ H01.conj().T
    sigma_l = H01.conj().T @ top @ H01
    return currents_of_blocks(H00, H01, VV, F, C, 1j * (sigma_l - sigma_l.conj().T), 1j * (sigma_r - sigma_r.conj().T))


def current_mp(H00, H01, V, z, *, digits=60):
    """The six arrays of `currents_of_blocks` as float64 from the decimation, both sweeps and the new lines in mpmath at `digits`
    digits, the sweeps as in device_model.device_mp (N <= 24: mpmath's matrices are slow)."""
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
        G, C = [None] * M, [None] * M
        G[M - 1] = C[M - 1] = g[M - 1]
        for p in range(M - 2, -1, -1):
            X = g[p] * h01
            G[p] = g[p] + (X * G[p + 1]) * (h10 * g[p])
            C[p] = X * C[p + 1]
        F = [Q[p] if p == M - 1 else G[p] if p == 0 else G[p] * (h10 * Q[p - 1]) for p in range(M)]
        hpp = [h00 + lift(V[p]) for p in range(M)]

        def bond(H, A):
            return [[2 * (H[i, j].conjugate() * A[i, j]).imag for j in range(N)] for i in range(N)]

        out = []
        for B, gamma in ((F, gamma_l), (C, gamma_r)):
            X = [B[p] * gamma for p in range(M)]
            inter = [bond(h01, X[p] * B[p + 1].H) for p in range(M - 1)]
            intra = [bond(hpp[p], X[p] * B[p].H) for p in range(M)]
            rows = [[float(sum(row)) for row in k] for k in inter]
            out.append((np.array(rows, dtype=np.float64).reshape(M - 1, N), np.array([[[float(x) for x in row] for row in k] for k in inter]).reshape(M - 1, N, N),
                        np.array([[[float(x) for x in row] for row in k] for k in intra]).reshape(M, N, N)))
        return out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2]


def identities(H00, H01, V, z, result, T_prime=None):
    """The residuals of the properties 1 - 3 of the docstring on `result` (anything with T, left, right and the six arrays), each with
    both sides' difference as it stands: a dict of arrays 'left' [M - 1] (layers 2 ... M), 'right' [M - 1] (layers 1 ... M - 1; the
    entry of layer 1 needs T_prime, else it is left out: [M - 2]), 'orbital_left', 'orbital_right' [M - 2][N] (layers 2 ... M - 1).
    M = 1 has no interface: empty arrays."""
    eta = float(np.imag(z))
    left, right = np.asarray(result.left), np.asarray(result.right)
    M = left.shape[0]
    tot_l = np.asarray(result.inter_left).sum(axis=(1, 2))
    tot_r = np.asarray(result.inter_right).sum(axis=(1, 2))
    res_l = [tot_l[p - 1] - (tot_l[p] if p < M - 1 else result.T) - 4.0 * np.pi * eta * left[p].sum() for p in range(1, M)]
    res_r = [tot_r[p - 1] - tot_r[p] - 4.0 * np.pi * eta * right[p].sum() for p in range(1, M - 1)]
    if T_prime is not None and M > 1:
        res_r.insert(0, -tot_r[0] - T_prime - 4.0 * np.pi * eta * right[0].sum())
    orbital = {}
    for name, K, J, rows in (("orbital_left", result.inter_left, result.intra_left, left), ("orbital_right", result.inter_right, result.intra_right, right)):
        K, J = np.asarray(K), np.asarray(J)
        N = J.shape[1]
        orbital[name] = np.array([K[p - 1].sum(axis=0) - K[p].sum(axis=1) - J[p].sum(axis=1) - 4.0 * np.pi * eta * rows[p] for p in range(1, M - 1)]).reshape(-1, N)
    return {"left": np.array(res_l), "right": np.array(res_r), **orbital}


def t_prime(C1, es, et):
    """T' = Re tr[Gamma_L C_1 Gamma_R C_1^H] of property 3 from the block C_1 = G_{1,M}"""
    gamma_r, gamma_l = tm._broadening(es), tm._broadening(et)  # pylint: disable=protected-access
    return float(np.trace(gamma_l @ C1 @ gamma_r @ C1.conj().T).real)


Tolerance = collections.namedtuple("Tolerance", NAMES + tuple("s_" + name for name in NAMES) + ("device", "t_prime"))


def tolerance(H00, H01, V, z, result):
    """The bounds of one (kp, z) from the model's own run `result` (a `DeviceCurrent`): `Tolerance` with current_left, current_right,
    inter_left, inter_right [M - 1] and intra_left, intra_right [M] (per component of layer p's matrix or row), the scales s_* they are
    relative to (the bound without E c), device_model's `Tolerance` of the same run (`device`) and the bound of property 3's T' = Re
    tr[Gamma_L C_1 Gamma_R C_1^H] formed from a C_1 that carries C's bound: (2 c(C_1) + 2) E N gamma_L gamma_R s(C_1)^2, T's scheme.

    E, c(.), s(.) and gamma_L = 2 |H01|_2^2 |G_top|_2, gamma_R are device_model.tolerance's.  A^L_{p,p+1} = (F_p
    Gamma_L) F_{p+1}^H has the factors F_p, Gamma_L and F_{p+1}, whose errors are counted as if they added, each relative to the product
    of the scales; K multiplies a component of it by an element of H01 and doubles it:

        |K^L_p - exact| <= 2 max|H01| (c(F_p) + c(F_{p+1}) + 1) E s(F_p) s(F_{p+1}) gamma_L
        |J^L_p - exact| <= 2 max|H_pp| (2 c(F_p) + 1) E s(F_p)^2 gamma_L
        K^R, J^R: C and gamma_R;     current_*: N times K's bound (a sum of N components)."""
    H00 = np.asarray(H00, dtype=np.complex128)
    H01 = np.asarray(H01, dtype=np.complex128)
    g = result.green
    N, M = g.G.shape[1], g.G.shape[0]
    VV = tm._device_argument(V, N)  # pylint: disable=protected-access
    base = dm.tolerance(H00, H01, VV, z, g)
    E = tm.relative_error(H00, H01, VV, z, g.iterations, g.rho)
    norm = lambda a: float(np.linalg.norm(a, 2))  # noqa: E731
    one = np.eye(N)
    b2 = norm(H01) ** 2
    gamma_l = 2.0 * b2 * norm(np.linalg.inv(z * one - g.et))
    gamma_r = 2.0 * b2 * norm(np.linalg.inv(z * one - g.es))
    layer = np.arange(1, M + 1, dtype=float)
    cG = 3.0 * (M - layer) + 1.0
    cC = (M - layer) + 1.0
    cF = cG + layer - 1.0  # (layer 1: c(G_1))
    cF[M - 1] = float(M)
    h01 = float(np.abs(H01).max())
    hpp = np.array([float(np.abs(H00 + VV[p]).max()) for p in range(M)])
    out, scales = {}, {}
    for side, s, c, gamma in (("left", base.sF, cF, gamma_l), ("right", base.sC, cC, gamma_r)):
        sK = 2.0 * h01 * s[:-1] * s[1:] * gamma
        sJ = 2.0 * hpp * s ** 2 * gamma
        scales["inter_" + side], out["inter_" + side] = sK, (c[:-1] + c[1:] + 1.0) * E * sK
        scales["intra_" + side], out["intra_" + side] = sJ, (2.0 * c + 1.0) * E * sJ
        scales["current_" + side], out["current_" + side] = N * sK, N * out["inter_" + side]
    bound_t = (2.0 * cC[0] + 2.0) * E * N * gamma_l * gamma_r * base.sC[0] ** 2
    return Tolerance(*[out[name] for name in NAMES], *[scales[name] for name in NAMES], base, float(bound_t))


def identity_bounds(z, tol, N):
    """The bounds of `identities`' residuals on outputs that carry the bounds `tol`: the sum of the bounds of the terms that enter each.
    A total over a matrix of K is N^2 components, sum_i left[p][i] N rows; T and T' carry their own.  A dict as `identities`', with
    'right' [M - 1] from layer 1 on (M > 1)."""
    eta = abs(float(np.imag(z)))
    d = tol.device
    M = d.left.shape[0]
    four = 4.0 * np.pi * eta
    kl, kr = N * N * tol.inter_left, N * N * tol.inter_right
    left = np.array([kl[p - 1] + (kl[p] if p < M - 1 else d.T) + four * N * d.left[p] for p in range(1, M)])
    right = [kr[p - 1] + kr[p] + four * N * d.right[p] for p in range(1, M - 1)]
    if M > 1:
        right.insert(0, kr[0] + tol.t_prime + four * N * d.right[0])
    right = np.array(right)
    orb_l = np.array([N * tol.inter_left[p - 1] + N * tol.inter_left[p] + N * tol.intra_left[p] + four * d.left[p] for p in range(1, M - 1)])
    orb_r = np.array([N * tol.inter_right[p - 1] + N * tol.inter_right[p] + N * tol.intra_right[p] + four * d.right[p] for p in range(1, M - 1)])
    wide = lambda a: np.repeat(a.reshape(-1, 1), N, axis=1)  # noqa: E731  (per layer, the same for every orbital)
    return {"left": left, "right": right, "orbital_left": wide(orb_l), "orbital_right": wide(orb_r)}


#: (n, L, M) of tests/test_gpu_device_current.py: N = 1, 3, 16, 17, 32, 33 and 64; M = 1: no interface, only J; (5, 1, 6): every stack
#: place is used again.  (8, 8, 3) stands where device_model's list has (16, 4, 3): there current_left's bound, N times K's, is 1.4e-4,
#: above the ceiling of 1e-4 the tests assert; at (8, 8, 3), also 64 rows and three layers, the largest bound is 3.7e-5.
GPU_CASES = [(1, 1, 1), (1, 1, 3), (3, 1, 2), (8, 2, 3), (17, 1, 2), (8, 4, 2), (11, 3, 2), (8, 8, 3), (64, 1, 1), (64, 1, 2), (5, 1, 6)]
GPU_Z = tm.GPU_Z
GPU_NK = tm.GPU_NK
gpu_case = tm.gpu_case


def device_current_function(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """[NK][NZ] lists of `DeviceCurrent` and of `Tolerance` from H00, H01 [NK][N][N] and V [M][N][N]."""
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    results, bounds = [], []
    for k in range(np.shape(H00)[0]):
        results.append([device_current(H00[k], H01[k], V, complex(zz), max_iterations=max_iterations) for zz in z])
        bounds.append([tolerance(H00[k], H01[k], V, complex(zz), r) for zz, r in zip(z, results[-1])])
    return results, bounds


stack = dm.stack


def write_golden(path):
    """The six arrays of `current_mp` at 60 digits for the GPU cases with N <= 17, [3][5][...] each."""
    out = {"Z": GPU_Z}
    for n, L, M in GPU_CASES:
        if n * L > 17:
            continue
        H00, H01, V = gpu_case(n, L, M)
        rows = [[current_mp(H00[k], H01[k], V, complex(z)) for z in GPU_Z] for k in range(GPU_NK)]
        tag = "_%d_%d_%d" % (n, L, M)
        for index, name in enumerate(NAMES):
            out[name + tag] = np.array([[x[index] for x in row] for row in rows])
        print("(n, L, M) = (%d, %d, %d) done" % (n, L, M), flush=True)
    np.savez(path, **out)


def main():
    print("the GPU cases: the model against the dense inverse, the largest bound and the identities' residuals")
    for n, L, M in GPU_CASES:
        if n * L > 33:
            continue
        H00, H01, V = gpu_case(n, L, M)
        worst, bound, resid = 0.0, 0.0, 0.0
        for z in GPU_Z:
            r = device_current(H00[0], H01[0], V, complex(z))
            tol = tolerance(H00[0], H01[0], V, complex(z), r)
            dense = current_dense(H00[0], H01[0], V, complex(z))
            for index, name in enumerate(NAMES):
                if getattr(r, name).size:
                    worst = max(worst, float(np.abs(getattr(r, name) - dense[index]).max()))
                    bound = max(bound, float(getattr(tol, name).max()))
            res = identities(H00[0], H01[0], V, complex(z), r, t_prime(r.green.C[0], r.green.es, r.green.et))
            resid = max([resid] + [float(np.abs(x).max()) for x in res.values() if x.size])
        print("    (n, L, M) = (%2d, %d, %d): max|model - dense| = %.2e, largest bound %.2e, largest residual of the identities %.2e" % (n, L, M, worst, bound, resid))


if __name__ == "__main__":
    import os
    import sys

    if "--golden" in sys.argv:
        write_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "current_mp.npz"))
    else:
        main()
