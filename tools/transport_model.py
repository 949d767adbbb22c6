#!/usr/bin/env python3
"""
NumPy model of the Landauer transmission of csrc/tbk_surface.hip: a device of M principal layers between two
semi-infinite leads of the crystal, the leads by the decimation of tools/surface_model.py, the device by a recursive sweep.

H00, H01, N and the decimation with its stopping rule are those of surface_model.  The device is the principal layers p = 1 ... M with
on-site blocks H00 + V_p (V_p Hermitian, N x N, ordered in blocks as H00), H01 between neighbouring layers and towards both leads;
the left lead is the crystal on the layers P <= 0, the right lead on P >= M + 1.  Per (kp, z), Im z != 0:

    es, et, iterations      `surface_model.decimate_terms`: the loop of the decimation, without the closing inversions
    Sigma_R = es - H00  (= H01 G_bottom H01^H)          Sigma_L = et - H00  (= H01^H G_top H01)
    Gamma_R = i (es - es^H)                             Gamma_L = i (et - et^H)            (H00 is Hermitian and drops out)

    D_1 = et + V_1
    for p = 1 ... M:   if p = M:  D_p = D_p + (es - H00)
                       g_p = (z - D_p)^-1                               `surface_model._invert`: the kernel's elimination
                       P_p = g_p                      (p = 1)
                       P_p = g_p (H01^H P_{p-1})      (p > 1)           P_p = G_{p,1} of the left-connected system
                       D_{p+1} = (H00 + V_{p+1}) + H01^H (g_p H01)      (p < M)
    T = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)] = Re sum_ij (Gamma_R P_M)[i][j] (Gamma_L P_M^H)[j][i]

P_M is block (M, 1) of the resolvent of the device with both lead self-energies attached.  The order of the operations is part of
the definition: products as bracketed, sums left to right, es - H00 formed before it is added.

`transmission_dense` is an independent route: the dense (M N) x (M N) inverse with the self-energies formed as products from G_bottom
and G_top.  `transmission_mp` is the same sweep in mpmath.  `chain_closed_form` is the chain with one impurity, exact at any eta.
`channels` counts the right-moving bands of the pristine crystal: T at eta -> 0 without a device potential.

`python tools/transport_model.py` prints a small table.  Design tooling: nothing in the product imports it.
"""

import numpy as np

import surface_model as sm

U_ROUND = sm.U_ROUND
MAX_ITERATIONS = sm.MAX_ITERATIONS
random_case = sm.random_case


def lead_terms(H00, H01, z, *, max_iterations=MAX_ITERATIONS):
    """(es, et, iterations, rho) of one (kp, z): H00 plus the self-energy of the right (es) and of the left (et) lead."""
    if H01 is None:
        raise ValueError("the transmission needs hopping between the principal layers (H01 is None)")
    es, et, _, iterations, rho = sm.decimate_terms(H00, H01, z, max_iterations=max_iterations)
    return es, et, iterations, rho


def _device_argument(V, N):
    V = np.asarray(V, dtype=np.complex128)
    if V.ndim != 3 or V.shape[0] < 1 or V.shape[1:] != (N, N):
        raise ValueError("V must have shape (M, %d, %d) with M >= 1, got %r" % (N, N, V.shape))
    return V


def _broadening(e):
    """i (e - e^H), element by element."""
    return 1j * (e - e.conj().T)


def _trace_of_product(a, b):
    """Re sum_ij a[i][j] b[j][i]"""
    return float((a.real * b.real.T - a.imag * b.imag.T).sum())


def transmission(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """(T, P_M, iterations, rho) of one (kp, z) by the sweep of the module's docstring.  V: [M][N][N].  rho: the largest growth
    factor of all inversions.  numpy.linalg.LinAlgError when the cap is reached or an inversion is singular."""
    H00 = np.asarray(H00, dtype=np.complex128)
    N = H00.shape[0]
    V = _device_argument(V, N)
    M = V.shape[0]
    es, et, iterations, rho = lead_terms(H00, H01, z, max_iterations=max_iterations)
    H01 = np.asarray(H01, dtype=np.complex128)
    H10 = H01.conj().T.copy()
    one = np.eye(N)
    D = et + V[0]
    P = None
    for p in range(M):
        if p == M - 1:
            D = D + (es - H00)
        g, growth = sm._invert(z * one - D)  # pylint: disable=protected-access
        rho = max(rho, growth)
        with np.errstate(all="ignore"):
            P = g if p == 0 else g @ (H10 @ P)
            if p < M - 1:
                D = (H00 + V[p + 1]) + H10 @ (g @ H01)
    if not np.all(np.isfinite(P.view(float))):
        raise np.linalg.LinAlgError("Singular matrix")
    a = _broadening(es) @ P
    b = _broadening(et) @ P.conj().T
    return _trace_of_product(a, b), P, iterations, rho


def device_hamiltonian(H00, H01, V):
    """The (M N) x (M N) block-tridiagonal matrix of the isolated device."""
    H00 = np.asarray(H00, dtype=np.complex128)
    N = H00.shape[0]
    V = _device_argument(V, N)
    M = V.shape[0]
    H = np.zeros((M * N, M * N), dtype=np.complex128)
    for p in range(M):
        H[p * N:(p + 1) * N, p * N:(p + 1) * N] = H00 + V[p]
        if p + 1 < M:
            H[p * N:(p + 1) * N, (p + 1) * N:(p + 2) * N] = H01
            H[(p + 1) * N:(p + 2) * N, p * N:(p + 1) * N] = np.conj(H01).T
    return H


def transmission_dense(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """(T, P_M, G) from the dense inverse G of z - H_device - Sigma, with Sigma_R = H01 G_bottom H01^H on the last and Sigma_L =
    H01^H G_top H01 on the first block formed as products, and T = Re tr[Gamma_R G_{M1} Gamma_L G_{M1}^H]."""
    H00 = np.asarray(H00, dtype=np.complex128)
    H01 = np.asarray(H01, dtype=np.complex128)
    N = H00.shape[0]
    H = device_hamiltonian(H00, H01, V)
    M = H.shape[0] // N
    bottom, top, _, _, _ = sm.decimate(H00, H01, z, max_iterations=max_iterations)
    sigma_r = H01 @ bottom @ H01.conj().T
    sigma_l = H01.conj().T @ top @ H01
    A = z * np.eye(M * N) - H
    A[:N, :N] -= sigma_l
    A[-N:, -N:] -= sigma_r
    G = np.linalg.inv(A)
    P = G[-N:, :N]
    gamma_r = 1j * (sigma_r - sigma_r.conj().T)
    gamma_l = 1j * (sigma_l - sigma_l.conj().T)
    T = float(np.trace(gamma_r @ P @ gamma_l @ P.conj().T).real)
    return T, P.copy(), G


def transmission_mp(H00, H01, V, z, *, digits=60):
    """(T, P_M) as a float and a complex128 array from the same decimation and sweep in mpmath at `digits` digits, the decimation
    run as in `surface_model.decimate_mp` (N <= 24: mpmath's matrices are slow)."""
    import mpmath  # pylint: disable=import-outside-toplevel

    N = np.shape(H00)[0]
    V = _device_argument(V, N)
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
        gamma_r = mpmath.mpc(0, 1) * (es - es.H)
        gamma_l = mpmath.mpc(0, 1) * (et - et.H)
        a = gamma_r * P
        b = gamma_l * P.H
        total = mpmath.mpf(0)
        for i in range(N):
            for j in range(N):
                total += (a[i, j] * b[j, i]).real
        return float(total), np.array([[complex(P[i, j]) for j in range(N)] for i in range(N)])


def chain_closed_form(z, t, t_plane, kpar, eps):
    """T of the chain of `surface_model.chain_closed_form` with one impurity eps on one site (M = 1, V_1 = eps): with g_s the surface
    function of the clean half chain, G = 1 / (zeta - eps - 2 t^2 g_s), Gamma = -2 t^2 Im g_s, T = Gamma^2 |G|^2.  Exact at any eta."""
    g_s, _ = sm.chain_closed_form(z, t, t_plane, kpar)
    zeta = z - 2.0 * t_plane * np.cos(2.0 * np.pi * kpar)
    G = 1.0 / (zeta - eps - 2.0 * t * t * g_s)
    gamma = -2.0 * t * t * g_s.imag
    return float(gamma * gamma * abs(G) ** 2)


def channels(layers, E, *, grid=4096):
    """The number of right-moving bands of H(k_a) = sum_m H_m exp(2 pi i m k_a) at the energy E (layers: H_m [2 L + 1][n][n], index
    m + L): the upward crossings of E by the sorted bands on a periodic grid of `grid` points."""
    layers = np.asarray(layers, dtype=np.complex128)
    L = (layers.shape[0] - 1) // 2
    ka = np.arange(grid) / float(grid)
    phase = np.exp(2j * np.pi * np.arange(-L, L + 1)[None, :] * ka[:, None])  # [grid][2 L + 1]
    bands = np.linalg.eigvalsh(np.einsum("gm,mij->gij", phase, layers)) - E    # [grid][n], ascending
    below = bands < 0.0
    return int(np.count_nonzero(below & ~np.roll(below, -1, axis=0)))


def scale(H00, H01, z, P, *, max_iterations=MAX_ITERATIONS):
    """N (2 |H01|^2 |G_bottom|) (2 |H01|^2 |G_top|) |P_M|^2 in 2-norms: the size of the terms T is a trace of."""
    H00 = np.asarray(H00, dtype=np.complex128)
    bottom, top, _, _, _ = sm.decimate(H00, H01, z, max_iterations=max_iterations)
    b2 = np.linalg.norm(np.asarray(H01), 2) ** 2
    return float(H00.shape[0] * (2.0 * b2 * np.linalg.norm(bottom, 2)) * (2.0 * b2 * np.linalg.norm(top, 2)) * np.linalg.norm(P, 2) ** 2)


def relative_error(H00, H01, V, z, iterations, rho):
    """eps_rel = 8 N u rho (|z| + |H00|_2 + 2 |H01|_2 + max_p |V_p|_2) / eta (iterations + M + 1): the normwise relative error of
    each of the four error-carrying factors of T (two broadenings, P_M twice).  One inversion errs by 8 N u rho kappa_2 relative to
    its result, kappa_2(z - D) <= (|z| + |D|_2) / eta for a causal D, and the iterations + M + 1 inversions behind a factor are
    counted as if their errors added."""
    H00 = np.asarray(H00, dtype=np.complex128)
    V = _device_argument(V, H00.shape[0])
    N, M = H00.shape[0], V.shape[0]
    size = np.linalg.norm(H00, 2) + 2.0 * np.linalg.norm(np.asarray(H01), 2) + max(np.linalg.norm(v, 2) for v in V)
    return 8.0 * N * U_ROUND * rho * (abs(z) + size) / abs(np.imag(z)) * (iterations + M + 1.0)


def tolerance(H00, H01, V, z, iterations, rho, P, *, max_iterations=MAX_ITERATIONS):
    """4 eps_rel scale: the bound on |T - exact| of one (kp, z), from the model's iterations, rho and P_M.  |tr X| <= N |X|_2."""
    return 4.0 * relative_error(H00, H01, V, z, iterations, rho) * scale(H00, H01, z, P, max_iterations=max_iterations)


def green_tolerance(H00, H01, V, z, iterations, rho):
    """The bound per component of P_M: `surface_model.tolerance` with iterations + M + 1 inversions in place of iterations + 1."""
    M = np.shape(V)[0]
    return float(sm.tolerance(np.asarray(H00)[None], np.asarray(H01)[None], z, iterations + M, rho)[0, 0])


def random_device(N, M, seed, *, norm=0.5):
    """V [M][N][N]: random Hermitian matrices of 2-norm `norm`."""
    rng = np.random.default_rng(seed)
    V = np.empty((M, N, N), dtype=np.complex128)
    for p in range(M):
        a = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
        a = (a + a.conj().T) / 2
        V[p] = a * (norm / np.linalg.norm(a, 2))
    return V


#: (n, L, M) of tests/test_gpu_transport.py: N = 1, 3, 16, 17, 32, 33, 64 (twice) and 65
GPU_CASES = [(1, 1, 1), (3, 1, 2), (8, 2, 3), (17, 1, 2), (8, 4, 2), (11, 3, 2), (16, 4, 3), (64, 1, 1), (13, 5, 2)]
GPU_Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])
GPU_NK = 3


def gpu_case(n, L, M):
    """(H00, H01 [3][N][N], V [M][N][N]) of a GPU test case: `random_case` and a random Hermitian device of norm 0.5."""
    _, H00, H01 = random_case(n, L, GPU_NK, 9300 + 37 * n + L)
    return H00, H01, random_device(n * L, M, 9400 + 37 * n + M)


def write_golden(path):
    """T of `transmission_mp` at 60 digits for the GPU cases with N <= 17, [3][5] each: mpmath takes two seconds per (k, z) at 17
    rows, too long for a test that runs with every suite."""
    out = {"Z": GPU_Z}
    for n, L, M in GPU_CASES:
        if n * L > 17:
            continue
        H00, H01, V = gpu_case(n, L, M)
        out["T_%d_%d_%d" % (n, L, M)] = np.array([[transmission_mp(H00[k], H01[k], V, complex(z))[0] for z in GPU_Z] for k in range(GPU_NK)])
        print("(n, L, M) = (%d, %d, %d) done" % (n, L, M))
    np.savez(path, **out)


def transmission_function(H00, H01, V, z, *, max_iterations=MAX_ITERATIONS):
    """(T [NK][NZ], P_M [NK][NZ][N][N], iterations [NK][NZ], rho [NK][NZ]) from H00, H01 [NK][N][N] and V [M][N][N]."""
    H00 = np.asarray(H00, dtype=np.complex128)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    n_k, N = H00.shape[0], H00.shape[-1]
    T = np.empty((n_k, len(z)))
    P = np.empty((n_k, len(z), N, N), dtype=np.complex128)
    its = np.zeros((n_k, len(z)), dtype=np.int32)
    rho = np.ones((n_k, len(z)))
    for k in range(n_k):
        for i, zz in enumerate(z):
            T[k, i], P[k, i], its[k, i], rho[k, i] = transmission(H00[k], H01[k], V, complex(zz), max_iterations=max_iterations)
    return T, P, its, rho


def main():
    t, t_plane, kpar = 1.0, 0.3, 0.17
    full = {(0, 1): np.array([[t]]), (0, -1): np.array([[t]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    H00, H01 = sm.principal(sm.layers_direct(full, 1, [kpar], 1))
    print("the chain with one impurity: t = %g along a, t' = %g in the plane, k = %g" % (t, t_plane, kpar))
    for eps in (0.0, 1.0, 4.0):
        V = np.full((1, 1, 1), eps, dtype=np.complex128)
        for z in (0.4 + 0.5j, 0.4 + 0.05j, 1.9 - 0.05j, 3.0 + 0.05j):
            T, P, its, rho = transmission(H00, H01, V, z)
            print("    eps = %g z = %-14s %2d iterations  T = %.12f  |T - closed| = %.2e  (bound %.2e)"
                  % (eps, z, its, T, abs(T - chain_closed_form(z, t, t_plane, kpar, eps)), tolerance(H00, H01, V, z, its, rho, P)))
    print("pristine crystals at eta = 1e-6: T against the number of right-moving bands")
    for (n, L, seed), M in (((3, 1, 1), 4), ((4, 2, 2), 3), ((6, 1, 3), 1)):
        layers, h00, h01 = random_case(n, L, 1, seed)
        V = np.zeros((M, n * L, n * L), dtype=np.complex128)
        for E in (-0.8, 0.1, 0.9, 3.0):
            T = transmission(h00[0], h01[0], V, E + 1e-6j)[0]
            print("    n = %d L = %d M = %d E = %+.1f: T = %.6f, channels %d" % (n, L, M, E, T, channels(layers[0], E)))


if __name__ == "__main__":
    import os
    import sys

    if "--golden" in sys.argv:
        write_golden(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "transport_mp.npz"))
    else:
        main()
