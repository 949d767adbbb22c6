#!/usr/bin/env python3
"""
NumPy model of the transmission of an ensemble of devices of csrc/tbk_ensemble.hip: S devices between the same
two leads, disorder samples after one decimation.

T[s] is `transport_model.transmission(H00, H01, V_s, z)[0]`, unchanged down to the order of the operations.  The decimation of a
(kp, z) does not depend on V, so `transmission_ensemble` computes the lead terms once and the sweep of `transport_model` per sample:

    es, et, iterations      `transport_model.lead_terms`, once
    for s = 0 ... S - 1:    D_1 = et + V_s1;  the sweep over p = 1 ... M;  T[s] = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)]

The devices are Hermitian matrices [S][M][N][N] or real on-site energies [S][M][N]; `expand` turns the second form into the first,
and the kernel's diagonal form has the bits of the matrix form on the expanded diagonal: it adds the energy on the diagonal and 0.0
elsewhere in the same expressions.  The bound per sample is `transport_model.tolerance`.

`python tools/ensemble_model.py` prints the largest bound of every GPU case.  Design tooling: nothing in the product imports it.
"""

import numpy as np

import surface_model as sm
import transport_model as tm

MAX_ITERATIONS = tm.MAX_ITERATIONS


def expand(onsite):
    """Real on-site energies [...][N] as diagonal matrices [...][N][N], complex128 with exact zeros elsewhere."""
    onsite = np.asarray(onsite)
    if np.iscomplexobj(onsite):
        raise ValueError("on-site energies must be real")
    onsite = np.asarray(onsite, dtype=np.float64)
    N = onsite.shape[-1]
    out = np.zeros(onsite.shape + (N,), dtype=np.complex128)
    index = np.arange(N)
    out[..., index, index] = onsite
    return out


def _devices_argument(devices, N):
    devices = np.asarray(devices)
    if devices.ndim == 3 and devices.shape[0] >= 1 and devices.shape[1] >= 1 and devices.shape[2] == N:
        return expand(devices)
    if devices.ndim == 4 and devices.shape[0] >= 1 and devices.shape[1] >= 1 and devices.shape[2:] == (N, N):
        return np.asarray(devices, dtype=np.complex128)
    raise ValueError("devices must have shape (S, M, %d) or (S, M, %d, %d), got %r" % (N, N, N, devices.shape))


def transmission_ensemble(H00, H01, devices, z, *, max_iterations=MAX_ITERATIONS):
    """(T [S], P_M [S][N][N], iterations, rho [S]) of one (kp, z): the lead terms once, the sweep of `transport_model.transmission`
    per sample.  rho[s]: the largest growth factor of the decimation's inversions and of the sample's."""
    H00 = np.asarray(H00, dtype=np.complex128)
    N = H00.shape[0]
    devices = _devices_argument(devices, N)
    S, M = devices.shape[:2]
    es, et, iterations, rho_leads = tm.lead_terms(H00, H01, z, max_iterations=max_iterations)
    H01 = np.asarray(H01, dtype=np.complex128)
    H10 = H01.conj().T.copy()
    one = np.eye(N)
    gamma_r, gamma_l = tm._broadening(es), tm._broadening(et)  # pylint: disable=protected-access
    T = np.empty(S)
    P_all = np.empty((S, N, N), dtype=np.complex128)
    rho = np.empty(S)
    for s in range(S):
        V = devices[s]
        growth_s = rho_leads
        D = et + V[0]
        P = None
        for p in range(M):
            if p == M - 1:
                D = D + (es - H00)
            g, growth = sm._invert(z * one - D)  # pylint: disable=protected-access
            growth_s = max(growth_s, growth)
            with np.errstate(all="ignore"):
                P = g if p == 0 else g @ (H10 @ P)
                if p < M - 1:
                    D = (H00 + V[p + 1]) + H10 @ (g @ H01)
        if not np.all(np.isfinite(P.view(float))):
            raise np.linalg.LinAlgError("Singular matrix (sample %d)" % s)
        T[s] = tm._trace_of_product(gamma_r @ P, gamma_l @ P.conj().T)  # pylint: disable=protected-access
        P_all[s] = P
        rho[s] = growth_s
    return T, P_all, iterations, rho


def tolerance(H00, H01, devices, z, iterations, rho, P, *, max_iterations=MAX_ITERATIONS):
    """[S]: `transport_model.tolerance` of every sample."""
    devices = _devices_argument(devices, np.shape(H00)[0])
    return np.array([tm.tolerance(H00, H01, devices[s], z, iterations, rho[s], P[s], max_iterations=max_iterations) for s in range(devices.shape[0])])


#: (n, L, M) of tests/test_gpu_ensemble.py: N = 1, 3, 16, 17, 32, 33, 64 (twice) and 65
GPU_CASES = [(1, 1, 1), (3, 1, 2), (8, 2, 3), (17, 1, 2), (8, 4, 2), (11, 3, 2), (16, 4, 3), (64, 1, 2), (13, 5, 2)]
GPU_Z = tm.GPU_Z
GPU_NK = tm.GPU_NK
GPU_S = 5


def gpu_case(n, L, M, S=GPU_S):
    """(H00, H01 [3][N][N], onsite [S][M][N]) of a GPU test case: `transport_model.gpu_case`'s leads and uniform on-site energies in
    [-0.5, 0.5)."""
    _, H00, H01 = tm.random_case(n, L, GPU_NK, 9300 + 37 * n + L)
    onsite = np.random.default_rng(9500 + 37 * n + M).uniform(-0.5, 0.5, (S, M, n * L))
    return H00, H01, onsite


def ensemble_function(H00, H01, devices, z, *, max_iterations=MAX_ITERATIONS):
    """(T [NK][NZ][S], iterations [NK][NZ], bound [NK][NZ][S]) from H00, H01 [NK][N][N] and the devices in either form."""
    H00 = np.asarray(H00, dtype=np.complex128)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    devices = _devices_argument(devices, H00.shape[-1])
    n_k, S = H00.shape[0], devices.shape[0]
    T = np.empty((n_k, len(z), S))
    bound = np.empty((n_k, len(z), S))
    its = np.zeros((n_k, len(z)), dtype=np.int32)
    for k in range(n_k):
        for i, zz in enumerate(z):
            T[k, i], P, its[k, i], rho = transmission_ensemble(H00[k], H01[k], devices, complex(zz), max_iterations=max_iterations)
            bound[k, i] = tolerance(H00[k], H01[k], devices, complex(zz), its[k, i], rho, P, max_iterations=max_iterations)
    return T, its, bound


def main():
    print("the largest bound over samples, points and energies of the GPU cases (S = %d)" % GPU_S)
    for n, L, M in GPU_CASES:
        H00, H01, onsite = gpu_case(n, L, M)
        _, its, bound = ensemble_function(H00, H01, onsite, GPU_Z)
        print("    (n, L, M) = (%2d, %d, %d)  N = %2d  iterations %2d ... %2d  largest bound %.1e" % (n, L, M, n * L, its.min(), its.max(), bound.max()))


if __name__ == "__main__":
    main()
