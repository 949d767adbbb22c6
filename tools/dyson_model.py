#!/usr/bin/env python3
"""
NumPy model of the dressed lattice Green's function of csrc/tbk_green.hip: a local, energy-dependent
self-energy by one general inversion per mesh point and energy.

    A(k, z) = (z 1 - H(k)) - Sigma(z)            H(k) of hamilton(k, convention=2) at k = (i_1 / n_1, ..., i_dim / n_dim)
    P(k, z) = A(k, z)^-1 / NK
    G(R, z) = sum_k exp(-2 pi i sum_d ((i_d R_d) mod n_d) / n_d) P(k, z)             the phases of tools/dm_model.py

`invert` is the elimination green_invert_kernel performs: Gauss-Jordan in place with IMPLICIT partial pivoting, in panels of 16
pivots.  Rows never move.  Step j takes, among the rows no step has taken, the one with the largest |re| + |im| in column j (ties:
the lowest row index) as its pivot row p_j and applies the elementary transformation to the 16 columns of its panel alone: row p_j
becomes a[p][c] / piv (1 / piv in column j), every other row i becomes a[i][c] - a[i][j] (a[p][c] / piv) (-a[i][j] / piv in column
j).  After the panel's steps its columns hold W = T E (T the product of the transformations, E the unit columns of the pivot rows)
and every other column block C -- earlier panels, which hold columns of the inverse, and later ones -- becomes mask(C) + W C[pivot
rows], mask zeroing the panel's pivot rows: the rank-16 update the kernel runs on the matrix pipe.  In the end storage[p_j][c] is
inverse[j][p_c].  1 / piv is conj(piv) / |piv|^2; the result is divided by NK element by element.

`python tools/dyson_model.py` prints a small worked case.  Design tooling: nothing in the product imports it.
"""

import numpy as np

import dm_model

U_ROUND = 2.0 ** -53
PANEL = 16


def _modulus(x):
    """The pivot measure |re| + |im|; a NaN counts as +inf (every lane of the kernel then reaches the same row)."""
    m = np.abs(x.real) + np.abs(x.imag)
    return np.where(np.isnan(m), np.inf, m)


def invert(A, *, panel=PANEL, pivoting=True):
    """(A^-1, rho, pivot rows) by the kernel's elimination.  rho = max over the elimination of |element| / max |A| (|.| the complex
    modulus).  ``pivoting=False`` takes row j at step j (for the test that shows pivoting is needed).  numpy.linalg.LinAlgError for
    a pivot that is exactly zero or a non-finite result."""
    a = np.array(A, dtype=np.complex128)
    n = a.shape[0]
    if a.shape != (n, n):
        raise ValueError("A must be square")
    scale = float(np.abs(a).max()) if n else 0.0
    growth = scale
    used = np.zeros(n, dtype=bool)
    prow = np.full(n, -1)
    jrow = np.full(n, -1)
    for j0 in range(0, n, panel):
        j1 = min(n, j0 + panel)
        cols = slice(j0, j1)
        for j in range(j0, j1):
            if pivoting:
                measure = np.where(used, -1.0, _modulus(a[:, j]))
                p = int(np.argmax(measure))  # (argmax returns the first of equal maxima: the lowest row)
            else:
                p = j
            piv = a[p, j]
            if piv == 0.0:
                raise np.linalg.LinAlgError("Singular matrix")
            with np.errstate(all="ignore"):
                inv = np.conj(piv) / (piv.real * piv.real + piv.imag * piv.imag)
                t = a[p, cols] * inv
                t[j - j0] = inv
                f = a[:, j].copy()
                block = a[:, cols] - f[:, None] * t[None, :]
                block[:, j - j0] = -f * inv
                block[p, :] = t
            a[:, cols] = block
            used[p] = True
            prow[j], jrow[p] = p, j
            growth = max(growth, float(np.abs(np.where(np.isfinite(a), a, 0)).max()))
        # the rank-16 update of the other columns
        others = np.r_[0:j0, j1:n]
        if len(others):
            rows = prow[j0:j1]
            with np.errstate(all="ignore"):
                pivot_rows = a[np.ix_(rows, others)].copy()
                rest = a[:, others].copy()
                rest[rows, :] = 0.0
                a[:, others] = rest + a[:, cols] @ pivot_rows
            growth = max(growth, float(np.abs(np.where(np.isfinite(a), a, 0)).max()))
    inverse = a[np.ix_(prow, jrow)]
    if not np.all(np.isfinite(inverse.view(float))):
        raise np.linalg.LinAlgError("Singular matrix")
    return inverse, (growth / scale if scale > 0 else 1.0), prow


def matrices(H, z, sigma):
    """A[NK][NZ][n][n] = (z 1 - H(k)) - Sigma(z)."""
    H = np.asarray(H, dtype=np.complex128)
    n = H.shape[-1]
    H = H.reshape(-1, n, n)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    sigma = np.asarray(sigma, dtype=np.complex128).reshape(len(z), n, n)
    return (z[None, :, None, None] * np.eye(n)[None, None] - H[:, None]) - sigma[None]


def dressed_green_function(H, mesh, z, sigma, R, *, pivoting=True):
    """(G[NR][NZ][n][n], rho[NK][NZ]) from H(k) [NK][n][n] in mesh order, the energies z [NZ], Sigma [NZ][n][n] and the integer
    vectors R [NR][dim], by `invert`."""
    A = matrices(H, z, sigma)
    n_k, n_z, n = A.shape[0], A.shape[1], A.shape[-1]
    P = np.empty_like(A)
    rho = np.empty((n_k, n_z))
    for k in range(n_k):
        for i in range(n_z):
            inverse, rho[k, i], _ = invert(A[k, i], pivoting=pivoting)
            P[k, i] = inverse / float(n_k)
    G = (dm_model.phases(mesh, R) @ P.reshape(n_k, -1)).reshape(-1, n_z, n, n)
    return G, rho


def direct(H, mesh, z, sigma, R):
    """The same quantity through numpy.linalg.inv."""
    A = matrices(H, z, sigma)
    n_k = A.shape[0]
    return np.einsum("rk,kzij->rzij", dm_model.phases(mesh, R), np.linalg.inv(A)) / float(n_k)


def tolerance(H, z, sigma, rho):
    """The bound per component of G(R, z), one number per energy [NZ]:

        max_k 8 n u rho(k, z) kappa_2(A) ||A^-1||_2  +  4 (NK + 32) u max_k ||A^-1||_2

    The first term is the first-order forward bound of inversion by elimination with partial pivoting (Higham, Accuracy and
    Stability, ch. 14; the complex-arithmetic constant folded into the 8), rho the growth factor of `invert` (a number or an array
    [NK][NZ]); the second the sum over k of NK terms of modulus <= ||A^-1|| / NK with the phase roundings, the form of
    green_model.green_tolerance.  kappa_2 and ||A^-1||_2 come from numpy on the reference A."""
    A = matrices(H, z, sigma)
    n_k, n_z, n = A.shape[0], A.shape[1], A.shape[-1]
    rho = np.broadcast_to(np.asarray(rho, dtype=float), (n_k, n_z))
    sv = np.linalg.svd(A, compute_uv=False)  # [NK][NZ][n], descending
    inv_norm = 1.0 / sv[..., -1]
    kappa = sv[..., 0] * inv_norm
    e_inv = 8.0 * n * U_ROUND * rho * kappa * inv_norm
    return e_inv.max(axis=0) + 4.0 * (n_k + 32) * U_ROUND * inv_norm.max(axis=0)


def causal_case(n, n_k, z, seed, *, spread=1.0):
    """Test inputs: Hermitian H [NK][n][n] with spectrum in [-2, 2] and Sigma(z) = S - i sign(Im z) Gamma with S Hermitian and Gamma
    positive semidefinite, ||Sigma|| <= 1.7 spread -- causal with z (retarded for Im z > 0, advanced for Im z < 0)."""
    rng = np.random.default_rng(seed)
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    q = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
    e = rng.uniform(-2.0, 2.0, (n_k, n))
    H = np.matmul(q * e[:, None, :], np.conj(np.transpose(q, (0, 2, 1))))
    H = (H + np.conj(np.transpose(H, (0, 2, 1)))) / 2
    sigma = np.empty((len(z), n, n), dtype=np.complex128)
    for i, zz in enumerate(z):
        u = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))[0]
        s = (u * rng.uniform(-1.0, 1.0, n)) @ u.conj().T
        v = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))[0]
        gamma = (v * rng.uniform(0.0, 0.7, n)) @ v.conj().T
        s, gamma = (s + s.conj().T) / 2, (gamma + gamma.conj().T) / 2
        sigma[i] = spread * (s - 1j * np.sign(zz.imag) * gamma)
    return np.ascontiguousarray(H), np.ascontiguousarray(sigma)


def main():
    mesh, n = (2, 2), 3
    z = np.array([0.3 + 0.1j, 0.3 - 0.1j])
    H, sigma = causal_case(n, 4, z, 1)
    R = np.array([[0, 0], [1, 0], [-1, 0]])
    G, rho = dressed_green_function(H, mesh, z, sigma, R)
    ref = direct(H, mesh, z, sigma, R)
    bound = tolerance(H, z, sigma, rho)
    print("3 orbitals on the mesh %s, z = %s, growth factor <= %.3f" % (mesh, [complex(x) for x in z], rho.max()))
    for line in G[0, 0]:
        print("    " + "  ".join("%+.6f%+.6fi" % (x.real, x.imag) for x in line))
    print("    max|G - direct| = %.3e (bound %.3e)" % (np.abs(G - ref).max(), bound.max()))


if __name__ == "__main__":
    main()
