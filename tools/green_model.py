#!/usr/bin/env python3
"""
NumPy model of csrc/tbk_green.hip: the lattice Green's function (the resolvent) of a uniform, periodic k mesh at complex energies
(DESIGN.md section 19).

    g[k][b](z)    = 1 / (z - E[k][b])                  dr = Re z - E, di = Im z, g = (dr - i di) / (dr^2 + di^2)
    P(k, z)[i][j] = sum_b (g[k][b](z) / NK) U[k][i][b] conj(U[k][j][b])
    G(R, z)[i][j] = sum_k exp(-2 pi i sum_d ((i_d R_d) mod n_d) / n_d) P(k, z)[i][j]        k = (i_1 / n_1, ..., i_dim / n_dim)

``E, U`` are those of ``eigh(k, convention=2)``; ``U[k][i][b]`` is component i of band b.  The sign is that of the density matrix
(tools/dm_model.py), the inverse of ``hamilton``, and the phase is reduced in integers exactly as there, so ``G(R + n_d e_d, z)``
has the bits of ``G(R, z)``.  Any ``Im z != 0`` of either sign: retarded, advanced, Matsubara or contour points.

`python tools/green_model.py` prints a small worked case.  Design tooling: nothing in the product imports it.
"""

import itertools

import numpy as np

import dm_model

U_ROUND = 2.0 ** -53


def weights(E, z):
    """g[NK][NZ][n] = 1 / (z - E) from the real and imaginary distances (no complex division)."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    z = np.atleast_1d(np.asarray(z, dtype=complex))
    dr = z.real[None, :, None] - E.reshape(-1, 1, n)
    di = np.broadcast_to(z.imag[None, :, None], dr.shape)
    den = dr * dr + di * di
    return (dr - 1j * di) / den


def projectors(E, U, z):
    """P[NK][NZ][n][n] from eigenvalues of shape mesh + (n,) or (NK, n), eigenvectors mesh + (n, n) or (NK, n, n) and energies z."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_u = np.asarray(U).reshape(-1, n, n)
    g = weights(E, z) / float(flat_u.shape[0])
    # (g o U) U^H as one batched matrix product per (k, z)
    return np.matmul(flat_u[:, None, :, :] * g[:, :, None, :], np.conj(np.transpose(flat_u, (0, 2, 1)))[:, None, :, :])


def green_function(E, U, mesh, z, R):
    """G[NR][NZ][n][n] for the integer vectors ``R`` of shape (NR, dim) and the complex energies ``z``."""
    P = projectors(E, U, z)
    return (dm_model.phases(mesh, R) @ P.reshape(P.shape[0], -1)).reshape((-1,) + P.shape[1:])


def green_tolerance(n_k, n, eta):
    """The bound of the kernels against this model on the same (E, U), per component: an element of G is a sum of NK n terms whose
    moduli add up to at most 1 / eta (|g| <= 1 / eta, Cauchy-Schwarz on the unit rows of U); 32 covers the few roundings of g, the
    complex multiplies and sincospi.  eta = min |Im z| of the call.  The density matrix's bound over eta."""
    return 4.0 * (n_k * n + 32) * U_ROUND / float(eta)


def resolvent(ham, mesh, z, R):
    """The same quantity without eigenvectors: G[NR][NZ][n][n] from H(k) [NK][n][n] at the mesh points (mesh order) by
    numpy.linalg.inv(z - H(k)) and the phases of tools/dm_model.py."""
    ham = np.asarray(ham)
    n_k, n = ham.shape[0], ham.shape[-1]
    z = np.atleast_1d(np.asarray(z, dtype=complex))
    inv = np.linalg.inv(z[None, :, None, None] * np.eye(n)[None, None] - ham[:, None])
    return np.einsum("rk,kzij->rzij", dm_model.phases(mesh, R), inv) / float(n_k)


def eigensystem_bound(ham, E, U, eta):
    """max over the mesh of (||U U^H - 1||_2 + ||H U - U E||_2 ||U||_2 / eta) / eta: how far U g U^H of a COMPUTED eigensystem
    is from (z - H)^-1 in the 2-norm, since (z - H) U g U^H = U U^H - (H U - U E) g U^H and ||(z - H)^-1|| <= 1 / eta."""
    worst = 0.0
    for h, e, u in zip(np.asarray(ham), np.asarray(E).reshape(len(ham), -1), np.asarray(U).reshape(np.asarray(ham).shape)):
        unit = np.linalg.norm(u @ u.conj().T - np.eye(len(e)), 2)
        resid = np.linalg.norm(h @ u - u * e[None, :], 2)
        worst = max(worst, (unit + resid * np.linalg.norm(u, 2) / eta) / eta)
    return worst


def whole_call_tolerance(ham, E, U, eta, g_ref):
    """The bound of a whole call against `resolvent`: twice the eigensystem bound (the call's own eigenvectors may come from another
    chunking than E, U), the kernels' bound, and 4 n u ||G_ref|| for the reference's own inverse."""
    n_k, n = np.asarray(ham).shape[0], np.asarray(ham).shape[-1]
    return 2.0 * eigensystem_bound(ham, E, U, eta) + green_tolerance(n_k, n, eta) + 4.0 * n * U_ROUND * float(np.abs(g_ref).max())


def torus_hoppings(mesh, R, hop):
    """H_torus[cell point][n][n]: the full set of hoppings (the stored half ``hop`` at ``R`` plus the Hermitian conjugates at -R)
    folded onto the mesh torus, indexed like itertools.product(range(n_1), ...).  H(k) = sum_R' exp(+2 pi i k . R') H_torus(R') at
    every mesh point."""
    mesh = [int(n) for n in mesh]
    hop = np.asarray(hop)
    out = np.zeros((int(np.prod(mesh)),) + hop.shape[1:], dtype=complex)
    strides = [int(np.prod(mesh[d + 1:])) for d in range(len(mesh))]
    for vec, mat in zip(np.asarray(R), hop):
        for sign, block in ((1, mat), (-1, mat.conj().T)):
            index = sum(int(np.mod(sign * int(v), n)) * s for v, n, s in zip(vec, mesh, strides))
            out[index] += block
    return out


def main():
    # the two-site chain of tools/dm_model.py on the mesh (2, 2)
    t, tp = -0.5, -1.0
    mesh = (2, 2)
    hop = {(0, 0): np.array([[0.0, t], [0.0, 0.0]]), (1, 0): np.array([[0.0, 0.0], [tp, 0.0]])}
    ham, eig, vec = [], [], []
    for i0, i1 in itertools.product(range(2), range(2)):
        k = np.array([i0 / 2, i1 / 2])
        h = sum(np.exp(2j * np.pi * np.dot(k, key)) * mat for key, mat in hop.items())
        h = h + h.conj().T
        e, u = np.linalg.eigh(h)
        ham.append(h)
        eig.append(e)
        vec.append(u)
    ham, eig, vec = np.array(ham), np.array(eig), np.array(vec)
    z = np.array([0.3 + 0.1j, 0.3 - 0.1j, 2.0j])
    R = np.array([[0, 0], [1, 0], [-1, 0], [3, 2]])
    G = green_function(eig, vec, mesh, z, R)
    ref = resolvent(ham, mesh, z, R)
    print("two-site chain, t = %g, t' = %g, mesh %s, z = %s" % (t, tp, mesh, list(z)))
    for r, mat in zip(R, G):
        print("    G(%s, z[0]) =" % (tuple(int(x) for x in r),))
        for line in mat[0]:
            print("        " + "  ".join("%+.6f%+.6fi" % (x.real, x.imag) for x in line))
    print("    max|G - resolvent| = %.3e (bound %.3e)" % (np.abs(G - ref).max(), whole_call_tolerance(ham, eig, vec, 0.1, ref)))
    print("    G(R, conj z) - G(-R, z)^H: %.3e;  G(3, 2) == G(1, 0) bit for bit: %s"
          % (np.abs(G[1, 1] - G[2, 0].conj().T).max(), np.array_equal(G[3], G[1])))
    print("    -Im tr G(0, z[0]) / pi = %.6f, Lorentzian sum = %.6f"
          % (-np.trace(G[0, 0]).imag / np.pi, float(np.mean(np.sum((0.1 / np.pi) / ((0.3 - eig) ** 2 + 0.01), axis=1)))))


if __name__ == "__main__":
    main()
