#!/usr/bin/env python3
"""
NumPy model of csrc/tbk_dm.hip: the real-space one-particle density matrix of a uniform, periodic k mesh.

    P(k)[i][j]   = sum_b w[k][b] U[k][i][b] conj(U[k][j][b])
    rho(R)[i][j] = sum_k exp(-2 pi i sum_d ((i_d R_d) mod n_d) / n_d) P(k)[i][j]        k = (i_1 / n_1, ..., i_dim / n_dim)

``w`` are the point weights of tools/occ_model.py at the chemical potential, ``U[k][i][b]`` is component i of band b.  The phase
is reduced in integers before any floating-point operation, by the common denominator: t_d = (i_d (R_d mod n_d)) mod n_d -- the
residue of i_d R_d, from factors below 2^31 each, so 64-bit arithmetic holds it -- then num = (sum_d t_d NK / n_d) mod NK with
NK = prod n_d, and the phase is cos(2 pi num / NK) - i sin(2 pi num / NK).  The kernel does the same and takes sincospi(2 num / NK).
R and R + n_d e_d give the same integers, so the same bits.

`python tools/dm_model.py` prints a small worked case.  Design tooling: nothing in the product imports it.
"""

import itertools

import numpy as np


def projectors(w, U):
    """P[NK][n][n] from weights ``w`` of shape mesh + (n,) or (NK, n) and eigenvectors ``U`` of shape mesh + (n, n) or (NK, n, n)."""
    w = np.asarray(w, dtype=float)
    n = w.shape[-1]
    flat_w, flat_u = w.reshape(-1, n), np.asarray(U).reshape(-1, n, n)
    return np.einsum("kb,kib,kjb->kij", flat_w, flat_u, flat_u.conj())


def phase_numerators(mesh, R):
    """num[NR][NK] in [0, NK): the phase of mesh point k (mesh order, last axis fastest) and vector R is exp(-2 pi i num / NK)."""
    mesh = [int(n) for n in mesh]
    R = np.asarray(R)
    if R.dtype.kind not in "iu":
        raise ValueError("R must be integers")
    R = R.astype(np.int64).reshape(-1, len(mesh))
    n_k = int(np.prod(mesh, dtype=object))
    index = np.array(list(itertools.product(*[range(n) for n in mesh])), dtype=np.int64).reshape(n_k, len(mesh))
    num = np.zeros((R.shape[0], n_k), dtype=np.int64)
    for d, n_d in enumerate(mesh):
        reduced = np.mod(R[:, d], n_d)  # non-negative
        t_d = np.mod(index[None, :, d] * reduced[:, None], n_d)
        num += t_d * (n_k // n_d)
    return np.mod(num, n_k), n_k


def phases(mesh, R):
    """exp(-2 pi i k . R) as complex128 [NR][NK] with the integer reduction of the module's head."""
    num, n_k = phase_numerators(mesh, R)
    angle = 2.0 * np.pi * (num.astype(float) / float(n_k))
    return np.cos(angle) - 1j * np.sin(angle)


def density_matrix(w, U, mesh, R):
    """rho[NR][n][n] for the integer vectors ``R`` of shape (NR, dim)."""
    P = projectors(w, U)
    return np.einsum("rk,kij->rij", phases(mesh, R), P)


def band_energy(rho, hop):
    """2 Re sum_R sum_ij conj(rho(R)[i][j]) hop[R][i][j] for the STORED half of the hoppings (H(k) = sum_R e^{2 pi i k R} hop[R] + h.c.)
    and rho at the same vectors: the band energy per cell, sum_k sum_b w[k][b] E[k][b]."""
    return 2.0 * float(np.real(np.sum(np.conj(rho) * np.asarray(hop))))


def main():
    # the two-site chain with hopping t inside the cell and t' to the next cell along axis 0, on the mesh (2, 2), lower band filled
    t, tp = -0.5, -1.0
    mesh = (2, 2)
    hop = {(0, 0): np.array([[0.0, t], [0.0, 0.0]]), (1, 0): np.array([[0.0, 0.0], [tp, 0.0]])}
    eig, vec = [], []
    for i0, i1 in itertools.product(range(2), range(2)):
        k = np.array([i0 / 2, i1 / 2])
        ham = sum(np.exp(2j * np.pi * np.dot(k, key)) * mat for key, mat in hop.items())
        ham = ham + ham.conj().T
        e, u = np.linalg.eigh(ham)
        eig.append(e)
        vec.append(u)
    eig, vec = np.array(eig), np.array(vec)
    w = np.zeros((4, 2))
    w[:, 0] = 0.25  # a full band: 1 / NK at every mesh point
    R = np.array([[0, 0], [1, 0], [-1, 0], [3, 2]])
    rho = density_matrix(w, vec, mesh, R)
    print("two-site chain, t = %g, t' = %g, mesh %s, lower band filled" % (t, tp, mesh))
    num, n_k = phase_numerators(mesh, R)
    for r, row in zip(R, num):
        print("    R = %-8s phase numerators over NK = %d: %s" % (tuple(int(x) for x in r), n_k, list(int(x) for x in row)))
    for r, mat in zip(R, rho):
        print("    rho(%s) =" % (tuple(int(x) for x in r),))
        for line in mat:
            print("        " + "  ".join("%+.6f%+.6fi" % (z.real, z.imag) for z in line))
    print("    rho(-R) - rho(R)^H: %.3e;  rho(3, 2) == rho(1, 0) bit for bit: %s" % (np.abs(rho[2] - rho[1].conj().T).max(), np.array_equal(rho[3], rho[1])))
    stored = np.array([hop[(0, 0)], hop[(1, 0)]])
    print("    band energy from rho: %.15f   sum_k w E: %.15f" % (band_energy(rho[:2], stored), float((w * eig).sum())))
    print("    bond order inside the cell rho(0)[0][1] = %.6f, to the next cell rho(1, 0)[1][0] = %.6f" % (rho[0][0, 1].real, rho[1][1, 0].real))


if __name__ == "__main__":
    main()
