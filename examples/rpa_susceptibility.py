#!/usr/bin/env python3
"""
A multi-orbital RPA on top of `Model.susceptibility_tensor`, the four-index bare bubble chi_0[i, l; j, m](q); the eigenvectors of the
mesh never leave the GPU, the m^2 x m^2 matrices of the RPA are tiny and stay in NumPy.

A three-orbital (xz, yz, xy) model on the square lattice; chi_0 along Gamma - X - M - Gamma; the Kanamori spin and charge vertices
U^s, U^c (U, U' = U - 2 J, J, J' = J) as m^2 x m^2 matrices in the index order of Graser, Maier, Hirschfeld and Scalapino, New J.
Phys. 11, 025016 (2009):

    chi_{l1 l2 l3 l4}(q) = chi[q, l2, l1, l4, l3]                      rows (l1, l2), columns (l3, l4)
    chi_s = (1 - chi_0 U^s)^-1 chi_0        chi_c = (1 + chi_0 U^c)^-1 chi_0

and the Stoner criterion: the largest eigenvalue of chi_0 U^s reaches 1 at the magnetic instability.  Both vertices are linear in U at
fixed J / U, so the critical U is 1 / max_q of that eigenvalue at U = 1; the RPA susceptibilities are printed at 0.8 of it.

Needs a GPU.

    python examples/rpa_susceptibility.py [mesh points per axis] [J / U]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def t2g_model():
    """xz hops along x, yz along y, xy along both and the diagonals; xz and yz mix on the diagonals with the sign of xy symmetry."""
    t1, t2, t3, t4, t5, split = 1.0, 0.1, 0.8, 0.3, 0.15, -0.2
    mix = np.zeros((3, 3), dtype=complex)
    mix[0, 1] = mix[1, 0] = -t5
    diagonal = np.diag([0.0, 0.0, -t4]).astype(complex)
    # half-space hoppings; the R = 0 block is stored halved (contains_cc=False adds the conjugate)
    hop = {(0, 0): np.diag([0.0, 0.0, split]).astype(complex) / 2, (1, 0): np.diag([-t1, -t2, -t3]).astype(complex),
           (0, 1): np.diag([-t2, -t1, -t3]).astype(complex), (1, 1): diagonal + mix, (1, -1): diagonal - mix}
    return tbmodels_amd.Model(hop=hop, size=3, dim=2, contains_cc=False)


def kanamori(m, U, J):
    """(U^s, U^c) as m^2 x m^2 matrices with rows (l1, l2) and columns (l3, l4)."""
    U1, J1 = U - 2.0 * J, J  # U', J'
    spin, charge = np.zeros((m, m, m, m)), np.zeros((m, m, m, m))
    for a in range(m):
        spin[a, a, a, a] = charge[a, a, a, a] = U
        for b in range(m):
            if a == b:
                continue
            spin[a, b, a, b], charge[a, b, a, b] = U1, -U1 + 2.0 * J  # l1 = l3 != l2 = l4
            spin[a, a, b, b], charge[a, a, b, b] = J, 2.0 * U1 - J    # l1 = l2 != l3 = l4
            spin[a, b, b, a] = charge[a, b, b, a] = J1                # l1 = l4 != l2 = l3
    return spin.reshape(m * m, m * m), charge.reshape(m * m, m * m)


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    ratio = float(sys.argv[2]) if len(sys.argv) > 2 else 0.25
    model = t2g_model()
    m, half = model.size, points // 2
    path = [(i, 0) for i in range(half + 1)] + [(half, i) for i in range(1, half + 1)] + [(i, i) for i in range(half - 1, 0, -1)]
    q = np.array(path, dtype=np.int64)
    result = model.susceptibility_tensor((points, points), q, temperature=0.05, n_electrons=2.0)
    bare = np.transpose(result.chi, (0, 2, 1, 4, 3)).reshape(len(q), m * m, m * m)  # chi_{l1 l2 l3 l4}, rows (l1, l2), columns (l3, l4)
    spin1, _ = kanamori(m, 1.0, ratio)
    stoner1 = np.array([np.linalg.eigvals(matrix @ spin1).real.max() for matrix in bare])
    critical = 1.0 / stoner1.max()
    U = 0.8 * critical
    spin, charge = kanamori(m, U, ratio * U)
    unit = np.eye(m * m)
    print("three-orbital model, mesh %d x %d, 2 electrons per spin (mu = %.4f), T = 0.05, J / U = %.2f" % (points, points, result.mu.mu, ratio))
    print("critical U of the Stoner criterion: %.4f at q = %s / %d; RPA at U = %.4f" % (critical, tuple(int(x) for x in q[stoner1.argmax()]), points, U))
    print("    q        largest eigenvalue of:  chi_0    chi_0 U^s    chi_s (RPA)    chi_c (RPA)    Hermitian to")
    for vector, matrix in zip(q, bare):
        chi_s = np.linalg.solve(unit - matrix @ spin, matrix)
        chi_c = np.linalg.solve(unit + matrix @ charge, matrix)
        print("  (%2d, %2d)                       %8.4f   %8.4f     %9.4f      %9.4f       %.1e"
              % (vector[0], vector[1], np.linalg.eigvalsh(matrix).max(), np.linalg.eigvals(matrix @ spin).real.max(),
                 np.linalg.eigvals(chi_s).real.max(), np.linalg.eigvals(chi_c).real.max(), np.abs(matrix - matrix.conj().T).max()))
    block = np.einsum("qiijj->qij", result.chi)
    orbital = model.orbital_susceptibility((points, points), q, temperature=0.05, n_electrons=2.0).chi
    print("density-density block against Model.orbital_susceptibility: max difference %.1e" % np.abs(block - orbital).max())


if __name__ == "__main__":
    main()
