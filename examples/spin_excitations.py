#!/usr/bin/env python3
"""
Spin excitations of a multi-orbital model in the RPA, on top of `Model.dynamic_orbital_susceptibility`, the orbital-resolved bare
bubble chi_0[i, j](q, omega + i eta); the eigenvectors of the mesh never leave the GPU, the m x m matrices of the RPA are tiny and
stay in NumPy.

The three-orbital (xz, yz, xy) model of examples/rpa_susceptibility.py with an intra-orbital Hubbard repulsion U (a multiple of the
unit matrix in the orbital indices).  The Stoner criterion of that vertex is the largest eigenvalue of chi_0(q) U reaching 1, with the
static `Model.orbital_susceptibility`; at 0.8 of the critical U

    chi_RPA(q, omega) = (1 - chi_0(q, omega) U)^-1 chi_0(q, omega)

along Gamma - X - M on a frequency grid, and for every q the frequency at which Im sum_ij chi_RPA peaks beside that of the bare bubble:
the interaction pulls the spectral weight down towards the paramagnon near the ordering vector.

Needs a GPU.

    python examples/spin_excitations.py [mesh points per axis] [frequencies]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import tbmodels_amd  # noqa: E402, F401
from rpa_susceptibility import t2g_model  # noqa: E402


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    n_w = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    model = t2g_model()
    m, half = model.size, points // 2
    path = [(i, 0) for i in range(half + 1)] + [(half, i) for i in range(1, half + 1)]  # Gamma - X - M
    q = np.array(path, dtype=np.int64)
    mesh, T, eta, n_el = (points, points), 0.05, 0.1, 2.0
    static = model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el)
    stoner = np.array([np.linalg.eigvalsh(matrix).max() for matrix in static.chi])
    critical = 1.0 / stoner.max()
    U = 0.8 * critical
    omega = np.linspace(0.0, 3.0, n_w)
    result = model.dynamic_orbital_susceptibility(mesh, q, omega, eta=eta, temperature=T, n_electrons=n_el)
    unit = np.eye(m)
    rpa = np.linalg.solve(unit[None, None] - U * result.chi, result.chi)
    bare_im, rpa_im = result.chi.sum(axis=(2, 3)).imag, rpa.sum(axis=(2, 3)).imag
    print("three-orbital model, mesh %d x %d, 2 electrons per spin (mu = %.4f), T = %g, eta = %g, %d frequencies in [0, 3]"
          % (points, points, result.mu.mu, T, eta, n_w))
    print("critical intra-orbital U of the Stoner criterion: %.4f at q = %s / %d; RPA at U = %.4f"
          % (critical, tuple(int(x) for x in q[stoner.argmax()]), points, U))
    print("    q        Im sum chi_0 peaks at omega =   (value)     Im sum chi_RPA peaks at omega =   (value)    ratio of the peaks")
    for index, vector in enumerate(q):
        j0, j1 = int(np.abs(bare_im[index]).argmax()), int(np.abs(rpa_im[index]).argmax())
        print("  (%2d, %2d)            %6.3f             %9.4f              %6.3f               %9.4f          %7.3f"
              % (vector[0], vector[1], omega[j0], bare_im[index, j0], omega[j1], rpa_im[index, j1],
                 np.abs(rpa_im[index]).max() / np.abs(bare_im[index]).max() if np.abs(bare_im[index]).max() > 1e-12 else float("nan")))
    gap = np.abs(result.chi[:, 0] - np.conj(np.swapaxes(result.chi[:, 0], 1, 2))).max()
    print("the anti-Hermitian part of chi_0(q, i eta) is at most %.1e; its Hermitian part lies below the static matrix by at most %.4f (largest eigenvalue)"
          % (gap, max(np.linalg.eigvalsh(s - (d + d.conj().T) / 2).max() for s, d in zip(static.chi, result.chi[:, 0]))))


if __name__ == "__main__":
    main()
