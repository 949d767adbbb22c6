#!/usr/bin/env python3
"""
The lattice Green's function of the bundled silicon model from one `Model.green_function` call: the orbital-resolved,
Lorentzian-broadened spectral function A_i(w) = -Im G_ii(R = 0, w + i eta) / pi beside the tetrahedron density of states of
`Model.dos`, and the on-site G at a few fermionic Matsubara points i w_n = i (2 n + 1) pi T -- the input of a DMFT self-consistency
loop.  Eigenvalues and eigenvectors never leave the GPU.  Needs a GPU.

    python examples/green_function.py [mesh points per axis] [eta]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    eta = float(sys.argv[2]) if len(sys.argv) > 2 else 0.25
    mesh = (points,) * 3
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    model = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"], uc=data["uc"])
    edges = model.band_edges(mesh)
    lo, hi = float(edges.emin.min()) - 1.0, float(edges.emax.max()) + 1.0
    grid = np.linspace(lo, hi, 49)
    mid = 0.5 * (grid[1:] + grid[:-1])

    # the spectral function at the bin midpoints of the tetrahedron grid: 48 energies on the retarded line, one vector
    local = model.green_function(mesh, mid + 1j * eta, R=[0, 0, 0])
    spectral = -np.diagonal(local.G[0], axis1=1, axis2=2).imag / np.pi  # (NZ, size)
    tetra = model.dos(mesh, grid)
    step = grid[1] - grid[0]
    print("silicon, mesh %d^3, eta = %.3g: A(w) = -Im tr G(0, w + i eta) / pi beside the tetrahedron dos" % (points, eta))
    print("       w     A(w)    dos(w)   A_i(w) of the first four orbitals")
    for j in range(0, len(mid), 4):
        print("%8.3f %8.4f %8.4f   %s" % (mid[j], spectral[j].sum(), tetra.dos[j], "  ".join("%.4f" % x for x in spectral[j, :4])))
    print("integral of A over the window: %.4f of %d states (the Lorentzian tails beyond it hold the rest); of the dos: %.4f"
          % (spectral.sum() * step, model.size, tetra.dos.sum() * step))

    # Matsubara points: G(0, -i w_n) = G(0, i w_n)^H, so the negative frequencies cost nothing new to a caller who keeps the positive ones
    temperature = 0.1
    w_n = (2 * np.arange(4) + 1) * np.pi * temperature
    matsubara = model.green_function(mesh, np.concatenate([1j * w_n, -1j * w_n]), R=[0, 0, 0]).G[0]
    print("on-site G at the first Matsubara points, T = %.2f:" % temperature)
    for n, w in enumerate(w_n):
        g = matsubara[n]
        print("    i w_%d = %.4fi: tr G = %+.6f%+.6fi, max|G(-i w) - G(i w)^H| = %.1e"
              % (n, w, np.trace(g).real, np.trace(g).imag, np.abs(matsubara[n + 4] - g.conj().T).max()))


if __name__ == "__main__":
    main()
