#!/usr/bin/env python3
"""
One lattice step of a DMFT-like loop on a small model with `Model.green_function(self_energy=...)`: from a model self-energy
Sigma(i w_n) the local lattice function G_loc = G(R = 0, i w_n) by one general inversion per mesh point and frequency on the GPU, then
the Weiss field of the impurity problem, G_0^-1 = G_loc^-1 + Sigma.  An impurity solver would turn G_0 into a new Sigma; here the
model Sigma is the atomic-limit form U^2 / 4 / (i w_n) on the first two orbitals, which opens a gap in their spectral weight.  Needs
a GPU.

    python examples/dmft_local_green.py [mesh points per axis] [U]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402
from tbmodels_amd import synthetic  # noqa: E402


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    interaction = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
    mesh = (points,) * 3
    r_vec, hop, pos = synthetic.dense_model_arrays(4, 7, synthetic.MODEL_SEED + 77)
    model = tbmodels_amd.Model.from_packed(r_vec, 2.0 * hop, pos=pos)
    n = model.size
    temperature = 0.05
    w_n = (2 * np.arange(8) + 1) * np.pi * temperature
    z = 1j * w_n

    # the model self-energy: correlated orbitals 0 and 1, the others bare
    sigma = np.zeros((len(z), n, n), dtype=complex)
    for orbital in (0, 1):
        sigma[:, orbital, orbital] = interaction ** 2 / 4.0 / z

    bare = model.green_function(mesh, z, R=[0, 0, 0]).G[0]
    g_loc = model.green_function(mesh, z, R=[0, 0, 0], self_energy=sigma).G[0]  # (NZ, size, size)
    weiss_inverse = np.linalg.inv(g_loc) + sigma  # G_0^-1 = G_loc^-1 + Sigma
    weiss = np.linalg.inv(weiss_inverse)

    print("4 orbitals, mesh %d^3, T = %.2f, U = %.2f: Sigma = U^2 / 4 / (i w_n) on orbitals 0 and 1" % (points, temperature, interaction))
    print("  n     w_n      Im G_loc[0,0]   bare Im G[0,0]   Im G_loc[3,3]   Weiss field G_0[0,0]")
    for i, w in enumerate(w_n):
        print("%3d %8.4f %14.6f %16.6f %15.6f     %+.6f%+.6fi"
              % (i, w, g_loc[i, 0, 0].imag, bare[i, 0, 0].imag, g_loc[i, 3, 3].imag, weiss[i, 0, 0].real, weiss[i, 0, 0].imag))
    # the hybridisation the impurity sees: Delta = i w_n - e_loc - G_0^-1, e_loc the on-site block
    e_loc = 2.0 * (hop[0] + hop[0].conj().T)
    delta = z[:, None, None] * np.eye(n)[None] - e_loc[None] - weiss_inverse
    print("hybridisation Delta[0,0] at the first and last frequency: %+.6f%+.6fi, %+.6f%+.6fi (causal: Im Delta < 0)"
          % (delta[0, 0, 0].real, delta[0, 0, 0].imag, delta[-1, 0, 0].real, delta[-1, 0, 0].imag))
    # Sigma = 0 is the undressed function
    zero = model.green_function(mesh, z, R=[0, 0, 0], self_energy=np.zeros_like(sigma)).G[0]
    print("max|G(Sigma = 0) - undressed G| = %.2e" % np.abs(zero - bare).max())


if __name__ == "__main__":
    main()
