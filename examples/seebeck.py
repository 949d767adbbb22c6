#!/usr/bin/env python3
"""
Boltzmann transport of silicon in the relaxation-time approximation from `Model.transport_distribution`: the transport distribution
Sigma_xx(E) across the gap, and from it sigma / tau and the Seebeck coefficient S(mu) at T = 0.025 eV (about room temperature) for
chemical potentials from the valence band through the gap into the conduction band.  Neither eigenvectors nor velocity matrices leave
the GPU; `transport_coefficients` is the small host step.  Units: e = hbar = k_B = 1 (S in units of k_B / e = 86.17 uV/K).

Needs a GPU.

    python examples/seebeck.py [mesh points per axis]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    model = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"], uc=data["uc"])
    mesh = (points,) * 3
    edges = model.band_edges(mesh)
    top, bottom = float(edges.emax[3]), float(edges.emin[4])  # four valence bands
    temperature = 0.025
    energies = np.linspace(top - 3.0, bottom + 3.0, 1201)
    result = model.transport_distribution(mesh, energies, cartesian=True)
    mid = 0.5 * (energies[:-1] + energies[1:])
    print("silicon, mesh %d^3: valence-band top %.3f eV, conduction-band bottom %.3f eV; Cartesian axes, per unit volume" % (points, top, bottom))
    print("Sigma_xx(E):")
    for j in range(0, len(mid), 100):
        print("  E = %7.3f   Sigma_xx = %10.4e   %s" % (mid[j], result.tdf[0, 0, j], "(gap)" if top < mid[j] < bottom else ""))
    mu = np.linspace(top - 0.5, bottom + 0.5, 13)
    out = tbmodels_amd.transport_coefficients(result, temperature, mu)
    print("T = %.3f eV: sigma_xx / tau and S_xx (k_B / e) against mu -- holes give S > 0, electrons S < 0" % temperature)
    for m, s, q in zip(mu, out.sigma[0, :, 0, 0], out.seebeck[0, :, 0, 0]):
        print("  mu = %7.3f   sigma/tau = %10.3e   S = %+8.3f   (%+7.1f uV/K)" % (m, s, q, 86.17 * q))


if __name__ == "__main__":
    main()
