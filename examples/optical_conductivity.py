#!/usr/bin/env python3
"""
Two uses of `Model.optical_conductivity`, the Kubo conductivity of a uniform k mesh; the velocity matrices never leave the GPU.

1. The Hall plateau of the Qi-Wu-Zhang model: 2 pi sigma_xy(0) at low temperature and small broadening next to the Chern number of
   the lower band from `Model.berry_flux`, for the masses u = -3, -1, 1, 3.
2. The absorption edge of silicon: Re sigma_xx(omega) on a frequency grid, next to the direct gap of the same mesh from
   `Model.eigenval_array` and the indirect gap from `Model.band_edges`.  Below the direct gap only the tails of the broadening absorb.

Needs a GPU.

    python examples/optical_conductivity.py [mesh points per axis of the QWZ model] [mesh points per axis of silicon]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def qwz(u):
    sx = np.array([[0, 1], [1, 0]], dtype=complex)
    sy = np.array([[0, -1j], [1j, 0]], dtype=complex)
    sz = np.array([[1, 0], [0, -1]], dtype=complex)
    # half-space hoppings; the R = 0 block is stored halved (contains_cc=False adds the conjugate)
    hop = {(0, 0): u * sz / 2, (1, 0): sz / 2 - 0.5j * sx, (0, 1): sz / 2 - 0.5j * sy}
    return tbmodels_amd.Model(hop=hop, size=2, dim=2, contains_cc=False)


def hall_plateau(points):
    mesh = (points, points)
    print("Qi-Wu-Zhang model, mesh %d x %d, mu = 0, T = 0.02, eta = 0.05" % mesh)
    for u in (-3.0, -1.0, 1.0, 3.0):
        model = qwz(u)
        chern = int(model.berry_flux(mesh, 1).chern[0][0, 0])
        sigma = model.optical_conductivity(mesh, [0.0], eta=0.05, temperature=0.02, energy=0.0).sigma[0]
        print("u = %+.1f: 2 pi sigma_xy(0) = %+.6f   C = %+d   (sigma_xx(0) = %.2e)" % (u, 2 * np.pi * sigma[0, 1].real, chern, sigma[0, 0].real))


def absorption_edge(points):
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    model = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"], uc=data["uc"])
    mesh = (points,) * 3
    edges = model.band_edges(mesh)
    top, bottom = float(edges.emax[3]), float(edges.emin[4])  # four valence bands
    axes = [np.arange(points) / points] * 3
    kpts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    bands = model.eigenval_array(kpts)
    direct = float((bands[:, 4] - bands[:, 3]).min())
    omega = np.linspace(0.0, direct + 2.0, 25)
    result = model.optical_conductivity(mesh, omega, eta=0.05, temperature=0.02, energy=(top + bottom) / 2, convention=1, cartesian=True)
    print("silicon, mesh %d^3: indirect gap %.3f eV (band_edges), direct gap %.3f eV; Re sigma_xx(omega), Cartesian axes, per unit volume" % (points, bottom - top, direct))
    for w, s in zip(omega, result.sigma):
        print("  omega = %6.3f   Re sigma_xx = %10.3e   %s" % (w, s[0, 0].real, "<- direct gap" if abs(w - direct) <= (omega[1] - omega[0]) / 2 else ""))


def main():
    hall_plateau(int(sys.argv[1]) if len(sys.argv) > 1 else 24)
    absorption_edge(int(sys.argv[2]) if len(sys.argv) > 2 else 12)


if __name__ == "__main__":
    main()
