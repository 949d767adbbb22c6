#!/usr/bin/env python3
"""
The Chern number of the Qi-Wu-Zhang model from the lattice Berry flux of a uniform k mesh: one `Model.berry_flux` call per mass u,
the eigenvectors never leave the GPU.  H(k) = sin K_x sigma_x + sin K_y sigma_y + (u + cos K_x + cos K_y) sigma_z, K = 2 pi k: the
lower band has C = +1 for 0 < u < 2, -1 for -2 < u < 0 and 0 outside.  Needs a GPU.

    python examples/chern_number.py [mesh points per axis]
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


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    mesh = (points, points)
    print("Qi-Wu-Zhang model, lower band, mesh %d x %d" % mesh)
    for u in (-3.0, -1.0, 1.0, 3.0):
        result = qwz(u).berry_flux(mesh, 1)
        print("u = %+.1f: C = %+d, largest |flux| = %.4f turn, smallest |link| = %.4f, sum of the fluxes / 2 pi = %+.12f"
              % (u, result.chern[0][0, 0], np.abs(result.flux).max() / (2 * np.pi), result.link_min[0], result.flux.sum() / (2 * np.pi)))


if __name__ == "__main__":
    main()
