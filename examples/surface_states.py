#!/usr/bin/env python3
"""
Edge states of a stack of Su-Schrieffer-Heeger chains from one `Model.surface_green_function` call.

Two orbitals A, B per cell; along the stacking axis y the chain alternates the hopping v (A-B inside a cell) and w (B of a cell to A
of the next); a hopping t' between A and B of neighbouring chains makes the intracell amplitude v + 2 t' cos(2 pi k) depend on the
in-plane k.  Where |v + 2 t' cos(2 pi k)| < w the chain is in its topological phase and both surfaces carry a state at E = 0: it shows
in `bottom` (on A, the first orbital of the surface cell) and `top` (on B) and is absent from `bulk`, whose spectral weight at E = 0
is the tail of the gapped bands alone.  The last lines form the lead self-energy H01 G_bottom H01^H and hand it to
`green_function(self_energy=...)`.  Needs a GPU.

    python examples/surface_states.py [k-points] [eta]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    points = int(sys.argv[1]) if len(sys.argv) > 1 else 17
    eta = float(sys.argv[2]) if len(sys.argv) > 2 else 0.02
    v, w, t_plane = 0.6, 1.0, 0.4
    intracell = np.array([[0.0, v], [0.0, 0.0]])      # A -> B inside the cell (the conjugate is added by the model)
    intercell = np.array([[0.0, 0.0], [w, 0.0]])      # B of the cell at R to A of the cell at R + (0, 1)
    in_plane = np.array([[0.0, t_plane], [0.0, 0.0]])  # A to B of the chain at R + (1, 0); its conjugate couples back
    model = tbmodels_amd.Model(hop={(0, 0): intracell, (0, 1): intercell, (1, 0): in_plane + in_plane.T}, size=2, dim=2,
                               pos=np.zeros((2, 2)), contains_cc=False)
    k = np.linspace(0.0, 0.5, points)[:, None]
    energies = np.array([0.0, 0.5, 1.5]) + 1j * eta
    maps = model.surface_green_function(k, energies, axis=1, spectral=True)
    print("SSH stack: v = %.2f, w = %.2f, t' = %.2f, eta = %.3g; principal layers of %d cell(s), %d ... %d iterations"
          % (v, w, t_plane, eta, maps.layers, maps.iterations.min(), maps.iterations.max()))
    print("-Im G_ii(k, E = 0) / pi      |v(k)|/w   bottom A   bottom B      top A      top B     bulk A     bulk B")
    for i, kk in enumerate(k[:, 0]):
        ratio = abs(v + 2 * t_plane * np.cos(2 * np.pi * kk)) / w
        row = np.concatenate([maps.bottom[i, 0], maps.top[i, 0], maps.bulk[i, 0]])
        print("k = %.4f %s %10.3f %s" % (kk, "edge state" if ratio < 1 else "  trivial ", ratio, " ".join("%10.4f" % x for x in row)))
    inside = np.abs(v + 2 * t_plane * np.cos(2 * np.pi * k[:, 0])) < 0.9 * w
    print("mean weight at E = 0 where the chain is topological: bottom A %.3f, top B %.3f, bulk %.4f (a pole of weight ~ 1 / (pi eta) = %.1f)"
          % (maps.bottom[inside, 0, 0].mean(), maps.top[inside, 0, 1].mean(), maps.bulk[inside, 0].mean(), 1 / (np.pi * eta)))

    # a lead self-energy for green_function: the semi-infinite stack beyond a layer, seen from that layer
    full = model.surface_green_function(k[:1], energies, axis=1)
    hop_up = np.array([[0.0, 0.0], [w, 0.0]])  # H01 = H_1(k): here independent of k
    sigma = np.array([hop_up @ g @ hop_up.conj().T for g in full.bottom[0]])
    dressed = model.green_function((8, 8), energies, R=[0, 0], self_energy=sigma)
    print("Sigma_lead(E = 0) = H01 G_bottom H01^H at k = 0:")
    for line in sigma[0]:
        print("    " + "  ".join("%+.5f%+.5fi" % (x.real, x.imag) for x in line))
    print("handed to green_function(self_energy=...): tr G(0, E = 0) = %+.5f%+.5fi" % (np.trace(dressed.G[0, 0]).real, np.trace(dressed.G[0, 0]).imag))


if __name__ == "__main__":
    main()
