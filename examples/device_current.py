#!/usr/bin/env python3
"""
The current through a layer with one impurity, from `Model.device_current`.

A strip of `width` chains (hopping t along the strip, t' between the chains) is one principal layer of `width` orbitals; the device is
`length` layers long and its middle layer carries one impurity, an on-site energy `eps` on the first chain.

1. The interface totals sum_i current_left[p, i] against the transmission T for a shrinking broadening eta: between two interfaces the
   current changes by 4 pi eta sum_i left[p, i], what eta absorbs in the layer, so every interface carries T as eta -> 0.
2. The current map at the smallest eta: per interface and chain the current of the states injected from the left lead, and inside the
   impurity's layer the bond currents J between the chains -- the current leaves the impurity's chain in front of it and returns behind.

Needs a GPU.

    python examples/device_current.py [width] [length] [eps] [energy]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    width = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    length = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    eps = float(sys.argv[3]) if len(sys.argv) > 3 else 3.0
    energy = float(sys.argv[4]) if len(sys.argv) > 4 else 0.3
    t, t_perp = 1.0, 0.6
    across = np.diag(np.full(width - 1, t_perp), 1)  # chain i -> chain i + 1 inside a cell
    strip = tbmodels_amd.Model(hop={(0,): across, (1,): t * np.eye(width)}, size=width, dim=1, pos=np.zeros((width, 1)), contains_cc=False)
    onsite = np.zeros((length, width))
    middle = length // 2
    onsite[middle, 0] = eps
    print("strip of %d chains, t = %.1f, t' = %.1f, E = %+.2f: %d layers, impurity %.1f on chain 1 of layer %d" % (width, t, t_perp, energy, length, eps, middle + 1))
    print("\n    eta        T       interface totals of current_left (p | p + 1)" + " " * 24 + "max|total - T|   4 pi eta sum left")
    for eta in (1e-1, 1e-2, 1e-3, 1e-4):
        got = strip.device_current(None, [energy + 1j * eta], device=onsite)
        totals = got.current_left[0, 0].sum(axis=1)
        T = got.transmission[0, 0]
        print("  %.0e  %8.5f   %s   %.2e         %.2e" % (eta, T, " ".join("%8.5f" % x for x in totals), np.abs(totals - T).max(),
                                                      4 * np.pi * eta * got.left[0, 0, 1:].sum()))
    got = strip.device_current(None, [energy + 1e-4j], device=onsite, bonds=True)
    print("\ncurrent of the left lead's states per interface and chain (eta = 1e-4):")
    print("  interface   " + " ".join("chain %-3d" % (i + 1) for i in range(width)))
    for p in range(length - 1):
        print("   %2d | %-2d    %s%s" % (p + 1, p + 2, " ".join("%9.5f" % x for x in got.current_left[0, 0, p]),
                                       "   <- in front of the impurity" if p + 1 == middle else "   <- behind it" if p == middle else ""))
    J = got.intra_left[0, 0]
    print("\nbond currents between neighbouring chains inside a layer, J[p, i, i + 1] (positive: away from chain 1):")
    for p in range(length):
        print("   layer %-2d   %s%s" % (p + 1, " ".join("%9.5f" % J[p, i, i + 1] for i in range(width - 1)), "   <- the impurity's layer" if p == middle else ""))
    # (the call takes H01 from Fourier sums of H(k): an absent hopping is zero there up to rounding, and so is its K)
    print("\nbetween different chains of neighbouring layers there is no hopping: max|K| there = %.1e, on the chains %.3f"
          % (np.abs(got.inter_left[0, 0][:, ~np.eye(width, dtype=bool)]).max(), np.abs(got.inter_left[0, 0][:, np.eye(width, dtype=bool)]).max()))


if __name__ == "__main__":
    main()
