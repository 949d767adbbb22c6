#!/usr/bin/env python3
"""
Landauer transmission through a barrier, from `Model.transmission`.

1. A chain (one orbital, hopping t): the pristine crystal transmits one channel inside its band [-2 t, 2 t] and nothing outside;
   a barrier of `length` sites raised by `height` suppresses it, the more the longer and higher it is.
2. A small 2-D model (two orbitals, stacked along y): T(k, E) of the pristine crystal counts the right-moving bands at every
   in-plane k -- the steps 0, 1, 2 -- and the mean over k is the conductance per cell in units of e^2 / h; a gated slab (an on-site
   shift on `length` layers, given in the (M, N) form) lowers it.

Needs a GPU.

    python examples/transmission.py [length] [height] [eta]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    length = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    height = float(sys.argv[2]) if len(sys.argv) > 2 else 1.5
    eta = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-4
    energies = np.linspace(-2.5, 2.5, 11) + 1j * eta

    t = 1.0
    chain = tbmodels_amd.Model(hop={(1,): np.array([[t]])}, size=1, dim=1, pos=np.zeros((1, 1)), contains_cc=False)
    clean = chain.transmission(None, energies, length=length)
    barrier = chain.transmission(None, energies, device=np.full((length, 1), height))
    longer = chain.transmission(None, energies, device=np.full((2 * length, 1), height))
    print("chain, t = %.1f, eta = %.0e: a barrier of height %.2f on %d and %d sites (%d ... %d iterations of the decimation)"
          % (t, eta, height, length, 2 * length, clean.iterations.min(), clean.iterations.max()))
    print("      E    pristine   barrier(%d)   barrier(%d)" % (length, 2 * length))
    for i, z in enumerate(energies):
        print("  %+5.2f  %10.6f  %11.3e  %11.3e" % (z.real, clean.transmission[0, i], barrier.transmission[0, i], longer.transmission[0, i]))

    # two orbitals with different on-site energies: bands that overlap in a window, so that 0, 1 or 2 channels are open
    onsite = np.diag([-0.6, 0.6])
    along = np.array([[0.5, 0.1], [0.1, -0.4]])     # to the cell at R + (0, 1), the stacking direction
    across = np.array([[0.15, 0.0], [0.0, 0.1]])    # to the cell at R + (1, 0)
    model = tbmodels_amd.Model(hop={(0, 0): onsite / 2, (0, 1): along, (1, 0): across}, size=2, dim=2, pos=np.zeros((2, 2)), contains_cc=False)
    k = (np.arange(32) / 32.0)[:, None]
    energies = np.linspace(-1.8, 1.8, 13) + 1j * eta
    clean = model.transmission(k, energies, axis=1, length=length)
    gate = np.tile(np.array([height, height]), (length, 1))  # the (M, N) form: real on-site shifts per layer
    gated = model.transmission(k, energies, axis=1, device=gate)
    print("\n2-D model, stacked along y, 32 in-plane k: open channels of the pristine crystal and the conductance per cell (e^2 / h)")
    print("      E    k with 0 / 1 / 2 channels    G pristine    G gated (+%.2f on %d layers)" % (height, length))
    for i, z in enumerate(energies):
        steps = np.rint(clean.transmission[:, i]).astype(int)
        print("  %+5.2f        %2d / %2d / %2d          %10.5f    %10.5f" % (z.real, (steps == 0).sum(), (steps == 1).sum(), (steps == 2).sum(),
                                                                         clean.transmission[:, i].mean(), gated.transmission[:, i].mean()))
    off = np.abs(clean.transmission - np.rint(clean.transmission)).max()
    print("largest distance of the pristine T(k, E) from an integer: %.2e (eta = %.0e; band edges are rounded on the scale of eta)" % (off, eta))


if __name__ == "__main__":
    main()
