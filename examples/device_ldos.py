#!/usr/bin/env python3
"""
A resonant level between two barriers, from `Model.device_green_function`.

A chain (one orbital, hopping t) with a device of 2 `width` + `well` sites: `width` sites raised by `height`, a well of `well` sites,
`width` raised sites again.  The well holds quasi-bound levels; at each of them the transmission peaks and the local density of states
piles up inside the well.

1. The LDOS map over layer x energy, printed as a table: the resonance shows as a ridge on the well's sites.
2. `left` against `right` at the strongest resonance: a symmetric structure is fed equally from both leads in the middle of the well,
   and each barrier's outer side belongs to the lead next to it; `ldos - left - right` is what the broadening eta absorbs.

Needs a GPU.

    python examples/device_ldos.py [width] [well] [height] [eta]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    width = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    well = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    height = float(sys.argv[3]) if len(sys.argv) > 3 else 2.5
    eta = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-3
    t = 1.0
    chain = tbmodels_amd.Model(hop={(1,): np.array([[t]])}, size=1, dim=1, pos=np.zeros((1, 1)), contains_cc=False)
    onsite = np.concatenate([np.full(width, height), np.zeros(well), np.full(width, height)])[:, None]  # the (M, N) form
    energies = np.linspace(-1.9, 1.9, 381) + 1j * eta
    got = chain.device_green_function(None, energies, device=onsite)
    ldos, left, right, T = got.ldos[0, :, :, 0], got.left[0, :, :, 0], got.right[0, :, :, 0], got.transmission[0]
    inside = ldos[:, width:width + well].sum(axis=1)
    peaks = [i for i in range(1, len(energies) - 1) if inside[i] > inside[i - 1] and inside[i] >= inside[i + 1] and T[i] > 0.05]
    print("chain, t = %.1f, eta = %.0e: barriers of %d sites raised by %.2f around a well of %d sites (%d ... %d iterations of the decimation)"
          % (t, eta, width, height, well, got.iterations.min(), got.iterations.max()))
    print("resonances (maxima of the well's LDOS with T > 0.05): " + ", ".join("E = %+.2f (T = %.3f)" % (energies[i].real, T[i]) for i in peaks))
    rows = sorted(set(peaks) | set(range(0, len(energies), 38)))
    print("\n      E        T    LDOS per site: " + " ".join("%s%-2d" % ("B" if v > 0 else "w", p + 1) for p, v in enumerate(onsite[:, 0])))
    for i in rows:
        print("  %+5.2f  %7.4f                 %s%s" % (energies[i].real, T[i], " ".join("%7.3f" % x for x in ldos[i]), "   <- resonance" if i in peaks else ""))
    if peaks:
        best = max(peaks, key=lambda i: T[i])
        print("\nat E = %+.2f: the density injected from each lead, per site" % energies[best].real)
        print("  site   ldos      left     right    ldos - left - right")
        for p in range(ldos.shape[1]):
            print("  %3d  %8.4f  %8.4f  %8.4f  %10.2e" % (p + 1, ldos[best, p], left[best, p], right[best, p], ldos[best, p] - left[best, p] - right[best, p]))
    rest = ldos - left - right
    print("\nldos - left - right over the whole map: %.2e ... %.2e (positive: eta |G|^2 / pi; it vanishes with eta)" % (rest.min(), rest.max()))


if __name__ == "__main__":
    main()
