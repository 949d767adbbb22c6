#!/usr/bin/env python3
"""
Shot noise of a disordered wire, from `Model.transmission_channels`: the Fano factor <sum T_n (1 - T_n)> / <sum T_n> against the
length of the disordered region, and the distribution of the transmission eigenvalues T_n.

A ladder of `width` chains (hopping t along the wire and across it) between two clean leads; on `M` sites along the wire every
orbital gets an on-site energy uniform in [-W / 2, W / 2].  One call per length takes all the samples and returns `width` numbers per
sample: no Green's function and no self-energy leaves the GPU.  A clean wire has T_n = 1 in every open channel and no noise; between
the mean free path and the localisation length the wire is diffusive, the T_n follow Dorokhov's bimodal density
1 / (T sqrt(1 - T)) -- most channels closed or open, few in between -- and the Fano factor is 1 / 3; longer wires localise, one
channel carries what is left and the Fano factor tends to 1.  The regime is narrow for a handful of channels: the printed 1 / 3 is
where to look, nothing is asserted about it.

Needs a GPU.

    python examples/shot_noise.py [width] [W] [samples]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    width = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    disorder = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    samples = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    t, eta = 1.0, 1e-8
    rungs = t * (np.eye(width, k=1) + np.eye(width, k=-1))  # across the wire: Hermitian, half of it with contains_cc=False
    wire = tbmodels_amd.Model(hop={(0,): rungs / 2, (1,): t * np.eye(width)}, size=width, dim=1, pos=np.zeros((width, 1)), contains_cc=False)
    energy = 0.3 + 1j * eta
    clean = wire.transmission_channels(None, energy, length=1)
    open_channels = int(np.count_nonzero(clean.channels[0, 0] > 0.5))
    print("a ladder of %d chains, t = %.1f, W = %.2f, E = %.1f, %d samples per length, eta = %.0e: %d open channels, clean noise %.1e"
          % (width, t, disorder, energy.real, samples, eta, open_channels, clean.noise[0, 0]))
    print("     M     <T>     <noise>    Fano   (diffusive: 1/3 = 0.3333)")
    rng = np.random.default_rng(1)
    kept = None
    for M in (4, 8, 16, 32, 64, 128, 256):
        onsite = rng.uniform(-disorder / 2, disorder / 2, (samples, M, width))
        got = wire.transmission_channels(None, energy, devices=onsite)
        mean_t, mean_noise = got.transmission[0, 0].mean(), got.noise[0, 0].mean()
        print("  %4d  %7.3f  %9.4f  %7.4f" % (M, mean_t, mean_noise, mean_noise / mean_t))
        if kept is None or abs(mean_noise / mean_t - 1.0 / 3.0) < abs(kept[1] - 1.0 / 3.0):
            kept = (M, mean_noise / mean_t, got.channels[0, 0, :, :open_channels].ravel())
    M, fano, values = kept
    print("the T_n of the open channels at M = %d (Fano %.4f); Dorokhov's density piles them up at both ends:" % (M, fano))
    edges = np.linspace(0.0, 1.0, 11)
    counts = np.histogram(values, bins=edges)[0]
    for lo, hi, c in zip(edges[:-1], edges[1:], counts):
        print("    [%.1f, %.1f)  %6d  %s" % (lo, hi, c, "#" * int(round(60.0 * c / max(counts.max(), 1)))))

if __name__ == "__main__":
    main()
