#!/usr/bin/env python3
"""
Anderson localisation of a wire, from `Model.transmission_ensemble`: <ln T> against the length of the disordered region.

A ladder of `width` chains (hopping t along the wire and across it) between two clean leads; on `M` sites along the wire every
orbital gets an on-site energy uniform in [-W / 2, W / 2].  One call per length takes all the samples: the lead decimation is done
once per energy for a group of samples, the on-site energies stay diagonal into the kernel, and `samples` doubles per energy come
back.  <ln T> falls linearly with M; its slope is -2 / xi, xi the localisation length of the most extended channel.  For one chain at
the band centre the weak-disorder result is xi = 96 t^2 / W^2 sites (Thouless; up to the Kappus-Wegner anomaly at E = 0).

Needs a GPU.

    python examples/disorder_average.py [width] [W] [samples]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    width = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    disorder = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
    samples = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    t, eta = 1.0, 1e-8
    rungs = t * (np.eye(width, k=1) + np.eye(width, k=-1))  # across the wire: Hermitian, half of it with contains_cc=False
    wire = tbmodels_amd.Model(hop={(0,): rungs / 2, (1,): t * np.eye(width)}, size=width, dim=1, pos=np.zeros((width, 1)), contains_cc=False)
    energies = np.array([0.1, 0.5, 1.0]) + 1j * eta
    lengths = [8, 16, 32, 64, 128]
    rng = np.random.default_rng(1)
    print("a ladder of %d chain(s), t = %.1f, W = %.2f, %d samples per length, eta = %.0e" % (width, t, disorder, samples, eta))
    print("     M   " + "   ".join("<ln T>(E = %.1f)  var" % z.real for z in energies))
    means = []
    for M in lengths:
        onsite = rng.uniform(-disorder / 2, disorder / 2, (samples, M, width))
        got = wire.transmission_ensemble(None, energies, onsite)
        log_t = np.log(got.transmission[0])  # (NZ, S)
        means.append(log_t.mean(axis=1))
        print("  %4d   " % M + "   ".join("%14.4f  %6.2f" % (log_t[i].mean(), log_t[i].var()) for i in range(len(energies))))
    slope = np.polyfit(lengths, np.array(means), 1)[0]
    print("localisation length xi = -2 / slope:  " + "   ".join("%.1f sites at E = %.1f" % (-2.0 / slope[i], z.real) for i, z in enumerate(energies)))
    if width == 1:
        print("one chain, weak disorder: 24 (4 t^2 - E^2) / W^2 = " + ", ".join("%.1f" % (24 * (4 * t * t - z.real ** 2) / disorder ** 2) for z in energies))


if __name__ == "__main__":
    main()
