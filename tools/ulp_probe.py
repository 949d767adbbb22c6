#!/usr/bin/env python3
"""
Compares the output of tools/ulp_probe.hip (the device's exp and expm1 in double precision) with NumPy's on the same arguments and
prints the largest distance in units of the last place of NumPy's value.  DESIGN.md 15.4 takes twice the figure as the allowance
of tol_chi.  Design tooling: nothing in the product imports it.
"""

import sys

import numpy as np


def ulps(got, want):
    """|got - want| in units of the spacing of doubles at ``want`` (subnormal results: of the subnormal spacing)."""
    spacing = np.spacing(np.abs(want))
    return np.abs(got - want) / spacing


def main():
    data = np.fromfile(sys.argv[1], dtype=np.float64).reshape(3, -1)
    x, dev_exp, dev_expm1 = data
    for name, got, want in (("exp", dev_exp, np.exp(x)), ("expm1", dev_expm1, np.expm1(x))):
        d = ulps(got, want)
        worst = int(np.argmax(d))
        normal = np.abs(want) >= np.finfo(float).tiny
        print("%-6s %d arguments in [%.3g, %.3g]: max %.2f ulp (at x = %.17g), max over normal results %.2f ulp, %.1f %% equal bits"
              % (name, len(x), x.min(), x.max(), d.max(), x[worst], d[normal].max(), 100.0 * np.mean(got == want)))


if __name__ == "__main__":
    main()
