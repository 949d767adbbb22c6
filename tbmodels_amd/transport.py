"""
Boltzmann transport in the relaxation-time approximation from a transport distribution: the small host step behind
``Model.transport_distribution``.  Pure NumPy; ``e = hbar = k_B = 1``, the relaxation time ``tau`` is left out (conductivities are
per ``tau``), reduced or Cartesian axes as the distribution has them.

    L_n[a, c] = sum_bins  tdf[a, c, j] (f(E_j) - f(E_{j+1})) (E_mid,j - mu)^n                 n = 0, 1, 2
    sigma / tau = L0,      S = -L0^-1 L1 / T,      kappa_e / tau = (L2 - L1 L0^-1 L1) / T

``f(E_j) - f(E_{j+1})`` is the exact integral of ``-f'`` over bin j, so a constant ``Sigma`` is integrated exactly in ``L0``; the
moments use the bin midpoint, the midpoint rule's ``step^2 / (24 T^2)`` relative error.
"""

import collections as co

import numpy as np

#: what :func:`transport_coefficients` returns; the leading axes of the tensors are ``(NT, NMU)``
TransportCoefficients = co.namedtuple("TransportCoefficients", ("T", "mu", "L0", "L1", "L2", "sigma", "seebeck", "kappa"))

THERMAL_WINDOW = 40.0  # the grid must cover mu +- 40 T: -f' is below exp(-40) = 4e-18 of its peak outside


def _fermi(x):
    """1 / (1 + exp(x)) without overflow."""
    x = np.asarray(x, dtype=np.float64)
    t = np.exp(-np.abs(x))
    return np.where(x > 0.0, t / (1.0 + t), 1.0 / (1.0 + t))


def transport_coefficients(distribution, temperature, mu):
    """
    ``distribution``: the ``(energies, cumulative, tdf)`` of ``Model.transport_distribution`` (any object with ``energies`` ``(NE,)``
    and ``tdf`` ``(dim, dim, NE - 1)``).  ``temperature``: a positive number or a 1-D array of them; ``mu``: a number or a 1-D array.
    Returns the named tuple ``(T, mu, L0, L1, L2, sigma, seebeck, kappa)``: ``T`` ``(NT,)``, ``mu`` ``(NMU,)``, the tensors
    ``(NT, NMU, dim, dim)``.  ``sigma = L0`` is the conductivity over tau, ``seebeck = -L0^-1 L1 / T`` the thermopower,
    ``kappa = (L2 - L1 L0^-1 L1) / T`` the electronic thermal conductivity over tau at zero electric current.  Where ``L0`` is
    singular (no carriers: mu deep in a gap at low T) ``seebeck`` and ``kappa`` are NaN.

    ``ValueError``: temperatures not positive and finite, mu not finite, or a thermal window ``mu +- 40 T`` that leaves the grid.
    """
    energies = np.asarray(distribution.energies, dtype=np.float64)
    tdf = np.asarray(distribution.tdf, dtype=np.float64)
    if energies.ndim != 1 or tdf.ndim != 3 or tdf.shape[0] != tdf.shape[1] or tdf.shape[2] != energies.shape[0] - 1:
        raise ValueError("distribution must hold energies (NE,) and tdf (dim, dim, NE - 1)")
    temps = np.atleast_1d(np.asarray(temperature, dtype=np.float64))
    mus = np.atleast_1d(np.asarray(mu, dtype=np.float64))
    if temps.ndim != 1 or mus.ndim != 1:
        raise ValueError("temperature and mu must be numbers or 1-D arrays")
    if not np.all(np.isfinite(temps)) or np.any(temps <= 0.0):
        raise ValueError("temperatures must be positive and finite")
    if not np.all(np.isfinite(mus)):
        raise ValueError("mu must be finite")
    if mus.min() - THERMAL_WINDOW * temps.max() < energies[0] or mus.max() + THERMAL_WINDOW * temps.max() > energies[-1]:
        raise ValueError("the thermal window mu +- {:g} T leaves the energy grid [{!r}, {!r}]".format(THERMAL_WINDOW, energies[0], energies[-1]))
    dim = tdf.shape[0]
    mid = 0.5 * (energies[:-1] + energies[1:])
    shape = (temps.shape[0], mus.shape[0], dim, dim)
    L = [np.empty(shape), np.empty(shape), np.empty(shape)]
    for i, t in enumerate(temps):
        for j, m in enumerate(mus):
            occ = _fermi((energies - m) / t)
            window = occ[:-1] - occ[1:]  # the integral of -f' over every bin
            x = mid - m
            for n in range(3):
                L[n][i, j] = tdf @ (window * x ** n)
    seebeck = np.full(shape, np.nan)
    kappa = np.full(shape, np.nan)
    for i, t in enumerate(temps):
        for j in range(mus.shape[0]):
            try:
                inv = np.linalg.inv(L[0][i, j])
            except np.linalg.LinAlgError:
                continue
            if not np.all(np.isfinite(inv)):
                continue
            seebeck[i, j] = -(inv @ L[1][i, j]) / t
            kappa[i, j] = (L[2][i, j] - L[1][i, j] @ inv @ L[1][i, j]) / t
    return TransportCoefficients(temps, mus, L[0], L[1], L[2], L[0].copy(), seebeck, kappa)
