"""
tools/fermi_model.py -- the exact statement of band edges and Fermi level the GPU tests compare with -- against closed forms written
out by hand.  CPU only.

One band, E = i on the mesh (4, 1).  The axis of one point returns to the same point, so the two triangles of the cell between
mesh points a = E[i] and b = E[i + 1] have the corners (a, b, b) and (a, a, b): filled fractions x^2 and 1 - (1 - x)^2 with
x = (E - a) / (b - a) clamped to [0, 1], mean x.  The cells are [0, 1], [1, 2], [2, 3] and the periodic one between 3 and 0, i.e.
x = E / 3:  N(E) = (clamp(E) + clamp(E - 1) + clamp(E - 2) + clamp(E / 3)) / 4, which is E / 3 on [0, 3].  So mu(n) is the
smallest double >= 3 n.
"""

import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fermi_model  # noqa: E402  pylint: disable=wrong-import-position
import tetra_exact  # noqa: E402  pylint: disable=wrong-import-position


def _clamp(x):
    return min(max(x, Fraction(0)), Fraction(1))


def _closed_form(energy):
    e = Fraction(energy)
    return (_clamp(e) + _clamp(e - 1) + _clamp(e - 2) + _clamp(e / 3)) / 4


LINEAR = np.arange(4.0).reshape(4, 1, 1)


@pytest.mark.parametrize("energy", [-1.0, 0.0, 0.1, 0.5, 1.0, 1.75, 2.0, 2.9, 3.0, 4.0])
def test_nos_of_a_linear_band_is_the_closed_form(energy):
    got = fermi_model.nos_exact(LINEAR, energy)
    assert got == _closed_form(energy)
    assert got == _clamp(Fraction(energy) / 3)
    assert float(got) == tetra_exact.nos(LINEAR, np.array([energy])).nos[0]  # the same number as the reference of the DOS tests


@pytest.mark.parametrize("n", [0.5, 0.25, 0.3, 1.0 / 3.0, 0.999, 2.0 ** -30])
def test_fermi_level_of_a_linear_band_is_the_smallest_double_at_or_above_3n(n):
    mu, lower, upper = fermi_model.fermi_level(LINEAR, n)
    assert mu == lower == upper
    below = np.nextafter(mu, -np.inf)
    assert Fraction(mu) >= 3 * Fraction(n) > Fraction(below)
    assert _closed_form(mu) >= Fraction(n) > _closed_form(below)
    if n in (0.5, 0.25, 2.0 ** -30):
        assert mu == 3 * n  # exact in doubles


def test_band_edges_are_the_extremes_of_every_band():
    rng = np.random.default_rng(3)
    eig = np.sort(rng.normal(size=(3, 4, 5)), axis=-1)
    emin, emax = fermi_model.band_edges(eig)
    assert np.array_equal(emin, eig.reshape(12, 5).min(axis=0)) and np.array_equal(emax, eig.reshape(12, 5).max(axis=0))


def test_two_separated_bands_give_the_midpoint_of_the_gap():
    rng = np.random.default_rng(4)
    eig = np.stack([rng.uniform(-1.0, -0.25, (2, 3, 2)), rng.uniform(0.5, 2.0, (2, 3, 2))], axis=-1)
    mu, lower, upper = fermi_model.fermi_level(eig, 1)
    assert lower == eig[..., 0].max() and upper == eig[..., 1].min() and lower < upper
    assert mu == lower + (upper - lower) / 2
    # half an electron less: inside the lower band, by the search
    mu, lower, upper = fermi_model.fermi_level(eig, 0.5)
    assert mu == lower == upper and eig[..., 0].min() < mu < eig[..., 0].max()
    assert fermi_model.nos_exact(eig, mu) >= Fraction(1, 2) > fermi_model.nos_exact(eig, np.nextafter(mu, -np.inf))


def test_touching_bands_take_the_search_and_return_the_touching_energy():
    eig = np.stack([np.linspace(-1.0, 0.0, 6).reshape(3, 2), np.linspace(0.0, 1.0, 6).reshape(3, 2)], axis=-1)
    assert eig[..., 0].max() == eig[..., 1].min() == 0.0
    assert fermi_model.fermi_level(eig, 1) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("n", [1.0625, 1.5, 2.0])
def test_a_flat_band_returns_its_energy_for_every_n_inside_the_jump(n):
    rng = np.random.default_rng(5)
    flat = 0.375
    eig = np.stack([rng.uniform(-1.0, 0.0, (3, 3)), np.full((3, 3), flat), rng.uniform(1.0, 2.0, (3, 3))], axis=-1)
    # N jumps from 1 to 2 at the flat energy.  n = 2 sits on top of the jump, and there is a gap above the flat band
    # (emax[1] = flat < emin[2]): that filling is the gap case and returns the midpoint instead
    mu, lower, upper = fermi_model.fermi_level(eig, n)
    if n == 2.0:
        assert (lower, upper) == (flat, eig[..., 2].min()) and mu == lower + (upper - lower) / 2
    else:
        assert mu == lower == upper == flat
    assert fermi_model.nos_exact(eig, flat) == 2 and fermi_model.nos_exact(eig, np.nextafter(flat, -np.inf)) == 1


@pytest.mark.parametrize("exponent", [-100, 100])
@pytest.mark.parametrize("n", [0.5, 0.7, 1.0, 1.25])
def test_scaling_by_a_power_of_two_scales_the_fermi_level_exactly(n, exponent):
    rng = np.random.default_rng(6)
    eig = np.sort(rng.uniform(-1.0, 1.0, (3, 2, 2)), axis=-1)
    factor = 2.0 ** exponent
    plain, scaled = fermi_model.fermi_level(eig, n), fermi_model.fermi_level(eig * factor, n)
    assert scaled == tuple(x * factor for x in plain)


def test_the_key_orders_the_doubles():
    values = [-np.inf, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.nextafter(1.0, 2.0), np.inf]
    keys = [fermi_model.key(x) for x in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(fermi_model.key(b) - fermi_model.key(a) == 1 for a, b in [(-0.0, 0.0), (1.0, np.nextafter(1.0, 2.0)), (-5e-324, -0.0)])
    for x in values:
        assert fermi_model.unkey(fermi_model.key(x)) == x and np.signbit(fermi_model.unkey(fermi_model.key(x))) == np.signbit(x)
