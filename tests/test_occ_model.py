"""
tools/occ_model.py, the statement csrc/tbk_occ.hip is tested against: the gather over the simplices that
contain a mesh point equals the scatter over the simplices of every cell, and both equal the exact rational point weights.

Bounds.  Model against exact: 1e-14 in NK w, the model-against-exact bound of DESIGN 10.5 (measured here: a few 1e-16).  Sum of the
weights against `dos_model.nos`: 1e-13.  No GPU.
"""

import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import occ_model  # noqa: E402  pylint: disable=wrong-import-position
import tetra_exact as exact  # noqa: E402  pylint: disable=wrong-import-position

MESHES = [(2, 2, 2), (3, 2, 1), (3, 3, 2), (3, 2), (1, 5), (1, 1, 1), (2, 1, 1), (4, 4, 4)]


def _energies(eig):
    levels = list(exact.LEVELS)
    between = [(a + b) / 2 for a, b in zip(levels[:-1], levels[1:])]
    above = [float(np.nextafter(x, np.inf)) for x in levels]
    return levels + between + above + [float(eig.min()) - 0.25, float(eig.max()) + 0.25]


def _inputs(mesh):
    return exact.tie_rich_inputs(mesh, 1 if mesh == (4, 4, 4) else 3, 1)[0]


def test_gather_table_counts():
    for dim, entries, points in ((3, 24, 15), (2, 6, 7)):
        table = occ_model.gather_table(dim)
        assert len(table) == entries
        offsets = {off for _, _, corners in table for off in corners}
        assert len(offsets) == points and (0,) * dim in offsets
        for _, p, corners in table:
            assert corners[p] == (0,) * dim
        for off in offsets:  # the non-zero components share one sign
            assert set(off) <= {0, 1} or set(off) <= {0, -1}
        assert len({(sigma, p) for sigma, p, _ in table}) == entries
    with pytest.raises(ValueError):
        occ_model.gather_table(1)


@pytest.mark.parametrize("mesh", MESHES)
def test_gather_equals_scatter_equals_exact(mesh):
    eig = _inputs(mesh)
    n_k = int(np.prod(mesh))
    worst_gs = worst_ge = worst_sum = 0.0
    for mu in _energies(eig):
        gather, scatter = occ_model.point_weights(eig, mu), occ_model.point_weights_scatter(eig, mu)
        want = occ_model.point_weights_exact(eig, mu)
        worst_gs = max(worst_gs, n_k * np.abs(gather - scatter).max())
        worst_ge = max(worst_ge, n_k * np.abs(gather - want).max(), n_k * np.abs(scatter - want).max())
        worst_sum = max(worst_sum, abs(gather.sum() - dos_model.nos(eig, [mu])[0]))
        assert np.all(gather >= 0.0) and np.all(n_k * gather <= 1.0), (mesh, mu)
        if mu < eig.min():
            assert np.all(gather == 0.0) and np.all(scatter == 0.0)
        if mu >= eig.max():
            assert np.all(gather == 1.0 / n_k), (mesh, mu)
    print("%s: NK max|gather - scatter| = %.3e, NK max|model - exact| = %.3e, max|sum w - nos| = %.3e" % (mesh, worst_gs, worst_ge, worst_sum))
    assert worst_gs <= 1e-14 and worst_ge <= 1e-14 and worst_sum <= 1e-13, (mesh, worst_gs, worst_ge, worst_sum)


def test_hand_worked_case_in_fractions():
    """One band on the mesh (2, 2) with the values 0, 1, 2, 3 at mu = 3/2.  The 8 triangles of the mesh are the value sets {0, 2, 3},
    {0, 1, 3}, {1, 2, 3} and {0, 1, 2}, each twice.  With A = (E - e1)^2 / ((e2 - e1)(e3 - e1)) for e1 <= E < e2 the cut-off corner
    triangle gives w2 = A / 3 * (E - e1) / (e2 - e1), w3 = A / 3 * (E - e1) / (e3 - e1), w1 = A - w2 - w3, and with
    B = (e3 - E)^2 / ((e3 - e1)(e3 - e2)) for e2 <= E < e3 the empty corner takes the same from 1/3 each.  By hand:
        {0, 1, 2}: 31/96, 30/96, 23/96      {0, 1, 3}: 26/96, 23/96, 11/96      {0, 2, 3}: 21/96, 9/96, 6/96      {1, 2, 3}: 9/96, 2/96, 1/96
    and w(value) = 2 * (sum over the sets) / (S NK = 8): 13/64, 31/192, 17/192, 3/64, which add up to N(3/2) = 1/2."""
    eig = np.array([[0.0, 1.0], [2.0, 3.0]]).reshape(2, 2, 1)
    want = np.array([[Fraction(13, 64), Fraction(31, 192)], [Fraction(17, 192), Fraction(3, 64)]], dtype=object).reshape(2, 2, 1)
    got = occ_model.point_weights_exact(eig, Fraction(3, 2), as_fractions=True)
    assert np.all(got == want), got
    assert got.sum() == Fraction(1, 2)
    for fn in (occ_model.point_weights, occ_model.point_weights_scatter):
        assert np.abs(fn(eig, 1.5) - want.astype(float)).max() <= 1e-16


def test_occupations_sum_rules_and_a_full_band():
    rng = np.random.default_rng(5)
    mesh, n = (3, 2, 2), 4
    n_k = int(np.prod(mesh))
    eig = np.sort(rng.uniform(-1.0, 1.0, mesh + (n,)), axis=-1)
    eig[..., 0] -= 2.0  # the lowest band lies below the others: full at mu = -0.9
    mu = -0.9
    U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
    w = occ_model.point_weights(eig, mu)
    q, f, eb = occ_model.occupations(w, eig, U)
    assert f[0] == pytest.approx(1.0, abs=1e-15) and np.all(w[..., 0] == 1.0 / n_k)
    assert abs(q.sum() - f.sum()) <= 1e-14 and abs(f.sum() - dos_model.nos(eig, [mu])[0]) <= 1e-13
    assert np.all(f >= 0.0) and np.all(f <= 1.0 + 1e-15)
    assert eb[0] == pytest.approx(eig[..., 0].mean(), abs=1e-14)
    assert occ_model.occupations(w, eig, None)[0] is None
