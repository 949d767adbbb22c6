"""
The density-of-states kernels (csrc/tbk_dos.hip, csrc/tbk_pdos.hip) against the exact rational reference (tools/tetra_exact.py) at
the places the random inputs of test_gpu_dos.py / test_gpu_pdos.py never reach: tied corners and grid points ON corner energies.

Inputs (tetra_exact.tie_rich_inputs): eigenvalues drawn from five dyadic levels, about 30 % of them moved up by one ulp, rows
sorted; weights uniform in [0, 1].  Grids: the aligned one (-0.75 + j / 16: every E_j exact, every level a grid point), an unaligned
one (-0.7 + 0.11 j), two points, and grids that put two levels on the last bin of an LDS tile and the first of the next.

Coverage is a condition: every parametrised case asserts from the reference's books that its inputs show every tie pattern of the
sorted corners its mesh can show (8 in three dimensions, 4 in two; a mesh of one point has one, and with an axis of ONE point the
step along it returns to the same point, so two corners of every simplex coincide and the pattern without a tie cannot occur),
each with a grid point inside its range, and that grid points equal corners of every rank.

What the grid hits can and cannot show.  n_T and the corner weights are continuous in E wherever two branches meet, so which of two
neighbouring branches a grid point ON a corner takes does not change the value: `E < e2` turned into `E <= e2` gives the same bits
(where e1 = e2 = E it forms 0 * inf, the fixed-point clamp makes that 0, and 0 is the value).  A grid point on a corner is
therefore a test of the arithmetic AT the corner -- the reciprocal of a zero or tiny gap next to a zero distance -- of the step of a
fully tied simplex (the one discontinuity) and of the search on the grid, not of the half-open comparisons between branches.

Bound: 1e-11 n_orb, the accumulate-stage bound of test_gpu_dos.py / test_gpu_pdos.py.  It rests on the fixed-point worst case of
9.1e-13 n_orb (4.5e-13 n_orb for tbk_dos); the floating-point arithmetic in front of it is the models', which
tests/test_tetra_exact.py holds to 1e-14 of exact.  Every case prints its measured maximum.
"""

import os
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import pdos_model  # noqa: E402  pylint: disable=wrong-import-position
import tetra_exact as exact  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

MESHES = [(2, 2, 2), (3, 2, 1), (3, 3, 2), (1, 1, 1), (3, 2), (1, 1)]
ORBITALS = [1, 3, 4]
GROUP_COUNTS = [1, 3, 16]
MAX_GROUPS = 16
TINY = 5e-324
# (e_min, step, n_e).  "two": both points are levels (-0.25 and 0.125)
GRIDS = {"aligned": exact.ALIGNED_GRID, "unaligned": (-0.7, 0.11, 13), "two": (-0.25, 0.375, 2)}

_REFERENCES = {}


def _points(e_min, step, n_e):
    return e_min + np.arange(n_e) * step  # the kernels' grid: two roundings per point


def _inputs(mesh, n_orb, shift=0.0):
    """The seeded tie-rich inputs of a (mesh, n_orb) with 16 groups; a case with G groups takes the first G."""
    eig, weights = exact.tie_rich_inputs(mesh, n_orb, MAX_GROUPS)
    return eig + shift, weights


def _reference(mesh, n_orb, grid, bins=None, shift=0.0, unit=False):
    """The exact values (computed once per module run, never modified): pnos of the 16 groups, or nos for unit=True."""
    key = (mesh, n_orb, grid, None if bins is None else tuple(bins), shift, unit)
    if key not in _REFERENCES:
        eig, weights = _inputs(mesh, n_orb, shift)
        e_min, step, n_e = grid
        points = _points(e_min + shift, step, n_e)
        result = exact.nos(eig, points, bins) if unit else exact.pnos(eig, weights, points, bins)
        result.nos.setflags(write=False)
        _REFERENCES[key] = result
    return _REFERENCES[key]


def _dos_kernel(eig, e_min, step, n_e):
    mesh = np.ascontiguousarray(eig.shape[:-1], dtype=np.int32)
    flat = np.ascontiguousarray(eig, dtype=np.float64)
    nos = np.full(n_e, np.nan)
    _lib.check(_lib.lib().tbk_dos_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), float(e_min), float(step), n_e,
                                                   _lib.ptr(nos)))
    return nos


def _pdos_kernel(eig, weights, e_min, step, n_e):
    mesh = np.ascontiguousarray(eig.shape[:-1], dtype=np.int32)
    n_groups = weights.shape[-2]
    # _lib.ptr is a bare address: the contiguous copies (a slice of the groups is not contiguous) must outlive the call
    flat_e, flat_w = np.ascontiguousarray(eig, dtype=np.float64), np.ascontiguousarray(weights, dtype=np.float64)
    nos = np.full((n_groups, n_e), np.nan)
    _lib.check(_lib.lib().tbk_pdos_from_eigensystem(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], n_groups, _lib.ptr(flat_e), _lib.ptr(flat_w),
                                                    float(e_min), float(step), n_e, _lib.ptr(nos)))
    return nos


def _assert_coverage(mesh, result):
    assert result.patterns_met == exact.possible_tie_patterns(mesh), (mesh, sorted(result.patterns_met))
    assert all(result.rank_hit), (mesh, result.rank_hit)


# ---- 1. both kernels against the exact reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
@pytest.mark.parametrize("n_orb", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_pdos_kernel_matches_exact_at_ties_and_grid_hits(mesh, n_orb, n_groups):
    eig, weights = _inputs(mesh, n_orb)
    weights = weights[..., :n_groups, :]
    _assert_coverage(mesh, _reference(mesh, n_orb, GRIDS["aligned"]))
    for name, grid in GRIDS.items():
        want = _reference(mesh, n_orb, grid).nos[:n_groups]
        got = _pdos_kernel(eig, weights, *grid)
        err = np.abs(got - want).max()  # a NaN in got makes err NaN and the assertion fail
        print("%s x %d G=%d %s: max|pdos - exact| = %.3e" % (mesh, n_orb, n_groups, name, err))
        assert err <= 1e-11 * n_orb, (mesh, n_orb, n_groups, name, err)


@pytest.mark.parametrize("n_orb", ORBITALS)
@pytest.mark.parametrize("mesh", MESHES)
def test_dos_kernel_matches_exact_and_unit_weights_give_it(mesh, n_orb):
    eig, _ = _inputs(mesh, n_orb)
    _assert_coverage(mesh, _reference(mesh, n_orb, GRIDS["aligned"], unit=True))
    for name, grid in GRIDS.items():
        want = _reference(mesh, n_orb, grid, unit=True).nos
        total = _dos_kernel(eig, *grid)
        ones = _pdos_kernel(eig, np.ones(tuple(mesh) + (1, n_orb)), *grid)[0]
        err, err_ones, err_unit = np.abs(total - want).max(), np.abs(ones - want).max(), np.abs(ones - total).max()
        print("%s x %d %s: max|dos - exact| = %.3e, max|pdos(W = 1) - exact| = %.3e, max|pdos(W = 1) - dos| = %.3e"
              % (mesh, n_orb, name, err, err_ones, err_unit))
        assert err <= 1e-11 * n_orb and err_ones <= 1e-11 * n_orb and err_unit <= 1e-11 * n_orb, (mesh, n_orb, name, err, err_ones, err_unit)


# ---- 2. levels on both sides of an LDS tile boundary -------------------------------------------------------------------------------
# step 1/16 and the levels 0.0625, 0.125 on bins (tile - 1, tile): e_min = 0.0625 - (tile - 1) / 16, exact.  The level -0.5 is then
# bin tile - 10 and -0.25 bin tile - 6; below bin tile - 10 nothing is filled.
@pytest.mark.parametrize("mesh", [(2, 2, 2), (3, 2)])
@pytest.mark.parametrize("n_groups, tile, sizes", [(16, 256, (256, 257, 258)), (1, 4096, (4097,))])
def test_levels_on_the_tile_boundary(mesh, n_groups, tile, sizes):
    n_orb = 3
    eig, weights = _inputs(mesh, n_orb)
    weights = weights[..., :n_groups, :]
    e_min, step = 0.0625 - (tile - 1) / 16.0, 2.0 ** -4
    bins = sorted({tile - 10, tile - 6} | set(range(tile - 6, max(sizes))))
    grid = (e_min, step, max(sizes))
    points = _points(*grid)
    assert points[tile - 1] == 0.0625 and points[tile] == 0.125 and points[tile - 10] == -0.5 and points[tile - 6] == -0.25
    parts, total = _reference(mesh, n_orb, grid, bins), _reference(mesh, n_orb, grid, bins, unit=True)
    # the two bins at the boundary hold corner energies and corners of every rank are hit.  The grid lengths are given, so the
    # grid ends at 0.1875, below the level 0.5: a pattern whose simplices only reach a grid point above that cannot be met here
    # (section 1 meets all of them on the same inputs).  Asserted instead: every pattern the aligned grid meets up to the end of
    # this grid is met on the evaluated bins.
    assert all(parts.rank_hit) and np.isin(points[tile - 1], eig) and np.isin(points[tile], eig)
    aligned = _points(*GRIDS["aligned"])
    assert parts.patterns_met == exact.coverage(eig, aligned[aligned <= points[-1]])[1], (mesh, sorted(parts.patterns_met))
    for n_e in sizes:
        keep = [i for i, j in enumerate(bins) if j < n_e]
        cols = [bins[i] for i in keep]
        got = _pdos_kernel(eig, weights, e_min, step, n_e)
        err = np.abs(got[:, cols] - parts.nos[:n_groups][:, keep]).max()
        got_total = _dos_kernel(eig, e_min, step, n_e)
        err_total = np.abs(got_total[cols] - total.nos[keep]).max()
        print("%s x %d G=%d NE=%d: max|pdos - exact| = %.3e, max|dos - exact| = %.3e" % (mesh, n_orb, n_groups, n_e, err, err_total))
        assert err <= 1e-11 * n_orb and err_total <= 1e-11 * n_orb, (mesh, n_groups, n_e, err, err_total)
        # below the lowest level nothing is filled: exact zeros
        assert np.array_equal(got[:, :tile - 10], np.zeros((n_groups, tile - 10))) and np.array_equal(got_total[:tile - 10], np.zeros(tile - 10))


# ---- 3. exact scalings and a shift ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exponent", [-100, 100])
@pytest.mark.parametrize("mesh", [(2, 2, 2), (3, 2)])
def test_scaling_by_a_power_of_two_changes_nothing(mesh, exponent):
    # no coverage assertion of its own: these are the inputs and grids of section 1, whose cases assert it, times a power of two
    n_orb, n_groups = 3, 3
    eig, weights = _inputs(mesh, n_orb)
    weights = weights[..., :n_groups, :]
    factor = 2.0 ** exponent
    for name in ("aligned", "unaligned"):
        e_min, step, n_e = GRIDS[name]
        plain, plain_total = _pdos_kernel(eig, weights, e_min, step, n_e), _dos_kernel(eig, e_min, step, n_e)
        scaled = _pdos_kernel(eig * factor, weights, e_min * factor, step * factor, n_e)
        scaled_total = _dos_kernel(eig * factor, e_min * factor, step * factor, n_e)
        err, err_total = np.abs(scaled - plain).max(), np.abs(scaled_total - plain_total).max()
        print("%s x %d %s scaled by 2^%d: max|pdos - unscaled| = %.3e (same bits: %s), max|dos - unscaled| = %.3e (same bits: %s)"
              % (mesh, n_orb, name, exponent, err, np.array_equal(scaled, plain), err_total, np.array_equal(scaled_total, plain_total)))
        assert err <= 1e-11 * n_orb and err_total <= 1e-11 * n_orb, (mesh, name, exponent, err, err_total)


@pytest.mark.parametrize("mesh", [(2, 2, 2), (3, 3, 2), (3, 2)])
def test_shift_by_two_to_the_twenty(mesh):
    """Eigenvalues and e_min moved by 2^20 on the aligned grid: the search on the grid (dos_first_at_or_above) and the branch
    selection at a magnitude where an ulp is 2^-32.  The grid points and the levels stay exact; an eigenvalue that was one ulp
    above a level rounds onto it, so the reference is computed for the shifted doubles (it is exact for whatever it is given)."""
    n_orb, n_groups, shift = 3, 3, 2.0 ** 20
    eig, weights = _inputs(mesh, n_orb, shift)
    weights = weights[..., :n_groups, :]
    e_min, step, n_e = GRIDS["aligned"]
    assert np.array_equal(_points(e_min + shift, step, n_e) - shift, _points(e_min, step, n_e))
    parts = _reference(mesh, n_orb, GRIDS["aligned"], shift=shift)
    total = _reference(mesh, n_orb, GRIDS["aligned"], shift=shift, unit=True)
    assert all(parts.rank_hit) and parts.patterns_met == exact.all_tie_patterns(len(mesh) + 1), (mesh, sorted(parts.patterns_met))
    err = np.abs(_pdos_kernel(eig, weights, e_min + shift, step, n_e) - parts.nos[:n_groups]).max()
    err_total = np.abs(_dos_kernel(eig, e_min + shift, step, n_e) - total.nos).max()
    print("%s x %d shifted by 2^20: max|pdos - exact| = %.3e, max|dos - exact| = %.3e" % (mesh, n_orb, err, err_total))
    assert err <= 1e-11 * n_orb and err_total <= 1e-11 * n_orb, (mesh, err, err_total)


# ---- 4. a subnormal gap with a grid point on its lower corner ---------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_subnormal_gap_with_a_grid_point_on_its_lower_corner(dim):
    """One simplex has the sorted corners (-0.5, 0, 5e-324, 0.5) (triangle: (-0.5, 0, 5e-324)) and E = 0 is a grid point: the
    reciprocal of the gap e3 - e2 overflows and E - e2 = 0.  The simplex is half full there (the triangle: all but 5e-324 of it)."""
    rng = np.random.default_rng(5)
    mesh = (2,) * dim
    eig = rng.choice(np.array([-0.5, 0.0, TINY, 0.5]), size=mesh + (1,))
    if dim == 3:
        eig[0, 0, 0, 0], eig[1, 0, 0, 0], eig[1, 1, 0, 0], eig[1, 1, 1, 0] = -0.5, 0.0, TINY, 0.5  # the simplex of the axis order (0, 1, 2)
        wanted = (-0.5, 0.0, TINY, 0.5)
    else:
        eig[0, 0, 0], eig[1, 0, 0], eig[1, 1, 0] = -0.5, 0.0, TINY  # the simplex of the axis order (0, 1)
        wanted = (-0.5, 0.0, TINY)
    corners = np.concatenate([np.sort(c.reshape(-1, dim + 1), axis=-1) for c in dos_model.simplex_corners(eig)])
    assert any(tuple(row) == wanted for row in corners)
    weights = rng.uniform(0.0, 1.0, mesh + (3, 1))
    e_min, step, n_e = -0.75, 0.25, 7
    points = _points(e_min, step, n_e)
    assert points[3] == 0.0
    parts, total = exact.pnos(eig, weights, points), exact.nos(eig, points)
    got, got_total = _pdos_kernel(eig, weights, e_min, step, n_e), _dos_kernel(eig, e_min, step, n_e)
    err, err_total = np.abs(got - parts.nos).max(), np.abs(got_total - total.nos).max()
    print("subnormal gap, dim %d: max|pdos - exact| = %.3e, max|dos - exact| = %.3e; at E = 0: dos %.17g, exact %.17g"
          % (dim, err, err_total, got_total[3], total.nos[3]))
    assert err <= 1e-11 and err_total <= 1e-11, (dim, err, err_total)


# ---- 5. the whole call at the Jacobi paddings ---------------------------------------------------------------------------------------
def _uneven_groups(n):
    """16 groups of sizes 1 ... n: all orbitals, one orbital, and 14 overlapping ones (stride 2 from a moving start; n is odd)."""
    groups = [list(range(n)), [n - 1]]
    for g in range(2, MAX_GROUPS):
        size, start = 1 + (5 * g) % n, (3 * g) % n
        groups.append([(start + 2 * i) % n for i in range(size)])
    assert all(len(set(group)) == len(group) for group in groups)
    return groups


@pytest.mark.parametrize("dim, mesh", [(3, (2, 3, 2)), (2, (3, 4))])
@pytest.mark.parametrize("n_orb", [9, 17, 33])  # the Jacobi eigensolver pads them to 16, 32 and 64
def test_whole_call_at_the_jacobi_paddings(n_orb, dim, mesh):
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, 6, syn.MODEL_SEED + 1300 + n_orb, dim=dim)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 5)  # 12 k-points: chunks of 5, 5 and 2 straddle the planes
    groups = _uneven_groups(n_orb)
    eig, vec = model.eigh(dos_model.mesh_kpoints(mesh))
    eig = eig.reshape(tuple(mesh) + (n_orb,))
    weights = pdos_model.band_weights(vec, groups).reshape(tuple(mesh) + (len(groups), n_orb))
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.1 * span, eig.max() + 0.1 * span, 129)
    result = model.pdos(mesh, grid, groups)
    err = np.abs(result.nos - pdos_model.pnos(eig, weights, grid, chunk=512)).max()
    err_sum = np.abs(result.nos[0] - model.dos(mesh, grid).nos).max()
    print("dense %d orbitals %s: max|Model.pdos - model| = %.3e, max|all orbitals - Model.dos| = %.3e" % (n_orb, mesh, err, err_sum))
    assert err <= 1e-11 * n_orb, (n_orb, mesh, err)
    assert err_sum <= 1e-9 * n_orb, (n_orb, mesh, err_sum)
