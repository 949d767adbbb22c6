"""
Model.pdos on the GPU (csrc/tbk_pdos.hip): the accumulate kernel against its NumPy model (tools/pdos_model.py) on identical
(E, W), unit weights against the density-of-states kernel, the whole call (weights kernel and plumbing) against the model fed with
Model.eigh of the same k list, chunk independence, the sum rule over a partition against Model.dos, bitwise reproducibility,
several handles, and the argument errors.

Bounds.  Accumulate stage on identical inputs: 1e-11 n_orb, the bound of the density-of-states kernel -- the fixed-point worst
case here is 2 n_orb 2^-41 = 9.1e-13 n_orb (fractions and steps are both rounded), 11 times inside it; the rest is a few dozen
roundings per simplex.  Whole call against the model on Model.eigh of the same k list: the same bound, the Jacobi result of a
matrix does not depend on the call shape.  Sum rule against Model.dos: 1e-9 n_orb, the project's whole-call bound (the eigenvalues
come from another solver path).  Every test prints its measured maximum.
"""

import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import pdos_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

MESHES = [(1, 1, 1), (2, 1, 3), (3, 3, 3), (5, 3, 2), (7, 6), (1, 5)]
MAX_GROUPS = _lib.TBK_PDOS_MAX_GROUPS
GROUP_COUNTS = [1, 3, MAX_GROUPS]
# windows for a spectrum inside [-1, 1]: bracketing it, clipping it on both sides, entirely above it, entirely below it
WINDOWS = {"bracket": (-1.25, 1.25), "clip": (-0.4, 0.55), "above": (1.5, 2.5), "below": (-3.0, -1.5)}
SILICON_GROUPS = [[0], [1, 2, 3], [4], [5, 6, 7], [0, 4]]

_INPUTS = {}


def _tile(n_groups):
    """Energy points per LDS tile of pdos_accumulate_kernel (include/tbk.h): 4096 / (n_groups rounded up to a power of two)."""
    group_tile = 1
    while group_tile < n_groups:
        group_tile *= 2
    return 4096 // group_tile


def _random_inputs(mesh, n_orb, n_groups):
    """Seeded eigenvalues in [-1, 1], every row ascending, from 8 orbitals on one flat band (the inputs of test_gpu_dos.py), and
    seeded weights in [0, 1]."""
    key = (mesh, n_orb, n_groups)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * n_orb + 10 * len(mesh) + sum(mesh))
        eig = rng.uniform(-1.0, 1.0, tuple(mesh) + (n_orb,))
        if n_orb >= 8:
            eig[..., 3] = -0.3217
        eig = np.sort(eig, axis=-1)
        weights = np.random.default_rng(77 * n_orb + 7 * n_groups + sum(mesh)).uniform(0.0, 1.0, tuple(mesh) + (n_groups, n_orb))
        eig.setflags(write=False)
        weights.setflags(write=False)
        _INPUTS[key] = (eig, weights)
    return _INPUTS[key]


def _kernel(eig, weights, e_min, step, n_e):
    mesh = np.ascontiguousarray(eig.shape[:-1], dtype=np.int32)
    n_groups = weights.shape[-2]
    nos = np.full((n_groups, n_e), np.nan)
    _lib.check(_lib.lib().tbk_pdos_from_eigensystem(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], n_groups,
                                                    _lib.ptr(np.ascontiguousarray(eig, dtype=np.float64)),
                                                    _lib.ptr(np.ascontiguousarray(weights, dtype=np.float64)), float(e_min), float(step), n_e,
                                                    _lib.ptr(nos)))
    return nos


def _grid(window, n_e):
    lo, hi = window
    step = (hi - lo) / (n_e - 1)
    return lo, step, lo + np.arange(n_e) * step  # the kernel's grid: two roundings per point


def _compare(eig, weights, window, n_e, label):
    lo, step, grid = _grid(window, n_e)
    got = _kernel(eig, weights, lo, step, n_e)
    want = pdos_model.pnos(eig, weights, grid, chunk=512)
    err = np.abs(got - want).max()
    print("%s NE=%d: max|nos - model| = %.3e" % (label, n_e, err))
    assert err <= 1e-11 * eig.shape[-1], (label, n_e, err)
    return got


# ---- 1. the accumulate stage against the model on identical inputs ------------------------------------------------------------
@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
@pytest.mark.parametrize("n_orb", [1, 8, 65])
@pytest.mark.parametrize("mesh", MESHES)
def test_kernel_matches_model_on_every_window(mesh, n_orb, n_groups):
    eig, weights = _random_inputs(mesh, n_orb, n_groups)
    ones = np.ones_like(weights)
    for name, window in WINDOWS.items():
        label = "%s x %d G=%d %s" % (mesh, n_orb, n_groups, name)
        got = _compare(eig, weights, window, 257, label)
        _compare(eig, weights, window, 2, label)
        if name == "below":
            assert np.array_equal(got, np.zeros((n_groups, 257)))
        if name == "above":  # unit weights: every step is exactly 2^40, the integer sums are exact
            lo, step, _ = _grid(window, 257)
            assert np.array_equal(_kernel(eig, ones, lo, step, 257), np.full((n_groups, 257), float(n_orb)))


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
@pytest.mark.parametrize("mesh", MESHES)
def test_kernel_matches_model_at_the_tile_boundary(mesh, n_groups):
    eig, weights = _random_inputs(mesh, 8, n_groups)
    tile = _tile(n_groups)
    for n_e in (tile - 1, tile, tile + 1):
        _compare(eig, weights, WINDOWS["clip"], n_e, "%s x 8 G=%d clip" % (mesh, n_groups))


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
@pytest.mark.parametrize("n_orb, mesh", [(1, (3, 3, 3)), (65, (2, 1, 3)), (65, (1, 5))])
def test_kernel_tile_boundary_at_the_other_orbital_counts(n_orb, mesh, n_groups):
    eig, weights = _random_inputs(mesh, n_orb, n_groups)
    tile = _tile(n_groups)
    for n_e in (tile - 1, tile, tile + 1):
        _compare(eig, weights, WINDOWS["bracket"], n_e, "%s x %d G=%d bracket" % (mesh, n_orb, n_groups))


# ---- 2. unit weights: the density-of-states kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_orb", [1, 8, 65])
@pytest.mark.parametrize("mesh", MESHES)
def test_unit_weights_give_the_density_of_states_kernel(mesh, n_orb):
    eig, _ = _random_inputs(mesh, n_orb, 1)
    mesh_array = np.ascontiguousarray(mesh, dtype=np.int32)
    flat = np.ascontiguousarray(eig)
    for name in ("bracket", "clip"):
        lo, step, _ = _grid(WINDOWS[name], 257)
        total = np.full(257, np.nan)
        _lib.check(_lib.lib().tbk_dos_from_eigenvalues(0, len(mesh), _lib.ptr(mesh_array), n_orb, _lib.ptr(flat), lo, step, 257, _lib.ptr(total)))
        got = _kernel(eig, np.ones(tuple(mesh) + (1, n_orb)), lo, step, 257)
        err = np.abs(got[0] - total).max()
        print("%s x %d %s: max|pdos(W = 1) - dos| = %.3e" % (mesh, n_orb, name, err))
        assert err <= 1e-11 * n_orb


# ---- 3. the weights kernel and the plumbing ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def silicon_model():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])


def _dense(n_orb, n_r, seed, dim=3):
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + seed, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def _whole_call(model, mesh, groups, label, n_e=257):
    eig, vec = model.eigh(dos_model.mesh_kpoints(mesh))
    eig = eig.reshape(tuple(mesh) + (model.size,))
    weights = pdos_model.band_weights(vec, groups).reshape(tuple(mesh) + (len(groups), model.size))
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.1 * span, eig.max() + 0.1 * span, n_e)
    result = model.pdos(mesh, grid, groups)
    assert isinstance(result, tbmodels_amd._model.ProjectedDensityOfStates)
    assert result.energies.shape == (n_e,) and result.nos.shape == (len(groups), n_e) and result.dos.shape == (len(groups), n_e - 1)
    assert np.array_equal(result.energies, grid)
    assert np.array_equal(result.dos, np.diff(result.nos, axis=1) / ((grid[-1] - grid[0]) / (n_e - 1)))
    err = np.abs(result.nos - pdos_model.pnos(eig, weights, grid, chunk=512)).max()
    print("%s %s: max|Model.pdos - model| = %.3e" % (label, mesh, err))
    assert err <= 1e-11 * model.size, (label, mesh, err)
    return result


def test_whole_call_silicon(silicon_model):
    result = _whole_call(silicon_model, (4, 4, 4), SILICON_GROUPS, "silicon")
    # group 4 = orbitals 0 and 4 = groups 0 and 2 together: the same squares, added in another order
    assert np.abs(result.nos[4] - result.nos[0] - result.nos[2]).max() <= 1e-11 * silicon_model.size


def test_whole_call_two_dimensions():
    _whole_call(_dense(3, 5, 1203, dim=2), (7, 6), [[0], [2, 1], [0, 2]], "2-D toy")


# ---- 4. chunk independence ---------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_k_chunk(silicon_model):
    grid = np.linspace(-8.0, 14.0, 257)
    whole = silicon_model.pdos((5, 3, 2), grid, SILICON_GROUPS)
    chunked = pickle.loads(pickle.dumps(silicon_model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 7)  # 30 k-points: chunks straddle the planes of 6, the last one holds 2
    pieces = chunked.pdos((5, 3, 2), grid, SILICON_GROUPS)
    print("k chunk 7 against the default: max|difference| = %.3e" % np.abs(pieces.nos - whole.nos).max())
    assert np.array_equal(pieces.nos, whole.nos)


# ---- 5. the gauge-independent sum rule ---------------------------------------------------------------------------------------------
def _sum_rule(model, mesh, groups, label):
    eig = np.array(model.eigenval_array(dos_model.mesh_kpoints(mesh)))
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.1 * span, eig.max() + 0.1 * span, 257)
    parts = model.pdos(mesh, grid, groups)
    total = model.dos(mesh, grid)
    err = np.abs(parts.nos.sum(axis=0) - total.nos).max()
    print("%s %s: max|sum over the partition - Model.dos| = %.3e" % (label, mesh, err))
    assert err <= 1e-9 * model.size


def test_partition_adds_up_to_the_density_of_states(silicon_model):
    _sum_rule(silicon_model, (4, 4, 4), [[0, 4], [3, 1, 2], [5, 6, 7]], "silicon")
    # 65 orbitals: eigenvectors from rocSOLVER
    _sum_rule(_dense(65, 6, 1202), (2, 2, 2), [list(range(0, 20)), list(range(20, 64)), [64]], "dense 65 orbitals")


# ---- 6. same bits, monotonicity, several handles -----------------------------------------------------------------------------------
def test_same_bits_and_monotonicity(silicon_model):
    grid = np.linspace(-8.0, 14.0, 401)
    first, second = silicon_model.pdos((4, 4, 4), grid, SILICON_GROUPS), silicon_model.pdos((4, 4, 4), grid, SILICON_GROUPS)
    assert np.array_equal(first.nos, second.nos)
    # neighbouring bins each carry at most 2 n_orb 2^-41 of fixed-point rounding
    assert np.all(np.diff(first.nos, axis=1) >= -silicon_model.size * 2.0 ** -39)
    eig, weights = _random_inputs((3, 3, 3), 65, 3)
    lo, step, _ = _grid(WINDOWS["bracket"], 257)
    runs = [_kernel(eig, weights, lo, step, 257) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("mesh", [(4, 4, 4), (5, 3, 2), (1, 4, 5)])
def test_two_handles_agree_with_one(silicon_model, mesh):
    grid = np.linspace(-8.0, 14.0, 257)
    single = silicon_model.pdos(mesh, grid, SILICON_GROUPS)
    twin = pickle.loads(pickle.dumps(silicon_model))
    twin.devices = [0, 0]
    both = twin.pdos(mesh, grid, SILICON_GROUPS)  # n_1 = 1: the second handle's slab is empty
    assert len(twin._handles) == 2
    err = np.abs(both.nos - single.nos).max()
    print("two handles %s: max|difference| = %.3e" % (mesh, err))
    assert err <= 1e-12 * silicon_model.size


def _pdos_timing(handle, reset=0):
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_pdos_timing(handle, ms, ctypes.byref(calls), reset))
    return list(ms), calls.value


def test_timing_getter_counts_the_timed_calls_only():
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    grid, groups = np.linspace(-8.0, 14.0, 257), [[0, 4], [3, 1, 2], [5, 6, 7]]
    model.pdos((4, 4, 4), grid, groups)  # TBK_OPT_TIMING is off: neither time nor a call is booked
    assert _pdos_timing(model._staged()) == ([0.0, 0.0, 0.0], 0)
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.pdos((4, 4, 4), grid, groups)
    model.pdos((4, 4, 4), grid, groups)
    ms, calls = _pdos_timing(model._staged(), reset=1)
    print("two timed calls: %.3f / %.3f / %.3f ms of kernels" % tuple(ms))
    assert calls == 2 and min(ms) > 0.0
    assert _pdos_timing(model._staged()) == ([0.0, 0.0, 0.0], 0)  # the read above reset the sums
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    twin.set_option(_lib.TBK_OPT_TIMING, 1)
    twin.pdos((4, 4, 4), grid, groups)  # one slab per handle
    assert len(twin._handles) == 2
    for handle in twin._staged_all():
        ms, calls = _pdos_timing(handle)
        assert calls == 1 and min(ms) > 0.0


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device(silicon_model, monkeypatch):
    grid = np.linspace(-1.0, 1.0, 11)
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    bad_groups = ([], [[]], [[0], []], [[8]], [[-1]], [[0, 1, 0]], [[0.5]], [[True]], 3, [3], [[0]] * (MAX_GROUPS + 1))
    for groups in bad_groups:
        with pytest.raises(ValueError):
            silicon_model.pdos((4, 4, 4), grid, groups)
    for mesh in ((4, 4), (4, 0, 4), (4, 2.5, 4), 4):  # the checks and the texts of Model.dos
        with pytest.raises(ValueError) as from_pdos:
            silicon_model.pdos(mesh, grid, [[0]])
        with pytest.raises(ValueError) as from_dos:
            silicon_model.dos(mesh, grid)
        assert str(from_pdos.value) == str(from_dos.value)
    for energies in ([0.5], grid[::-1], [0.0, 1.0, np.nan]):
        with pytest.raises(ValueError) as from_pdos:
            silicon_model.pdos((4, 4, 4), energies, [[0]])
        with pytest.raises(ValueError) as from_dos:
            silicon_model.dos((4, 4, 4), energies)
        assert str(from_pdos.value) == str(from_dos.value)
    with pytest.raises(ValueError):
        one_d.pdos((8,), grid, [[0]])


def test_nan_hopping_kdotp_and_the_c_interface():
    nan_model = tbmodels_amd.Model(hop={(0, 0, 0): np.array([[1.0, np.nan], [np.nan, 2.0]], dtype=complex) / 2}, size=2, dim=3,
                                   contains_cc=False)
    with pytest.raises(ValueError):
        nan_model.pdos((2, 2, 2), np.linspace(-1.0, 3.0, 9), [[0], [1]])
    assert not hasattr(tbmodels_amd.KdotpModel, "pdos")

    lib = _lib.lib()
    mesh = np.array([2, 1, 3], dtype=np.int32)
    offsets, orbitals = np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32)
    nos = np.zeros((1, 9))
    # a k.p handle: tbk_kdotp holds the tbk_model of its dense pipeline as its first member (csrc/tbk_internal.h)
    kp = tbmodels_amd.KdotpModel({(0, 0, 0): np.eye(2, dtype=complex), (1, 0, 0): np.array([[0, 1], [1, 0]], dtype=complex)})
    core = ctypes.c_void_p(ctypes.c_void_p.from_address(kp._staged().value).value)
    assert lib.tbk_pdos(core, _lib.ptr(mesh), _lib.ptr(offsets), _lib.ptr(orbitals), 1, -1.0, 0.25, 9, _lib.ptr(nos)) == _lib.TBK_ERR_ARGUMENT
    assert "k.p" in _lib.last_error()

    eig, weights = _random_inputs((2, 1, 3), 8, 3)
    eig, weights = np.ascontiguousarray(eig), np.ascontiguousarray(weights)
    out = np.zeros((3, 9))

    def call(dim=3, mesh_=mesh, n_orb=8, n_groups=3, eig_=eig, weights_=weights, e_min=-1.0, step=0.25, n_e=9, out_=out):
        return lib.tbk_pdos_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, n_groups, _lib.ptr(eig_), _lib.ptr(weights_), e_min, step, n_e,
                                             _lib.ptr(out_))

    assert call() == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=np.array([2, 0, 3], dtype=np.int32)), call(n_e=1), call(step=0.0), call(step=float("nan")),
           call(mesh_=None), call(eig_=None), call(weights_=None), call(out_=None), call(n_orb=0), call(n_groups=0),
           call(n_groups=MAX_GROUPS + 1)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad

    # the groups of the whole call, checked in front of any device work
    g = load_golden("silicon")
    silicon = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    handle = silicon._staged()
    grid_mesh = np.array([2, 2, 2], dtype=np.int32)

    def whole(offsets_, orbitals_, n_groups):
        offsets_, orbitals_ = np.array(offsets_, dtype=np.int32), np.array(orbitals_, dtype=np.int32)
        return lib.tbk_pdos(handle, _lib.ptr(grid_mesh), _lib.ptr(offsets_), _lib.ptr(orbitals_), n_groups, -8.0, 0.5, 9, _lib.ptr(out))

    bad = [whole([0, 0], [0], 1), whole([0, 1], [8], 1), whole([0, 1], [-1], 1), whole([0, 2], [3, 3], 1), whole([1, 2], [0, 1], 1),
           whole([0, 1], [0], 0), whole(list(range(MAX_GROUPS + 2)), list(range(MAX_GROUPS + 1)), MAX_GROUPS + 1)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
