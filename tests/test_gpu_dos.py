"""
Model.dos on the GPU (csrc/tbk_dos.hip): the kernel against its NumPy model (tools/dos_model.py) on identical eigenvalues, the
whole call against the model fed with eigenval_array of the same mesh, sum rule / monotonicity / flat-band step, bitwise
reproducibility, several handles, and the argument errors.

Bounds.  Kernel on identical inputs: 1e-11 n_orb -- the differences are the order of a few dozen roundings per simplex and the
fixed-point resolution of the kernel, 2^-41 per simplex, at most 4.5e-13 n_orb per bin.  Whole call: 1e-9 n_orb --
the internal eigenvalue call may take another shape than eigenval_array and differ at the 1e-13 level (include/tbk.h), which moves
nos by g(E) * 1e-13; any formula or indexing error is of order 1 / NK or larger.
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

pytestmark = pytest.mark.gpu

MESHES = [(1, 1, 1), (2, 1, 3), (3, 3, 3), (5, 3, 2), (4, 4, 4), (7, 6), (1, 5)]
TILE = 4096  # DOS_TILE of csrc/tbk_dos.hip: energy bins per LDS tile
# windows for a spectrum inside [-1, 1]: bracketing it, clipping it on both sides, entirely above it, entirely below it
WINDOWS = {"bracket": (-1.25, 1.25), "clip": (-0.4, 0.55), "above": (1.5, 2.5), "below": (-3.0, -1.5)}

_EIG = {}


def _random_eig(mesh, n_orb):
    """Seeded eigenvalues in [-1, 1], every row ascending; from 8 orbitals on, one band is flat (clean steps)."""
    key = (mesh, n_orb)
    if key not in _EIG:
        rng = np.random.default_rng(1000 * n_orb + 10 * len(mesh) + sum(mesh))
        eig = rng.uniform(-1.0, 1.0, tuple(mesh) + (n_orb,))
        if n_orb >= 8:
            eig[..., 3] = -0.3217
        eig = np.sort(eig, axis=-1)
        eig.setflags(write=False)
        _EIG[key] = eig
    return _EIG[key]


def _kernel(eig, e_min, step, n_e):
    mesh = np.ascontiguousarray(eig.shape[:-1], dtype=np.int32)
    flat = np.ascontiguousarray(eig, dtype=np.float64)
    nos = np.full(n_e, np.nan)
    _lib.check(_lib.lib().tbk_dos_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), float(e_min),
                                                   float(step), n_e, _lib.ptr(nos)))
    return nos


def _compare(eig, window, n_e, label):
    lo, hi = window
    step = (hi - lo) / (n_e - 1)
    grid = lo + np.arange(n_e) * step  # the kernel's grid: two roundings per point
    got = _kernel(eig, lo, step, n_e)
    want = dos_model.nos(eig, grid, chunk=512)
    err = np.abs(got - want).max()
    print("%s NE=%d: max|nos - model| = %.3e" % (label, n_e, err))
    assert err <= 1e-11 * eig.shape[-1], (label, n_e, err)
    return got


# ---- 1. the kernel against the model on identical inputs --------------------------------------------------------------------
@pytest.mark.parametrize("n_orb", [1, 8, 65])
@pytest.mark.parametrize("mesh", MESHES)
def test_kernel_matches_model_on_every_window(mesh, n_orb):
    eig = _random_eig(mesh, n_orb)
    for name, window in WINDOWS.items():
        got = _compare(eig, window, 257, "%s x %d %s" % (mesh, n_orb, name))
        if name == "above":
            assert np.array_equal(got, np.full(257, float(n_orb)))
        if name == "below":
            assert np.array_equal(got, np.zeros(257))


@pytest.mark.parametrize("mesh", MESHES)
def test_kernel_matches_model_on_short_grids_and_at_the_tile_boundary(mesh):
    eig = _random_eig(mesh, 8)
    for n_e in (2, 3, TILE - 1, TILE, TILE + 1):
        _compare(eig, WINDOWS["clip"], n_e, "%s x 8 clip" % (mesh,))
    for n_e in (2, 3):
        _compare(eig, WINDOWS["bracket"], n_e, "%s x 8 bracket" % (mesh,))


@pytest.mark.parametrize("n_orb, mesh", [(1, (4, 4, 4)), (65, (2, 1, 3)), (65, (1, 5))])
def test_kernel_tile_boundary_at_the_other_orbital_counts(n_orb, mesh):
    eig = _random_eig(mesh, n_orb)
    for n_e in (TILE - 1, TILE, TILE + 1):
        _compare(eig, WINDOWS["bracket"], n_e, "%s x %d bracket" % (mesh, n_orb))


@pytest.fixture(scope="module")
def silicon_model():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"]), g


def _mesh_eig(model, mesh):
    eig = model.eigenval_array(dos_model.mesh_kpoints(mesh))
    return np.array(eig).reshape(tuple(mesh) + (model.size,))


@pytest.mark.parametrize("mesh", [(4, 4, 4), (5, 3, 2)])
def test_kernel_matches_model_on_the_gpus_own_silicon_eigenvalues(silicon_model, mesh):
    model, _ = silicon_model
    eig = _mesh_eig(model, mesh)
    lo, hi = eig.min(), eig.max()
    span = hi - lo
    for name, window in (("bracket", (lo - 0.1 * span, hi + 0.1 * span)), ("clip", (lo + 0.3 * span, hi - 0.25 * span))):
        _compare(eig, window, 257, "silicon %s %s" % (mesh, name))


# ---- 2. the whole call against the model ----------------------------------------------------------------------------------------
def _dense(n_orb, n_r, seed, dim=3):
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + seed, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def _whole_call(model, mesh, label, n_e=301):
    eig = _mesh_eig(model, mesh)
    span = eig.max() - eig.min()
    grid = np.linspace(eig.min() - 0.1 * span, eig.max() + 0.1 * span, n_e)
    result = model.dos(mesh, grid)
    assert result.energies.shape == (n_e,) and result.nos.shape == (n_e,) and result.dos.shape == (n_e - 1,)
    assert np.array_equal(result.energies, grid)
    assert np.array_equal(result.dos, np.diff(result.nos) / ((grid[-1] - grid[0]) / (n_e - 1)))
    err = np.abs(result.nos - dos_model.nos(eig, grid, chunk=512)).max()
    print("%s %s: max|Model.dos - model| = %.3e" % (label, mesh, err))
    assert err <= 1e-9 * model.size, (label, mesh, err)
    return result


@pytest.mark.parametrize("mesh", [(6, 6, 6), (5, 4, 3)])
def test_whole_call_silicon(silicon_model, mesh):
    _whole_call(silicon_model[0], mesh, "silicon")


def test_whole_call_dense_sparse_and_two_dimensions():
    small = _dense(8, 12, 1201)
    dense = _whole_call(small, (5, 4, 3), "dense 8 orbitals")
    _whole_call(_dense(65, 6, 1202), (3, 4, 2), "dense 65 orbitals")
    sparse = pickle.loads(pickle.dumps(small))
    sparse.set_sparse()
    csr = _whole_call(sparse, (5, 4, 3), "the same 8 orbitals, sparse")
    assert np.abs(csr.nos - dense.nos).max() <= 1e-9 * 8
    _whole_call(_dense(3, 5, 1203, dim=2), (7, 6), "2-D toy")


# ---- 3. sum rule, monotonicity, the flat-band step ------------------------------------------------------------------------------
def test_sum_rule_and_monotonicity(silicon_model):
    model, _ = silicon_model
    result = _whole_call(model, (5, 4, 3), "silicon sum rule", n_e=513)
    # below / above the spectrum the fractional bins are empty and the integer counts are exact
    assert result.nos[0] == 0.0 and result.nos[-1] == float(model.size)
    # neighbouring bins each carry at most n_orb 2^-41 of fixed-point rounding
    assert np.all(np.diff(result.nos) >= -model.size * 2.0 ** -40)


@pytest.mark.parametrize("dim, mesh", [(3, (3, 2, 4)), (2, (4, 3))])
def test_flat_bands_give_the_exact_step_function(dim, mesh):
    levels = np.array([-0.5, 0.25, 0.25, 1.0])  # a doubly degenerate level
    model = tbmodels_amd.Model(hop={(0,) * dim: np.diag(levels).astype(complex) / 2}, size=4, dim=dim, contains_cc=False)
    grid = np.linspace(-1.0, 1.5, 21) + 0.03  # no grid point within 0.03 of a level
    result = model.dos(mesh, grid)
    want = (levels[None, :] <= grid[:, None]).sum(axis=1).astype(float)
    assert np.array_equal(result.nos, want)


# ---- 4. reproducibility ---------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits(silicon_model):
    model, _ = silicon_model
    grid = np.linspace(-8.0, 14.0, 401)
    first, second = model.dos((6, 6, 6), grid), model.dos((6, 6, 6), grid)
    assert np.array_equal(first.nos, second.nos)
    eig = _random_eig((4, 4, 4), 65)
    lo, hi = WINDOWS["bracket"]
    runs = [_kernel(eig, lo, (hi - lo) / 256, 257) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("mesh", [(6, 6, 6), (5, 4, 3), (1, 4, 5)])
def test_two_handles_agree_with_one(silicon_model, mesh):
    model, _ = silicon_model
    grid = np.linspace(-8.0, 14.0, 257)
    single = model.dos(mesh, grid)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    both = twin.dos(mesh, grid)  # n_1 = 1: the second handle's slab is empty
    assert len(twin._handles) == 2
    err = np.abs(both.nos - single.nos).max()
    print("two handles %s: max|difference| = %.3e" % (mesh, err))
    assert err <= 1e-12 * model.size


def _dos_timing(handle, reset=0):
    ms, calls = ctypes.c_double(-1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_dos_timing(handle, ctypes.byref(ms), ctypes.byref(calls), reset))
    return ms.value, calls.value


def test_timing_getter_counts_the_timed_calls_only():
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    grid = np.linspace(-8.0, 14.0, 257)
    model.dos((4, 4, 4), grid)  # TBK_OPT_TIMING is off: neither time nor a call is booked
    assert _dos_timing(model._staged()) == (0.0, 0)
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.dos((4, 4, 4), grid)
    model.dos((4, 4, 4), grid)
    ms, calls = _dos_timing(model._staged(), reset=1)
    print("two timed calls: %.3f ms of kernels" % ms)
    assert calls == 2 and ms > 0.0
    assert _dos_timing(model._staged()) == (0.0, 0)  # the read above reset the sums
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    twin.set_option(_lib.TBK_OPT_TIMING, 1)
    twin.dos((4, 4, 4), grid)  # one slab per handle
    assert len(twin._handles) == 2
    for handle in twin._staged_all():
        ms, calls = _dos_timing(handle)
        assert calls == 1 and ms > 0.0


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device(silicon_model, monkeypatch):
    model, _ = silicon_model
    grid = np.linspace(-1.0, 1.0, 11)
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    for mesh in ((4, 4), (4, 4, 4, 4), (4, 0, 4), (4, -2, 4), (4, 2.5, 4), (4.0, 4.0, 4.0), 4):
        with pytest.raises(ValueError):
            model.dos(mesh, grid)
    uneven = np.array(grid)
    uneven[5] += 1e-6
    for energies in ([0.5], [], grid[::-1], [0.0, 0.0, 0.0], uneven, grid.reshape(1, -1), [0.0, 1.0, np.nan]):
        with pytest.raises(ValueError):
            model.dos((4, 4, 4), energies)
    with pytest.raises(ValueError):
        one_d.dos((8,), grid)


def test_nan_hopping_kdotp_and_the_c_interface():
    nan_model = tbmodels_amd.Model(hop={(0, 0, 0): np.array([[1.0, np.nan], [np.nan, 2.0]], dtype=complex) / 2}, size=2, dim=3,
                                   contains_cc=False)
    with pytest.raises(ValueError):
        nan_model.dos((2, 2, 2), np.linspace(-1.0, 3.0, 9))
    assert not hasattr(tbmodels_amd.KdotpModel, "dos")

    lib = _lib.lib()
    eig = np.ascontiguousarray(_random_eig((2, 1, 3), 8))
    mesh = np.array([2, 1, 3], dtype=np.int32)
    nos = np.zeros(9)

    def call(dim=3, mesh_=mesh, n_orb=8, eig_=eig, e_min=-1.0, step=0.25, n_e=9, out=nos):
        return lib.tbk_dos_from_eigenvalues(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), e_min, step, n_e, _lib.ptr(out))

    assert call() == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=np.array([2, 0, 3], dtype=np.int32)), call(n_e=1), call(step=0.0), call(step=-0.25),
           call(step=float("nan")), call(step=float("inf")), call(mesh_=None), call(eig_=None), call(out=None), call(n_orb=0)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
