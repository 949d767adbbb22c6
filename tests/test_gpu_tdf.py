"""
The transport distribution on the GPU (csrc/tbk_tdf.hip): the weights kernels against tools/tdf_model.py
`channels` on identical (E, U, D), the accumulate stage of the projected density of states on the scaled channels against
`tdf_model.cumulative`, and `Model.transport_distribution` against the model fed with the eigensystem `Model.eigh` returns, against
its sum rule and its symmetry, with the identities of bits asserted as such.

Bound: tdf_model.tolerance -- derived from the number formats, the orbital count, the Frobenius norms of D^a and the
scales; nothing measured on the kernels enters it.  Every case prints its measured error over the bound.
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
import optics_model  # noqa: E402  pylint: disable=wrong-import-position
import tdf_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

U_ROUND = 2.0 ** -53
DELTA = 1e-8
_CACHE = {}


def _inputs(n, dim, n_k, near):
    """15.6's kind of eigensystem: random ascending bands, a random unitary U, a random Hermitian D^a per axis.  Planted: the pair
    (1, 2) tied exactly (from 3 orbitals; `near`: 1e-12 apart instead) and, from 6 orbitals, the pair (4, 5) 1e-12 apart (`near`: tied).
    Shared by the cases and never written."""
    key = (n, dim, n_k, near)
    if key not in _CACHE:
        rng = np.random.default_rng(7100 + 1000 * dim + 17 * n + n_k)
        E = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
        planted = np.zeros((n_k, n, n), dtype=bool)
        if n >= 3:
            E[:, 2] = E[:, 1] + (1e-12 if near else 0.0)
            planted[:, 1, 2] = planted[:, 2, 1] = True
        if n >= 6:
            E[:, 5] = E[:, 4] + (0.0 if near else 1e-12)
            planted[:, 4, 5] = planted[:, 5, 4] = True
        assert np.all(np.diff(E, axis=-1) >= 0.0)
        # no pair gap of the inputs lies in (DELTA / 100, 100 DELTA) apart from the planted ones (which are 0 or 1e-12: below it)
        gaps = np.abs(E[:, :, None] - E[:, None, :])
        free = gaps[~planted & ~np.eye(n, dtype=bool)[None]]
        assert not np.any((free > DELTA / 100.0) & (free < 100.0 * DELTA)) and np.all(free > 100.0 * DELTA), (n, dim, n_k)
        assert np.all((gaps[planted] == 0.0) | ((gaps[planted] > 0.5e-12) & (gaps[planted] < 2e-12)))
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        D = rng.normal(size=(n_k, dim, n, n)) + 1j * rng.normal(size=(n_k, dim, n, n))
        D = (D + D.conj().transpose(0, 1, 3, 2)) / 2.0
        arrays = tuple(np.ascontiguousarray(a) for a in (E, U.astype(np.complex128), D))
        for array in arrays:
            array.setflags(write=False)
        _CACHE[key] = arrays
    return _CACHE[key]


def _norms(D):
    return np.sqrt((np.abs(D) ** 2).sum(axis=(-1, -2))).max(axis=0)


def _scales_of(D):
    """Powers of two above the channels' bounds from the Frobenius norms of the D^a at hand (||V||_2 <= ||D||_F)."""
    B = _norms(D)
    dim = len(B)
    bounds = [B[a] ** 2 for a in range(dim)] + [(B[a] + B[c]) ** 2 for a, c in tdf_model.pairs(dim)]
    return np.array([tdf_model.power_of_two_above(1.0000001 * b) for b in bounds])


def _kernel(E, U, D, delta, scale):
    n_k, dim, n = D.shape[0], D.shape[1], D.shape[2]
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    out = np.full((n_k, len(scale), n), np.nan)
    status = _lib.lib().tbk_tdf_weights_from_eigensystem(0, dim, n, n_k, _lib.ptr(E), _lib.ptr(U), _lib.ptr(D), float(delta), _lib.ptr(scale), _lib.ptr(out))
    return status, out


# ---- 1. the weights kernels against the model on the same (E, U, D) ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16, 17, 33, 64, 65])
def test_weights_kernels_match_the_model(n):
    worst = 0.0
    for dim in (2, 3):
        for n_k in (1, 5):
            for near in ((False, True) if 3 <= n < 6 else (False,)):
                E, U, D = _inputs(n, dim, n_k, near)
                scale = _scales_of(D)
                tol = tdf_model.tolerance(n, _norms(D), scale)["channel_weights"][None, :, None]
                for delta in (DELTA, 0.0):
                    where = (n, dim, n_k, near, delta)
                    status, got = _kernel(E, U, D, delta, scale)
                    assert status == _lib.TBK_OK, where + (_lib.last_error(),)
                    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0, where
                    want = tdf_model.channels(E, U, D, delta)
                    ratio = float((np.abs(got * scale[None, :, None] - want) / tol).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, where + (ratio,)
                    again = _kernel(E, U, D, delta, scale)[1]
                    assert np.array_equal(got.view(np.int64), again.view(np.int64)), where + ("a second call differs",)
                if n >= 3:
                    # the mask matters: with delta = 0 the pair 1e-12 apart drops out and the weights of its bands change
                    a, b = _kernel(E, U, D, DELTA, scale)[1], _kernel(E, U, D, 0.0, scale)[1]
                    pair = [1, 2] if near else ([4, 5] if n >= 6 else None)
                    if pair is not None:
                        assert np.abs(a[:, :, pair] - b[:, :, pair]).max() > 1e3 * float((tol / scale[None, :, None]).max()), (n, dim, n_k, near)
    print("n = %d: max error / tol = %.3e" % (n, worst))


def test_a_scale_that_is_too_small_is_an_error():
    for n in (9, 33, 65):  # a fused template with padding, one in two waves per row, the library route
        E, U, D = _inputs(n, 3, 5, False)
        scale = _scales_of(D)
        assert _kernel(E, U, D, DELTA, scale)[0] == _lib.TBK_OK
        small = scale.copy()
        small[4] = 2.0 ** -20  # the pair (0, 2)
        status, _ = _kernel(E, U, D, DELTA, small)
        assert status == _lib.TBK_ERR_ARGUMENT and "channel 4" in _lib.last_error() and "above 1" in _lib.last_error(), (n, status, _lib.last_error())


# ---- 2. the accumulate stage on the scaled channels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(2, 3, 2), (3, 4)])
def test_accumulate_stage_on_the_scaled_channels(mesh):
    dim, n_k, n = len(mesh), int(np.prod(mesh)), 9
    E, U, D = _inputs(n, dim, n_k, False)
    E = E.copy()
    E[0, 0], E[n_k - 1, n - 1] = -1.0, 0.75  # corners on points of the aligned grid
    E = np.sort(E, axis=-1)
    scale = _scales_of(D)
    ch = tdf_model.channels(E, U, D, DELTA)
    scaled = np.ascontiguousarray(ch / scale[None, :, None])
    G = len(scale)
    bound = tdf_model.tolerance(n, _norms(D), scale)["channel_fixed"][:, None]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    for name, e_min, step, n_e in (("aligned", -1.25, 0.125, 21), ("unaligned", -1.1 - np.pi / 100.0, 0.1 * np.sqrt(2.0), 17)):
        grid = e_min + np.arange(n_e) * step
        got = np.full((G, n_e), np.nan)
        _lib.check(_lib.lib().tbk_pdos_from_eigensystem(0, dim, _lib.ptr(mesh32), n, G, _lib.ptr(np.ascontiguousarray(E)), _lib.ptr(scaled), float(e_min),
                                                        float(step), n_e, _lib.ptr(got)))
        want = tdf_model.cumulative(E.reshape(mesh + (n,)), ch.reshape(mesh + (G, n)), grid)
        ratio = float((np.abs(got * scale[:, None] - want) / bound).max())
        print("mesh %s %s grid: accumulate max error / tol = %.3e" % (mesh, name, ratio))
        assert ratio <= 1.0, (mesh, name, ratio)


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------------
def _silicon_sparse():
    """The model and the hoppings it holds, read before the twin stores them as CSR (tests/test_gpu_optics.py)."""
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    r_vec, hop = model.packed_hop()
    model.set_sparse()
    return model, r_vec.astype(np.int64), hop


def _dense(n, dim, seed):
    r_vec, hop, pos = syn.dense_model_arrays(n, 6, syn.MODEL_SEED + seed, dim=dim)
    uc = np.eye(dim) + 0.25 * np.triu(np.ones((dim, dim)), 1)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos, uc=uc)
    r_own, hop_own = model.packed_hop()
    return model, r_own.astype(np.int64), hop_own


CALLS = {
    "dense 9 on 2 x 3 x 2": (lambda: _dense(9, 3, 3100), (2, 3, 2), True),
    "dense 9 on 3 x 4": (lambda: _dense(9, 2, 3101), (3, 4), True),
    "silicon CSR on 4^3": (_silicon_sparse, (4, 4, 4), True),
    "dense 17 on 2 x 3 x 2": (lambda: _dense(17, 3, 3102), (2, 3, 2), False),
}


def _derivative_rounding(r_vec, hop, norm):
    """`extra` of the bound (tests/test_gpu_optics.py): the derivative rows' own rounding, 1e-13 sum_R |R_a| ||hop[R]|| per element at
    most, as a Frobenius norm over G in units of u."""
    weights = np.sqrt((np.abs(hop) ** 2).sum(axis=(1, 2)))
    worst = max(float((np.abs(r_vec[:, a]) * weights).sum()) for a in range(r_vec.shape[1]))
    return 1e-13 * worst * hop.shape[1] / norm / U_ROUND


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("name", list(CALLS))
def test_whole_call(name):
    make, mesh, stable = CALLS[name]
    model, r_vec, hop = make()
    n, dim, n_k = model.size, len(mesh), int(np.prod(mesh))
    kpts = optics_model.mesh_kpoints(mesh)
    E, U = model.eigh(kpts)
    D = optics_model.derivatives(r_vec, hop, kpts)
    grid = np.linspace(float(E.min()) - 0.31, float(E.max()) + 0.47, 41)  # ends above the spectrum
    result = model.transport_distribution(mesh, grid)
    assert isinstance(result, tbmodels_amd.TransportDistribution) and np.array_equal(result.energies, grid)
    N = result.cumulative
    assert N.shape == (dim, dim, 41) and N.dtype == np.float64 and result.tdf.shape == (dim, dim, 40) and np.all(np.isfinite(N))
    assert _bits_equal(N, N.transpose(1, 0, 2)) and _bits_equal(result.tdf, result.tdf.transpose(1, 0, 2)), "not symmetric to the bit"
    assert _bits_equal(result.tdf, np.diff(N, axis=2) / ((grid[-1] - grid[0]) / 40))
    scale = tdf_model.scales(r_vec, hop)
    assert np.array_equal(scale, model._transport_scales())
    norms = _norms(D)
    tol = tdf_model.tolerance(n, norms, scale, _derivative_rounding(r_vec, hop, float(norms.min())))["cumulative"][:, :, None]
    want, _ = tdf_model.transport_distribution(E, U, D, mesh, grid)
    ratio = float((np.abs(N - want) / tol).max())
    # the sum rule: the tetrahedron method's own identity, on the kernel's result
    total = tdf_model.weights(E, U, D).sum(axis=(0, 3)) / n_k
    rule = float((np.abs(N[:, :, -1] - total) / tol[:, :, 0]).max())
    print("%s: max error / tol = %.3e, sum rule / tol = %.3e, max|N| = %.3e" % (name, ratio, rule, np.abs(N).max()))
    assert ratio <= 1.0 and rule <= 1.0, (name, ratio, rule)
    # cartesian=True is the host transform of the plain result
    moved = model.transport_distribution(mesh, grid, cartesian=True)
    cell = np.asarray(model.uc, dtype=float)
    host = np.einsum("ia,ijw,jc->acw", cell, N, cell) / abs(np.linalg.det(cell))
    assert np.allclose(moved.cumulative, host, rtol=1e-13, atol=1e-13 * np.abs(host).max()) and _bits_equal(moved.cumulative, moved.cumulative.transpose(1, 0, 2))
    # a timed call books all three stages and changes no bit
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_tdf_timing(model._staged(), ms, ctypes.byref(calls), 1))
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    timed = model.transport_distribution(mesh, grid)
    model.set_option(_lib.TBK_OPT_TIMING, 0)
    _lib.check(_lib.lib().tbk_tdf_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("%s: derivative H(k) %.3f ms, weights %.3f ms, accumulate + reduce + scan %.3f ms" % (name, ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0 and _bits_equal(timed.cumulative, N)
    if not stable:
        return
    # the bits know neither the chunk, nor the devices, nor the call (sparse models and dense ones on the matrix-vector H(k) kernel)
    for chunk in (1, 5, 0):
        model.set_option(_lib.TBK_OPT_K_CHUNK, chunk)
        assert _bits_equal(model.transport_distribution(mesh, grid).cumulative, N), (name, "TBK_OPT_K_CHUNK", chunk)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.transport_distribution(mesh, grid)
    assert len(twin._handles) == 2 and _bits_equal(two.cumulative, N), (name, "two handles", np.abs(two.cumulative - N).max())


def test_c_argument_errors_on_handles():
    lib = _lib.lib()
    model, _, _ = _dense(9, 3, 3100)
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    powers = np.zeros((1, 3), dtype=np.int32)
    coeffs = np.ascontiguousarray([[[0.5, 0.1j], [-0.1j, -0.5]]], dtype=np.complex128)
    kdotp = ctypes.c_void_p()
    _lib.check(lib.tbk_kdotp_create(0, 3, 2, 1, _lib.ptr(powers), _lib.ptr(coeffs), ctypes.byref(kdotp)))
    try:
        # the tbk_model* of a k.p handle is its first member (tests/test_tetra_arguments.py)
        kp = ctypes.c_void_p(ctypes.c_void_p.from_address(kdotp.value).value)
        mesh, zero = np.array([2, 3, 2], dtype=np.int32), np.array([2, 0, 2], dtype=np.int32)
        scale, out = model._transport_scales(), np.zeros((6, 5))
        nan, inf = float("nan"), float("inf")

        def call(h=handle, mesh_=mesh, e_min=-1.0, step=0.5, n_e=5, delta=1e-8, scale_=scale, out_=out):
            return lib.tbk_transport_distribution(h, _lib.ptr(mesh_), e_min, step, n_e, delta, _lib.ptr(scale_), _lib.ptr(out_))

        def several(handles, count, delta=1e-8):
            return lib.tbk_transport_distribution_multi(handles, count, _lib.ptr(mesh), -1.0, 0.5, 5, delta, _lib.ptr(scale), _lib.ptr(out))

        assert call() == _lib.TBK_OK and call(delta=0.0) == _lib.TBK_OK
        bad = [call(h=None), call(h=kp), call(mesh_=None), call(mesh_=zero), call(step=0.0), call(step=nan), call(n_e=1), call(n_e=2 ** 20 + 1),
               call(e_min=nan), call(e_min=inf), call(delta=-1e-9), call(delta=nan), call(delta=inf), call(scale_=None), call(out_=None),
               call(scale_=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])), call(scale_=np.array([1.0, inf, 1.0, 1.0, 1.0, 1.0])),
               several(twice, 2), several(None, 1), several((ctypes.c_void_p * 1)(kp.value), 1), several((ctypes.c_void_p * 2)(handle.value, kp.value), 2)]
        assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
        # a scale that is too small fails the whole call, naming the channel
        small = scale.copy()
        small[1] = 2.0 ** -30
        assert call(scale_=small) == _lib.TBK_ERR_ARGUMENT and "channel 1" in _lib.last_error()
    finally:
        lib.tbk_kdotp_destroy(kdotp)


def test_doubled_model_on_the_gpu():
    """H (+) H: every band doubly degenerate, the eigensolver picks the basis inside every pair; twice the single model's result."""
    mesh, dim, n = (3, 4), 2, 3
    r_vec, hop, pos = syn.dense_model_arrays(n, 6, syn.MODEL_SEED + 3110, dim=dim)
    double = np.zeros((len(hop), 2 * n, 2 * n), dtype=np.complex128)
    double[:, :n, :n] = hop
    double[:, n:, n:] = hop
    one = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    two = tbmodels_amd.Model.from_packed(r_vec, double, pos=np.concatenate([pos, pos]))
    E = one.eigenval(optics_model.mesh_kpoints(mesh))
    E = np.asarray(E)
    grid = np.linspace(float(E.min()) - 0.2, float(E.max()) + 0.2, 17)
    a, b = one.transport_distribution(mesh, grid).cumulative, two.transport_distribution(mesh, grid).cumulative
    r_own, hop_own = two.packed_hop()
    D = optics_model.derivatives(r_own.astype(np.int64), hop_own, optics_model.mesh_kpoints(mesh))
    tol = tdf_model.tolerance(2 * n, _norms(D), tdf_model.scales(r_own, hop_own))["cumulative"][:, :, None]
    # (as in tests/test_tdf_model.py: the two solves' eigenvalues differ by rounding, which the tetrahedron sum sees over the step)
    shift = 2 * n * U_ROUND * float(np.abs(E).max()) / ((grid[1] - grid[0]) / 4.0) * float(np.abs(b).max())
    ratio = float((np.abs(b - 2.0 * a) / (3.0 * tol + shift)).max())
    print("H (+) H on the GPU: max error / tol = %.3e" % ratio)
    assert ratio <= 1.0
