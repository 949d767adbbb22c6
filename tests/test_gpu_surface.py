"""
The surface Green's function: surface_decimate_kernel of csrc/tbk_surface.hip against tools/surface_model.py on identical principal
layers (`tbk_surface_from_matrices`), and `Model.surface_green_function` against the model on `Model.hamilton`, the chain's closed
form and the fixed points of the decimation.

Bounds (u = 2^-53), none measured on the code under test: surface_model.tolerance,

    8 N u rho (|z| + |H00|_2 + 2 |H01|_2) / eta^2 (iterations + 1)

with rho the growth factor and iterations the count of the model's run.  The inputs have spectra in [-2, 2] and |Im z| >= 0.05, so the
bound stays below 1e-8, which is asserted.  Kernel against model is held to the sum of both bounds (twice the formula); what the
whole call adds -- H(k) and the Fourier extraction of the layers, a few u per element -- disappears in it.  Every case prints its
measured maximum.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

# both signs of Im z, |Im z| in {0.05, 0.5} (test_gpu_dyson.py's Z)
Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])
NK = 5
# (n, L): N = 1, 3, 16, 17, 32, 33, 64 (twice): every edge of the templates NP = 16, 32, 64; N = 65 and 80: the library route
SHAPES = [(1, 1), (3, 1), (8, 2), (17, 1), (8, 4), (11, 3), (16, 4), (64, 1), (13, 5), (40, 2)]
_CACHE = {}


def _inputs(n, L):
    """Principal layers of surface_model.random_case and the model's results, shared by the cases and never written."""
    key = (n, L)
    if key not in _CACHE:
        _, H00, H01 = sm.random_case(n, L, NK, 9100 + 37 * n + L)
        bottom, top, bulk, its, rho = sm.surface_green_function(H00, H01, Z)
        bound = sm.tolerance(H00, H01, Z, its, rho)
        for array in (H00, H01, bottom, top, bulk, its, bound):
            if array is not None:
                array.setflags(write=False)
        _CACHE[key] = (H00, H01, (bottom, top, bulk), its, bound)
    return _CACHE[key]


def _from_matrices(H00, H01, z, *, k_chunk=0, spectral=False, max_iterations=64, check=True):
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    shape = (n_k, len(z), N) if spectral else (n_k, len(z), N, N)
    outs = [np.full(shape, np.nan, dtype=np.float64 if spectral else np.complex128) for _ in range(3)]
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    status = _lib.lib().tbk_surface_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), None if H01 is None else _lib.ptr(np.ascontiguousarray(H01)),
                                                  len(z), _lib.ptr(z), max_iterations, k_chunk, 1 if spectral else 0, _lib.ptr(its), _lib.ptr(outs[0]),
                                                  _lib.ptr(outs[1]), _lib.ptr(outs[2]))
    if check:
        _lib.check(status)
        return outs, its
    return status


def _check(got, want, bound, what):
    """max over the matrix axes per (k, z) against the bound of that (k, z); `bound` is already the sum of both sides'"""
    worst = 0.0
    for name, g, w in zip(("bottom", "top", "bulk"), got, want):
        assert np.all(np.isfinite(g.view(float))), (what, name)
        err = np.abs(g - w).reshape(g.shape[0], g.shape[1], -1).max(axis=2)
        assert np.all(err <= bound), (what, name, err, bound)
        worst = max(worst, err.max())
    print("%s: max|difference| = %.2e (bounds %.2e ... %.2e)" % (what, worst, bound.min(), bound.max()))


# ---- 1. the kernel against the model on the same principal layers ---------------------------------------------------------------------
@pytest.mark.parametrize("n, L", SHAPES)
def test_kernel_matches_the_model(n, L):
    H00, H01, want, its, bound = _inputs(n, L)
    assert np.all(bound < 1e-8), bound.max()
    first = None
    for chunk in (0, 1, 2):
        got, count = _from_matrices(H00, H01, Z, k_chunk=chunk)
        _check(got, want, 2 * bound, "n = %d L = %d (N = %d) chunk %d" % (n, L, n * L, chunk))
        assert np.array_equal(count, its), (n, L, chunk, count, its)
        if first is None:
            first = got
            again, _ = _from_matrices(H00, H01, Z, k_chunk=chunk)
            assert all(np.array_equal(a, b) for a, b in zip(got, again)), (n, L, "two calls differ")
        else:
            assert all(np.array_equal(a, b) for a, b in zip(got, first)), (n, L, chunk, "the chunk changed bits")
    print("n = %d L = %d: iterations %d ... %d" % (n, L, its.min(), its.max()))
    diag, count = _from_matrices(H00, H01, Z, spectral=True)
    assert np.array_equal(count, its)
    for d, g in zip(diag, first):
        assert np.array_equal(d, -np.diagonal(g, axis1=-2, axis2=-1).imag / np.pi), (n, L, "spectral=True has other bits")


@pytest.mark.parametrize("n, L", [(3, 1), (17, 1), (16, 4), (13, 5)])
def test_bits_of_an_energy_do_not_depend_on_the_list(n, L):
    H00, H01, _, its, _ = _inputs(n, L)
    base, _ = _from_matrices(H00, H01, Z)
    order = [3, 0, 4, 2, 1]
    moved, count = _from_matrices(H00, H01, Z[order])
    assert all(np.array_equal(m, b[:, order]) for m, b in zip(moved, base)), "a reordered list changed bits"
    assert np.array_equal(count, its[:, order])
    for index in (0, 4):
        alone, _ = _from_matrices(H00, H01, Z[index:index + 1])
        assert all(np.array_equal(a[:, 0], b[:, index]) for a, b in zip(alone, base)), "an energy alone has other bits"
    rows = [4, 2, 0]  # the k list reordered and shortened
    fewer, _ = _from_matrices(H00[rows], H01[rows], Z, k_chunk=2)
    assert all(np.array_equal(f, b[rows]) for f, b in zip(fewer, base)), "a point's bits depend on its neighbours"


def test_no_hopping_between_the_layers():
    _, H00, _ = sm.random_case(19, 0, NK, 77)
    want = np.linalg.inv(Z[None, :, None, None] * np.eye(19) - H00[:, None])
    b, t, m, its, rho = sm.surface_green_function(H00, None, Z)
    bound = sm.tolerance(H00, None, Z, its, rho)
    got, count = _from_matrices(H00, None, Z)
    assert np.all(count == 0)
    _check(got, (want, want, want), 2 * bound, "L = 0, 19 orbitals against numpy.linalg.inv")
    _check(got, (b, t, m), 2 * bound, "L = 0, 19 orbitals against the model")
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- 2. the cap and a singular matrix are statuses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, L", [(3, 1), (8, 4), (11, 3), (13, 5)])
def test_the_cap_names_the_first_point_that_reached_it(n, L):
    H00, H01, _, its, _ = _inputs(n, L)
    order = [1, 2, 4, 0, 3]  # the slowest energies are not the first of the list
    z, its = Z[order], its[:, order]
    cap = int(its.max()) - 1
    k, zi = [int(x[0]) for x in np.nonzero(its > cap)]  # the first in (k, z) order
    assert (k, zi) != (0, 0)
    status = _from_matrices(H00, H01, z, max_iterations=cap, check=False)
    message = _lib.last_error()
    print("cap %d:" % cap, message)
    assert status == _lib.TBK_ERR_NO_CONVERGENCE
    assert "k index %d and energy %d " % (k, zi) in message and "%d iterations" % cap in message
    with pytest.raises(np.linalg.LinAlgError):
        _lib.check(status)
    status = _from_matrices(H00, H01, z, max_iterations=cap, k_chunk=1, check=False)
    assert status == _lib.TBK_ERR_NO_CONVERGENCE and "k index %d and energy %d " % (k, zi) in _lib.last_error()
    _from_matrices(H00, H01, z, max_iterations=cap + 1)  # the cap itself is enough


@pytest.mark.parametrize("size", [2, 20, 40, 70])
def test_a_singular_input_is_named_exactly(size):
    z = np.array([0.1 + 0.2j, 0.3 + 0.2j, -0.4 - 0.1j])
    H00 = np.zeros((4, size, size), dtype=np.complex128)
    H00[:] = np.diag(np.linspace(-1.0, 1.0, size))
    H00[2, size - 1, size - 1] = z[1]  # z 1 - H00 has a zero on its diagonal at k index 2, energy 1
    status = _from_matrices(H00, None, z, check=False)
    print("singular input:", _lib.last_error())
    assert status == _lib.TBK_ERR_SINGULAR
    assert "Singular matrix" in _lib.last_error() and "k index 2 and energy 1 " in _lib.last_error()
    H00[2, size - 1, size - 1] = 1.0
    got, _ = _from_matrices(H00, None, z)
    want = np.linalg.inv(z[None, :, None, None] * np.eye(size) - H00[:, None])
    assert np.abs(got[2] - want).max() <= 8 * size * 2.0 ** -53 * (abs(z).max() + 1) / 0.01  # diagonal matrices: rho = 1


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------
def _scaled(r_vec, hop):
    """the hoppings scaled so that the norms of the full set add up to 2: the spectrum lies in [-2, 2]"""
    total = sum(np.linalg.norm(m, 2) for m in sm.full_hoppings(r_vec, hop).values())
    return hop * (2.0 / total)


def _synthetic(n, dim, n_r):
    r_vec, hop, pos = syn.dense_model_arrays(n, n_r, syn.MODEL_SEED + 2100 + 10 * n + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, _scaled(r_vec, hop), pos=pos), r_vec


def _reference(model, kpar, axis, L):
    """The model's run on principal layers taken from `Model.hamilton` at the 2 L + 1 samples of every in-plane point."""
    kpar = np.asarray(kpar, dtype=float).reshape(len(kpar), -1)
    pts = np.concatenate([sm.sample_points(kp, axis, L, model.dim) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    pairs = [sm.principal(sm.layers_from_samples(h)) for h in ham]
    H00 = np.stack([p[0] for p in pairs])
    H01 = None if L == 0 else np.stack([p[1] for p in pairs])
    bottom, top, bulk, its, rho = sm.surface_green_function(H00, H01, Z)
    return H00, H01, (bottom, top, bulk), its, sm.tolerance(H00, H01, Z, its, rho)


@pytest.mark.parametrize("n, dim, n_r, axis, L", [(6, 3, 8, 2, 1), (5, 3, 30, 0, 2), (24, 2, 5, 1, 1), (3, 3, 60, 1, 3)])
def test_whole_call_matches_the_model_on_hamilton(n, dim, n_r, axis, L):
    model, r_vec = _synthetic(n, dim, n_r)
    assert max(abs(int(R[axis])) for R in r_vec) == L
    kpar = np.random.default_rng(31 + n).random((4, dim - 1)) - 0.5
    _, _, want, its, bound = _reference(model, kpar, axis, L)
    assert np.all(bound < 1e-8)
    got = model.surface_green_function(kpar, Z, axis=axis)
    assert got.layers == L and np.array_equal(got.z, Z) and np.array_equal(got.k, kpar) and got.iterations.dtype == np.int32
    assert got.bottom.shape == (4, 5, n * L, n * L)
    _check((got.bottom, got.top, got.bulk), want, 2 * bound, "dense %d orbitals dim %d axis %d L = %d" % (n, dim, axis, L))
    assert np.array_equal(got.iterations, its)
    negative = model.surface_green_function(kpar, Z, axis=axis - dim)
    assert np.array_equal(negative.bottom, got.bottom)
    diag = model.surface_green_function(kpar, Z, axis=axis, spectral=True)
    assert diag.bottom.shape == (4, 5, n * L) and diag.bottom.dtype == np.float64
    for d, g in zip(diag[4:], got[4:]):
        assert np.array_equal(d, -np.diagonal(g, axis1=-2, axis2=-1).imag / np.pi)
    one = model.surface_green_function(kpar[2], Z[1], axis=axis)
    assert one.bottom.shape == (1, 1, n * L, n * L) and np.array_equal(one.bottom[0, 0], got.bottom[2, 1])


def test_csr_twin_two_handles_and_chunks():
    n, dim, axis, L = 6, 3, 2, 1
    model, _ = _synthetic(n, dim, 8)
    kpar = np.random.default_rng(5).random((7, dim - 1))
    _, _, _, _, bound = _reference(model, kpar, axis, L)
    one = model.surface_green_function(kpar, Z)
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    other = sparse.surface_green_function(kpar, Z)
    _check(other[4:], one[4:], 2 * bound, "CSR against dense")
    assert np.array_equal(other.iterations, one.iterations)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.surface_green_function(kpar, Z)
    assert len(twin._handles) == 2  # pylint: disable=protected-access
    chunked = pickle.loads(pickle.dumps(model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 3)
    three = chunked.surface_green_function(kpar, Z)
    for name, other in (("two handles", two), ("chunks of 3 points", three)):  # the bits of a (k, z) depend on nothing else
        assert np.array_equal(other.iterations, one.iterations), name
        assert all(np.array_equal(a, b) for a, b in zip(other[4:], one[4:])), name + ": other bits than one call"
    # an error in the second handle's slab carries the index of the caller's list
    its = one.iterations
    cap = int(its.max()) - 1
    fast = [int(r) for r in np.nonzero(its.max(axis=1) <= cap)[0]]
    slow = int(np.nonzero(its.max(axis=1) > cap)[0][0])
    assert fast, "every point needs the largest count"
    order = (fast * 4)[:4] + [slow, fast[0], fast[0]]  # the first slab (points 0 ... 3) stays below the cap, point 4 does not
    k, zi = 4, int(np.nonzero(its[slow] > cap)[0][0])
    with pytest.raises(np.linalg.LinAlgError) as raised:
        twin.surface_green_function(kpar[order], Z, max_iterations=cap)
    print("two handles, the cap:", raised.value)
    assert "k index %d and energy %d " % (k, zi) in str(raised.value)


def test_permuted_axes_give_the_same_functions():
    n, n_r = 4, 20
    r_vec, hop, pos = syn.dense_model_arrays(n, n_r, syn.MODEL_SEED + 2190, dim=3)
    hop = _scaled(r_vec, hop)
    last = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)
    first = tbmodels_amd.Model.from_packed(r_vec[:, [2, 0, 1]], hop, pos=pos[:, [2, 0, 1]])  # the stacking axis moved to the front
    kpar = np.random.default_rng(6).random((3, 2))
    a = last.surface_green_function(kpar, Z, axis=-1)
    b = first.surface_green_function(kpar, Z, axis=0)
    _, _, _, _, bound = _reference(last, kpar, 2, a.layers)
    assert a.layers == b.layers == max(abs(int(R[2])) for R in r_vec)
    _check(b[4:], a[4:], 2 * bound, "axis 0 of the permuted model against axis -1")
    assert np.array_equal(a.iterations, b.iterations)


def test_chain_and_fixed_points():
    t_hop, t_plane = 0.8, 0.3
    model = tbmodels_amd.Model(hop={(0, 1): np.array([[t_hop]]), (1, 0): np.array([[t_plane]])}, size=1, dim=2, pos=np.zeros((1, 2)),
                               contains_cc=False)
    kpar = np.array([[0.0], [0.17], [0.5]])
    got = model.surface_green_function(kpar, Z)
    assert got.layers == 1
    H00, H01, _, its, bound = _reference(model, kpar, 1, 1)
    worst = 0.0
    for k in range(3):
        for i, z in enumerate(Z):
            gs, gb = sm.chain_closed_form(complex(z), t_hop, t_plane, kpar[k, 0])
            err = max(abs(got.bottom[k, i, 0, 0] - gs), abs(got.top[k, i, 0, 0] - gs), abs(got.bulk[k, i, 0, 0] - gb))
            zeta = z - 2 * t_plane * np.cos(2 * np.pi * kpar[k, 0])
            own = 64 * 2.0 ** -53 * (abs(zeta) ** 2 + 4 * t_hop ** 2) / abs(1 / gb) / (2 * t_hop ** 2)  # the closed form's rounding
            assert err <= bound[k, i] + own < 1e-8, (k, i, err)
            worst = max(worst, err)
    print("chain: max|G - closed form| = %.2e" % worst)
    # the fixed points on a model with a principal layer of two cells
    model, _ = _synthetic(5, 3, 30)
    kpar = np.random.default_rng(8).random((2, 2))
    got = model.surface_green_function(kpar, Z, axis=0)
    H00, H01, _, _, bound = _reference(model, kpar, 0, got.layers)
    worst = 0.0
    for k in range(2):
        b = np.linalg.norm(H01[k], 2)
        for i, z in enumerate(Z):
            one = z * np.eye(H00.shape[-1])
            sig_b = H01[k] @ got.bottom[k, i] @ H01[k].conj().T
            sig_t = H01[k].conj().T @ got.top[k, i] @ H01[k]
            res = max(np.abs(got.bottom[k, i] - np.linalg.inv(one - H00[k] - sig_b)).max(),
                      np.abs(got.top[k, i] - np.linalg.inv(one - H00[k] - sig_t)).max(),
                      np.abs(got.bulk[k, i] - np.linalg.inv(one - H00[k] - sig_b - sig_t)).max())
            assert res <= (3 + 2 * b * b / z.imag ** 2) * 2 * bound[k, i], (k, i, res)  # test_surface_model.py's argument
            worst = max(worst, res)
    print("fixed points: largest residual %.2e" % worst)


def test_one_dimensional_model():
    rng = np.random.default_rng(3)
    n = 3
    hop = {(0,): None, (1,): None, (2,): None}
    for key in hop:
        hop[key] = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    hop[(0,)] = (hop[(0,)] + hop[(0,)].conj().T) / 4
    r_vec = np.array(sorted(hop))
    mats = _scaled(r_vec, np.array([hop[tuple(r)] for r in r_vec]))
    model = tbmodels_amd.Model.from_packed(r_vec, mats, pos=np.zeros((n, 1)))
    got = model.surface_green_function(None, Z)
    assert got.layers == 2 and got.k.shape == (1, 0) and got.bottom.shape == (1, 5, 6, 6)
    _, _, want, its, bound = _reference(model, np.zeros((1, 0)), 0, 2)
    _check(got[4:], want, 2 * bound, "a 1-D model, L = 2")
    assert np.array_equal(got.iterations, its)
    assert np.array_equal(model.surface_green_function(np.zeros((1, 0)), Z).bottom, got.bottom)


def test_the_cap_raises_and_the_handle_goes_on():
    model, _ = _synthetic(6, 3, 8)
    kpar = np.random.default_rng(9).random((3, 2))
    with pytest.raises(np.linalg.LinAlgError) as raised:
        model.surface_green_function(kpar, Z, max_iterations=2)
    print("the cap:", raised.value)
    assert "k index 0 and energy 0 " in str(raised.value) and "2 iterations" in str(raised.value)
    _, _, want, _, bound = _reference(model, kpar, 2, 1)
    got = model.surface_green_function(kpar, Z)  # the same model and handle
    _check(got[4:], want, 2 * bound, "after the cap, a regular call")
    for bad in ({"axis": 3}, {"axis": 0.5}, {"max_iterations": 0}, {"max_iterations": 5000}):
        with pytest.raises(ValueError):
            model.surface_green_function(kpar, Z, **bad)
    with pytest.raises(ValueError):
        model.surface_green_function(kpar, [0.3, 0.1j])  # a real energy
    with pytest.raises(ValueError):
        model.surface_green_function(np.zeros((2, 3)), Z)
    status = _from_matrices(np.zeros((1, 1025, 1025), dtype=complex), None, Z, check=False)
    assert status == _lib.TBK_ERR_ARGUMENT and "at most 1024" in _lib.last_error()
    # layers below the reach of the stored vectors is refused by the library itself
    outs = [np.zeros((3, 5, 6, 6), dtype=complex) for _ in range(3)]
    its = np.zeros((3, 5), dtype=np.int32)
    status = _lib.lib().tbk_surface_green(model._staged(), 2, 0, _lib.ptr(np.ascontiguousarray(kpar)), 3, 5, _lib.ptr(Z), 64, 0,  # pylint: disable=protected-access
                                          _lib.ptr(its), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]))
    assert status == _lib.TBK_ERR_ARGUMENT and "reaches 1 cells" in _lib.last_error()


def test_surface_calls_are_timed_on_their_own_row():
    model, _ = _synthetic(24, 2, 5)
    kpar = np.linspace(0.0, 0.5, 6)[:, None]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.surface_green_function(kpar, Z, spectral=True)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_surface_timing(model._staged(), ms, ctypes.byref(calls), 1))  # pylint: disable=protected-access
    print("24 orbitals, 6 points, 5 energies: H(k) and layers %.3f ms, decimation %.3f ms, output %.3f ms" % (ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_green_dressed_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0


# ---- 4. the library route: above 64 rows, and on request -----------------------------------------------------------------------------
def _library_calls(model):
    counter = ctypes.c_int64(0)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), _lib.TBK_CNT_LIBRARY_CALLS, ctypes.byref(counter)))  # pylint: disable=protected-access
    return counter.value


def test_forced_library_route_against_the_own_kernel():
    model, _ = _synthetic(5, 3, 30)  # L = 2 along axis 0: 10 rows
    kpar = np.random.default_rng(14).random((4, 2))
    _, _, want, its, bound = _reference(model, kpar, 0, 2)
    own = model.surface_green_function(kpar, Z, axis=0)
    before = _library_calls(model)
    assert before == 0
    model.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    library = model.surface_green_function(kpar, Z, axis=0)
    assert _library_calls(model) == before + 1
    _check(library[4:], own[4:], 2 * bound, "the library route on request against the own kernel")
    _check(library[4:], want, 2 * bound, "the library route on request against the model")
    assert np.array_equal(library.iterations, its)
    diag = model.surface_green_function(kpar, Z, axis=0, spectral=True)
    for d, g in zip(diag[4:], library[4:]):
        assert np.array_equal(d, -np.diagonal(g, axis1=-2, axis2=-1).imag / np.pi)


def test_whole_call_above_64_rows():
    model, r_vec = _synthetic(40, 3, 30)  # L = 2 along axis 0: 80 rows
    kpar = np.random.default_rng(15).random((2, 2))
    _, _, want, its, bound = _reference(model, kpar, 0, 2)
    assert np.all(bound < 1e-8)
    got = model.surface_green_function(kpar, Z, axis=0)
    assert got.layers == 2 and got.bottom.shape == (2, 5, 80, 80) and _library_calls(model) == 1
    _check(got[4:], want, 2 * bound, "dense 40 orbitals L = 2 (80 rows, the library route)")
    assert np.array_equal(got.iterations, its)
