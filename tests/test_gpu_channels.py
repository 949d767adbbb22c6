"""
The transmission eigenvalues: transmission_channels_kernel of csrc/tbk_channels.hip against tools/channels_model.py on identical
principal layers (`tbk_transmission_channels_from_matrices`), T and iterations bit for bit against the ensemble's and the
single-device call, every sample against the one-sample call, mpmath, the properties of the output, rank-deficient leads, the
errors, and `Model.transmission_channels`.

Bounds (u = 2^-53), none measured on the code under test: channels_model.tolerance per (k, z, sample) with rho,
iterations and sweeps of the model's run; kernel against model is held to twice it, and it stays at or below 1e-4 in every case,
which is asserted.  sum_n T_n against T: twice transport_model.tolerance.  Against mpmath (tests/golden/channels_mp.npz, N <= 17): 16
times the model's own error or 16 u, in units of transport_model.scale / N; the three largest T_n relative to themselves, 16 times
the model's or 16 N u.  The cases: transport_model.GPU_CASES up to 64 rows with three points and five energies -- every edge of the
templates NP = 16, 32, 64.  The cap of the Jacobi is not provoked here: tests/test_channels_model.py counts the model's sweeps on
every input of this file.  Every case prints its measured maximum.
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
import channels_model as cm  # noqa: E402  pylint: disable=wrong-import-position
import ensemble_model as em  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

U = cm.U_ROUND
Z = cm.GPU_Z
S = cm.GPU_S
SHAPES = cm.GPU_CASES
_CACHE = {}


def _frozen(*arrays):
    for array in arrays:
        array.setflags(write=False)
    return arrays


def _inputs(n, L, M):
    """channels_model.gpu_case and the model's results, shared by the tests and never written."""
    key = (n, L, M)
    if key not in _CACHE:
        H00, H01, V = cm.gpu_case(n, L, M)
        _CACHE[key] = _frozen(H00, H01, V, *cm.channels_function(H00, H01, V, Z))
    return _CACHE[key]


def _channels(H00, H01, devices, z, *, k_chunk=0, sample_chunk=0, max_iterations=64, check=True):
    """devices (S, M, N): the on-site form; (S, M, N, N): the matrix form.  (T [NK][NZ][S], iterations, channels [NK][NZ][S][N])"""
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    devices = np.asarray(devices)
    diagonal = devices.ndim == 3
    devices = np.ascontiguousarray(devices, dtype=np.float64 if diagonal else np.complex128)
    T = np.full((n_k, len(z), devices.shape[0]), np.nan)
    values = np.full((n_k, len(z), devices.shape[0], N), np.nan)
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    status = _lib.lib().tbk_transmission_channels_from_matrices(
        0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), None if H01 is None else _lib.ptr(np.ascontiguousarray(H01)), devices.shape[1], devices.shape[0],
        None if diagonal else _lib.ptr(devices), _lib.ptr(devices) if diagonal else None, len(z), _lib.ptr(z), max_iterations, k_chunk, sample_chunk,
        _lib.ptr(its), _lib.ptr(T), _lib.ptr(values))
    if check:
        _lib.check(status)
        return T, its, values
    return status


def _ensemble(H00, H01, devices, z):
    n_k, N = H00.shape[0], H00.shape[-1]
    devices = np.asarray(devices)
    diagonal = devices.ndim == 3
    devices = np.ascontiguousarray(devices, dtype=np.float64 if diagonal else np.complex128)
    z = np.ascontiguousarray(z, dtype=np.complex128)
    T = np.full((n_k, len(z), devices.shape[0]), np.nan)
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    _lib.check(_lib.lib().tbk_transmission_ensemble_from_matrices(
        0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), _lib.ptr(np.ascontiguousarray(H01)), devices.shape[1], devices.shape[0],
        None if diagonal else _lib.ptr(devices), _lib.ptr(devices) if diagonal else None, len(z), _lib.ptr(z), 64, 0, 0, _lib.ptr(its), _lib.ptr(T)))
    return T, its


def _single(H00, H01, V, z):
    """tbk_transmission_from_matrices with one device"""
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    V = np.ascontiguousarray(V, dtype=np.complex128)
    T = np.full((n_k, len(z)), np.nan)
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    _lib.check(_lib.lib().tbk_transmission_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), _lib.ptr(np.ascontiguousarray(H01)), V.shape[0],
                                                         _lib.ptr(V), len(z), _lib.ptr(z), 64, 0, _lib.ptr(its), _lib.ptr(T), None))
    return T, its


# ---- 1, 2, 5. the kernel against the model, the bits of the existing calls, the properties ------------------------------------------------
@pytest.mark.parametrize("n, L, M", SHAPES)
def test_kernel_matches_the_model(n, L, M):
    H00, H01, V, want, want_t, its, bound, sweeps, bound_t = _inputs(n, L, M)
    N = n * L
    print("(n, L, M) = (%d, %d, %d): bounds %.2e ... %.2e, the model's sweeps %d ... %d, iterations %d ... %d"
          % (n, L, M, bound.min(), bound.max(), sweeps.min(), sweeps.max(), its.min(), its.max()))
    assert np.all(bound <= 1e-4), bound.max()
    base = None
    for k_chunk in (0, 1, 2):
        T, count, values = _channels(H00, H01, V[None], Z, k_chunk=k_chunk)
        assert values.shape == (3, 5, 1, N) and np.all(np.isfinite(values)) and np.all(np.isfinite(T))
        if base is None:
            base = (T, count, values)
            err = np.abs(values[:, :, 0] - want).max(axis=-1)
            print("    max|T_n - model| = %.2e (bounds %.2e ... %.2e), T_n from %.3e to %.6f"
                  % (err.max(), 2 * bound.min(), 2 * bound.max(), values.min(), values.max()))
            assert np.all(err <= 2 * bound), (n, L, M, err, bound)
            assert np.array_equal(count, its), (n, L, M, count, its)
        else:
            assert all(np.array_equal(a, b) for a, b in zip((T, count, values), base)), "k_chunk %d changed bits" % k_chunk
    T, count, values = base
    again = _channels(H00, H01, V[None], Z)
    assert all(np.array_equal(a, b) for a, b in zip(again, base)), "two calls differ"
    # the bits of the existing calls
    ens_t, ens_its = _ensemble(H00, H01, V[None], Z)
    assert np.array_equal(T, ens_t) and np.array_equal(count, ens_its), "T or iterations have other bits than tbk_transmission_ensemble_from_matrices"
    one_t, one_its = _single(H00, H01, V, Z)
    assert np.array_equal(T[:, :, 0], one_t) and np.array_equal(count, one_its), "T or iterations have other bits than tbk_transmission_from_matrices"
    # the properties of the output
    total = values[:, :, 0].sum(axis=-1)
    print("    max|sum T_n - T| = %.2e (bounds from %.2e)" % (np.abs(total - T[:, :, 0]).max(), 2 * bound_t.min()))
    assert np.all(np.abs(total - T[:, :, 0]) <= 2 * bound_t)
    assert np.all(values >= 0.0), "a negative T_n"
    assert np.all(values[:, :, 0] <= 1.0 + 2 * bound[:, :, None])
    assert np.all(np.diff(values, axis=-1) <= 0.0), "not in descending order"


# ---- 3. the groups of samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", cm.GROUP_CASES)
def test_every_sample_has_the_bits_of_the_one_sample_call(n, L, M):
    H00, H01, onsite, matrices = cm.group_case(n, L, M)
    assert onsite.shape[0] == S == 5
    dense = em.expand(onsite)
    for name, devices, expanded in (("on-site", onsite, dense), ("matrices", matrices, matrices)):
        alone = [_channels(H00, H01, expanded[s:s + 1], Z) for s in range(S)]
        for sample_chunk in (0, 1, 2, 5):
            T, count, values = _channels(H00, H01, devices, Z, sample_chunk=sample_chunk)
            assert values.shape == (3, 5, S, n * L)
            for s in range(S):
                assert np.array_equal(values[:, :, s], alone[s][2][:, :, 0]), "%s, sample_chunk %d: sample %d has other bits" % (name, sample_chunk, s)
                assert np.array_equal(T[:, :, s], alone[s][0][:, :, 0]) and np.array_equal(count, alone[s][1])
        if name == "on-site":
            expanded_run = _channels(H00, H01, dense, Z)
            assert all(np.array_equal(a, b) for a, b in zip(expanded_run, (T, count, values))), "the on-site form has other bits than the expanded diagonal"
    ens_t, ens_its = _ensemble(H00, H01, onsite, Z)
    T, count, _ = _channels(H00, H01, onsite, Z)
    assert np.array_equal(T, ens_t) and np.array_equal(count, ens_its)


# ---- 4. mpmath --------------------------------------------------------------------------------------------------------------------------
def test_against_mpmath_up_to_17_rows():
    """The largest |T_n - mp| / (scale / N) of a case is at most 16 max(u, the model's own); the three largest T_n of every (k, z) have
    a relative error of at most 16 times the model's or 16 N u, whichever is larger."""
    data = np.load(os.path.join(ROOT, "tests", "golden", "channels_mp.npz"))
    assert np.array_equal(data["Z"], Z)
    for n, L, M in SHAPES:
        N = n * L
        if N > 17:
            continue
        H00, H01, V, want = _inputs(n, L, M)[:4]
        exact = data["Tn_%d_%d_%d" % (n, L, M)]
        values = _channels(H00, H01, V[None], Z)[2][:, :, 0]
        gpu, model, rel_gpu, rel_model = 0.0, 0.0, 0.0, 0.0
        for k in range(3):
            for i, z in enumerate(Z):
                P = tm.transmission(H00[k], H01[k], V, complex(z))[1]
                unit = tm.scale(H00[k], H01[k], complex(z), P) / N
                gpu = max(gpu, np.abs(values[k, i] - exact[k, i]).max() / unit)
                model = max(model, np.abs(want[k, i] - exact[k, i]).max() / unit)
                top = slice(0, min(3, N))
                rel_gpu = max(rel_gpu, (np.abs(values[k, i] - exact[k, i])[top] / exact[k, i][top]).max())
                rel_model = max(rel_model, (np.abs(want[k, i] - exact[k, i])[top] / exact[k, i][top]).max())
        print("(n, L, M) = (%d, %d, %d): max|T_n - mp| / unit = %.2e on the GPU, %.2e in the model; the three largest relative: %.2e, %.2e"
              % (n, L, M, gpu, model, rel_gpu, rel_model))
        assert gpu <= 16 * max(U, model), (n, L, M, gpu, model)
        assert rel_gpu <= 16 * max(N * U, rel_model), (n, L, M, rel_gpu, rel_model)


# ---- 6. rank-deficient leads ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cm.DEFICIENT_SHAPES)
@pytest.mark.parametrize("N", cm.DEFICIENT_N)
def test_rank_deficient_leads(N, shape):
    """H01 with entries in row 0 and column 0 of a 3-row block (the cross: rank 2 of 3 in both broadenings, two live columns rotated
    beside a zero one, as t or as t^H), and the row and the column alone (rank 1, exact in the right or the left broadening)."""
    H00, H01, V = cm.deficient_case(N, shape)
    want, _, its, bound, _, bound_t = cm.channels_function(H00, H01, V, Z)
    ranks = np.array([[cm.channels(H00[k], H01[k], V, complex(z))[6] for z in Z] for k in range(3)])  # [3][5][2]: (r_R, r_L) of the model
    least = ranks.min(axis=-1)
    live = 2 if shape == "cross" else 1
    assert np.all(bound <= 1e-4) and np.all(least >= live) and np.all(ranks <= 3)
    T, count, values = _channels(H00, H01, V[None], Z)  # no error is raised
    values = values[:, :, 0]
    err = np.abs(values - want).max(axis=-1)
    print("N = %d, %s: the model's ranks (r_R, r_L) %s, T_n[:3] from %s to %s, max|T_n - model| = %.2e (bounds from %.2e)"
          % (N, shape, sorted(set(map(tuple, ranks.reshape(-1, 2).tolist()))), values[:, :, :3].min(axis=(0, 1)), values[:, :, :3].max(axis=(0, 1)),
             err.max(), 2 * bound.min()))
    assert np.array_equal(count, its)
    assert np.all(err <= 2 * bound), "every T_n, the leading ones included, within twice the tolerance of the model"
    assert np.all(values >= 0.0) and np.all(np.diff(values, axis=-1) <= 0.0) and np.all(values[:, :, :live] > 0.0)
    assert np.all(values[:, :, 3:] == 0.0), "rows without hopping along the axis open no channel: exact zeros whatever the rounding"
    assert np.all(np.abs(values.sum(axis=-1) - T[:, :, 0]) <= 2 * bound_t)
    for k in range(3):
        for i in range(len(Z)):  # the entries beyond the model's min(r_R, r_L) are exactly 0.0
            assert np.all(values[k, i, least[k, i]:] == 0.0), (N, shape, k, i, ranks[k, i], values[k, i, :3])
    if live == 1:
        assert np.all(least == 1) and np.all(values[:, :, 1:] == 0.0)


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_c_interface():
    H00, H01, V = _inputs(3, 1, 2)[:3]
    big = np.zeros((1, 65, 65), dtype=np.complex128)
    assert _channels(big, big, np.zeros((1, 1, 65)), Z, check=False) == _lib.TBK_ERR_ARGUMENT
    print("65 rows:", _lib.last_error())
    assert "65 rows" in _lib.last_error() and "at most 64" in _lib.last_error()
    assert _channels(H00, None, V[None], Z, check=False) == _lib.TBK_ERR_ARGUMENT and "H01" in _lib.last_error()
    assert _channels(H00, H01, V[None], Z, sample_chunk=-1, check=False) == _lib.TBK_ERR_ARGUMENT and "sample_chunk" in _lib.last_error()
    T, its = np.zeros((3, 5, 1)), np.zeros((3, 5), dtype=np.int32)
    dense = np.ascontiguousarray(V[None])
    status = _lib.lib().tbk_transmission_channels_from_matrices(0, 3, 3, _lib.ptr(np.ascontiguousarray(H00)), _lib.ptr(np.ascontiguousarray(H01)), 2, 1,
                                                               _lib.ptr(dense), None, 5, _lib.ptr(Z), 64, 0, 0, _lib.ptr(its), _lib.ptr(T), None)
    assert status == _lib.TBK_ERR_ARGUMENT and "channels is NULL" in _lib.last_error()
    # the cap of the decimation: the ensemble's message
    want_its = _inputs(3, 1, 2)[5]
    cap = int(want_its.max()) - 1
    k, zi = [int(x[0]) for x in np.nonzero(want_its > cap)]
    onsite = np.random.default_rng(5).uniform(-0.5, 0.5, (S, 2, 3))
    for sample_chunk in (0, 2):
        status = _channels(H00, H01, onsite, Z, max_iterations=cap, sample_chunk=sample_chunk, check=False)
        print("cap %d:" % cap, _lib.last_error())
        assert status == _lib.TBK_ERR_NO_CONVERGENCE
        assert "decimation" in _lib.last_error() and "k index %d and energy %d " % (k, zi) in _lib.last_error() and "%d iterations" % cap in _lib.last_error()
    with pytest.raises(np.linalg.LinAlgError):
        _lib.check(_channels(H00, H01, onsite, Z, max_iterations=1, check=False))
    assert "k index 0 and energy 0 " in _lib.last_error()


@pytest.mark.parametrize("size", [2, 20, 40])
def test_a_singular_first_layer_in_one_sample_is_named_exactly(size):
    """tests/test_gpu_ensemble.py's construction: V_1 of sample 1 alone puts z[1] on an uncoupled diagonal element at k index 2."""
    z = np.array([0.1 + 0.2j, 0.3 + 0.2j, -0.4 - 0.1j])
    H00 = np.zeros((4, size, size), dtype=np.complex128)
    H00[:] = np.diag(np.linspace(-1.0, 1.0, size))
    H00[:, size - 1, size - 1] = 1.0
    H00[2, size - 1, size - 1] = 0.5
    H01 = np.zeros_like(H00)
    H01[:, 0, 0] = 0.7
    V = np.zeros((3, 2, size, size), dtype=np.complex128)
    V[1, 0, size - 1, size - 1] = z[1] - 0.5
    assert 0.5 + V[1, 0, size - 1, size - 1] == z[1]
    for k_chunk, sample_chunk in ((0, 0), (1, 1), (3, 2)):
        status = _channels(H00, H01, V, z, k_chunk=k_chunk, sample_chunk=sample_chunk, check=False)
        print("singular first layer:", _lib.last_error())
        assert status == _lib.TBK_ERR_SINGULAR
        assert "Singular matrix" in _lib.last_error() and "k index 2, energy 1 " in _lib.last_error() and _lib.last_error().endswith("sample 1")
    T, _, values = _channels(H00, H01, V[[0, 2]], z)  # the other samples are regular: one open row, one channel
    assert np.all(np.isfinite(T)) and np.all(values[..., 1:] == 0.0) and np.all(values[..., 0] > 0.0)


# ---- 8. whole calls -------------------------------------------------------------------------------------------------------------------
def _reference(model, kpar, axis, L, devices):
    """The model's run on principal layers taken from `Model.hamilton` at the 2 L + 1 samples of every in-plane point:
    (T_n [NK][NZ][S][N], T [NK][NZ][S], iterations, bound [NK][NZ][S])"""
    kpar = np.asarray(kpar, dtype=float).reshape(len(kpar), -1)
    pts = np.concatenate([sm.sample_points(kp, axis, L, model.dim) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    pairs = [sm.principal(sm.layers_from_samples(h)) for h in ham]
    H00, H01 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    runs = [cm.channels_function(H00, H01, V, Z) for V in devices]
    return (np.stack([r[0] for r in runs], axis=2), np.stack([r[1] for r in runs], axis=2), runs[0][2], np.stack([r[3] for r in runs], axis=2))


def _check_whole_call(model, kpar, axis, L, devices, dense):
    want, want_t, its, bound = _reference(model, kpar, axis, L, dense)
    assert np.all(bound <= 1e-4)
    count, M = len(dense), dense.shape[1]
    got = model.transmission_channels(kpar, Z, axis=axis, devices=devices)
    assert len(got) == 9 and got.layers == L and got.length == M and got.samples == count and np.array_equal(got.z, Z)
    assert got.channels.shape == want.shape and got.transmission.shape == want_t.shape and got.noise.shape == want_t.shape
    err = np.abs(got.channels - want).max(axis=-1)
    print("size %d dim %d axis %d L = %d M = %d S = %d: max|T_n - model| = %.2e (bounds %.2e ... %.2e)"
          % (model.size, model.dim, axis, L, M, count, err.max(), 2 * bound.min(), 2 * bound.max()))
    assert np.all(err <= 2 * bound) and np.array_equal(got.iterations, its)
    assert np.array_equal(got.noise, (got.channels * (1.0 - got.channels)).sum(axis=-1))
    assert np.array_equal(got.transmission, model.transmission_ensemble(kpar, Z, devices, axis=axis).transmission)
    for s in range(count):  # device= is one sample, without the S axis
        one = model.transmission_channels(kpar, Z, axis=axis, device=devices[s])
        assert one.samples == 1 and one.channels.shape == want.shape[:2] + want.shape[3:] and one.transmission.shape == want.shape[:2]
        assert one.noise.shape == want.shape[:2]
        assert np.array_equal(one.channels, got.channels[:, :, s]) and np.array_equal(one.transmission, got.transmission[:, :, s])
        assert np.array_equal(one.transmission, model.transmission(kpar, Z, axis=axis, device=devices[s]).transmission)
        assert np.array_equal(one.noise, got.noise[:, :, s])
    return got


def test_whole_call_on_the_chain():
    t, t_plane = 1.0, 0.3
    model = tbmodels_amd.Model(hop={(0, 1): np.array([[t]]), (1, 0): np.array([[t_plane]])}, size=1, dim=2, pos=np.zeros((1, 2)),
                               contains_cc=False)
    kpar = np.array([[0.17], [-0.4], [0.05]])
    onsite = np.array([[[0.7], [-0.3]], [[0.0], [1.5]]])
    got = _check_whole_call(model, kpar, 1, 1, onsite, em.expand(onsite))
    assert got.channels.shape == (3, 5, 2, 1)
    pristine = model.transmission_channels(kpar, Z, length=3)  # length= pristine layers
    assert pristine.length == 3 and pristine.samples == 1 and pristine.channels.shape == (3, 5, 1) and pristine.noise.shape == (3, 5)
    assert np.array_equal(pristine.transmission, model.transmission(kpar, Z, length=3).transmission)
    assert np.array_equal(pristine.noise, pristine.channels[..., 0] * (1.0 - pristine.channels[..., 0]))


def _scaled(r_vec, hop):
    total = sum(np.linalg.norm(m, 2) for m in sm.full_hoppings(r_vec, hop).values())
    return hop * (2.0 / total)


def test_whole_call_on_a_synthetic_model_two_handles_and_the_timing_row():
    n, dim, axis, L, M = 6, 3, 2, 1, 3
    r_vec, hop, pos = syn.dense_model_arrays(n, 8, syn.MODEL_SEED + 2100 + 10 * n + dim, dim=dim)
    model = tbmodels_amd.Model.from_packed(r_vec, _scaled(r_vec, hop), pos=pos)
    kpar = np.random.default_rng(31 + n).random((3, dim - 1)) - 0.5
    devices = np.stack([tm.random_device(n * L, M, 177 + n + s) for s in range(2)])
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    one = _check_whole_call(model, kpar, axis, L, devices, devices)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_transmission_channels_timing(model._staged(), ms, ctypes.byref(calls), 1))  # pylint: disable=protected-access
    print("H(k) and layers %.3f ms, decimation, sweeps and channels %.3f ms, output %.3f ms in %d calls" % (ms[0], ms[1], ms[2], calls.value))
    assert calls.value == 3 and min(ms) > 0.0  # the ensemble call and the two device= calls of _check_whole_call
    _lib.check(_lib.lib().tbk_transmission_ensemble_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 1, "the ensemble's row counts its own call alone"
    _lib.check(_lib.lib().tbk_transmission_channels_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0, "the row was not reset"
    onsite = np.random.default_rng(78 + n).uniform(-0.5, 0.5, (S, M, n * L))
    base = model.transmission_channels(kpar, Z, devices=onsite)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.transmission_channels(kpar, Z, devices=onsite)
    assert len(twin._handles) == 2  # pylint: disable=protected-access
    chunked = pickle.loads(pickle.dumps(model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 2)
    three = chunked.transmission_channels(kpar, Z, devices=onsite)
    for name, other in (("two handles", two), ("chunks of 2 points", three)):
        assert np.array_equal(other.iterations, base.iterations), name
        assert np.array_equal(other.transmission, base.transmission) and np.array_equal(other.channels, base.channels), name + ": other bits"
        assert np.array_equal(other.noise, base.noise)
    with pytest.raises(np.linalg.LinAlgError) as raised:
        model.transmission_channels(kpar, Z, devices=onsite, max_iterations=2)
    assert "decimation" in str(raised.value) and "k index 0 and energy 0 " in str(raised.value)
