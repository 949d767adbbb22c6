"""
The transmission of an ensemble of devices: transmission_ensemble_kernel of csrc/tbk_ensemble.hip (and the library route above 64 rows)
against tools/ensemble_model.py on identical principal layers (`tbk_transmission_ensemble_from_matrices`), bit for bit against
`tbk_transmission_from_matrices` called with every sample alone, and `Model.transmission_ensemble` against `Model.transmission`.

Bounds (u = 2^-53), none measured on the code under test: transport_model.tolerance = 4 eps scale per sample,
with rho and iterations of the model's run; kernel against model is held to twice it, and it stays at or below 1e-4 in every case,
which is asserted.  The cases: tools/ensemble_model.py's nine with S = 5 samples, three points and five energies -- every edge of
the templates NP = 16, 32, 64, the library route at N = 65, and an uneven last group of samples.  Every case prints its measured
maximum.
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
import ensemble_model as em  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

Z = em.GPU_Z
S = em.GPU_S
SHAPES = em.GPU_CASES
OWN = [s for s in SHAPES if s[0] * s[1] <= 64]
_CACHE = {}


def _inputs(n, L, M):
    """ensemble_model.gpu_case and the model's results, shared by the cases and never written."""
    key = (n, L, M)
    if key not in _CACHE:
        H00, H01, onsite = em.gpu_case(n, L, M)
        T, its, bound = em.ensemble_function(H00, H01, onsite, Z)
        for array in (H00, H01, onsite, T, its, bound):
            array.setflags(write=False)
        _CACHE[key] = (H00, H01, onsite, T, its, bound)
    return _CACHE[key]


def _ensemble(H00, H01, devices, z, *, k_chunk=0, sample_chunk=0, max_iterations=64, check=True):
    """devices (S, M, N): the on-site form; (S, M, N, N): the matrix form"""
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    devices = np.asarray(devices)
    diagonal = devices.ndim == 3
    devices = np.ascontiguousarray(devices, dtype=np.float64 if diagonal else np.complex128)
    T = np.full((n_k, len(z), devices.shape[0]), np.nan)
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    status = _lib.lib().tbk_transmission_ensemble_from_matrices(
        0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), None if H01 is None else _lib.ptr(np.ascontiguousarray(H01)), devices.shape[1], devices.shape[0],
        None if diagonal else _lib.ptr(devices), _lib.ptr(devices) if diagonal else None, len(z), _lib.ptr(z), max_iterations, k_chunk, sample_chunk,
        _lib.ptr(its), _lib.ptr(T))
    if check:
        _lib.check(status)
        return T, its
    return status


def _single(H00, H01, V, z, *, max_iterations=64):
    """tbk_transmission_from_matrices with one device"""
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    V = np.ascontiguousarray(V, dtype=np.complex128)
    T = np.full((n_k, len(z)), np.nan)
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    _lib.check(_lib.lib().tbk_transmission_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), _lib.ptr(np.ascontiguousarray(H01)), V.shape[0],
                                                         _lib.ptr(V), len(z), _lib.ptr(z), max_iterations, 0, _lib.ptr(its), _lib.ptr(T), None))
    return T, its


# ---- 1. the kernel against the model on the same principal layers ---------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", SHAPES)
def test_kernel_matches_the_model(n, L, M):
    H00, H01, onsite, want, its, bound = _inputs(n, L, M)
    print("(n, L, M) = (%d, %d, %d): bounds %.2e ... %.2e, T up to %.3f, iterations %d ... %d" % (n, L, M, bound.min(), bound.max(), want.max(),
                                                                                               its.min(), its.max()))
    assert np.all(bound <= 1e-4), bound.max()
    for name, devices in (("on-site", onsite), ("matrices", em.expand(onsite))):
        T, count = _ensemble(H00, H01, devices, Z)
        assert T.shape == (3, 5, S) and np.all(np.isfinite(T))
        err = np.abs(T - want)
        print("    %s: max|T - model| = %.2e (bounds %.2e ... %.2e)" % (name, err.max(), 2 * bound.min(), 2 * bound.max()))
        assert np.all(err <= 2 * bound), (n, L, M, name, err, bound)
        assert np.array_equal(count, its), (n, L, M, name, count, its)


# ---- 2. the bits of tbk_transmission with every sample alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", OWN)
def test_every_sample_has_the_bits_of_the_single_device_call(n, L, M):
    H00, H01, onsite, _, its, _ = _inputs(n, L, M)
    dense = em.expand(onsite)
    T, count = _ensemble(H00, H01, onsite, Z)
    assert np.array_equal(count, its)
    for s in range(S):
        alone, alone_its = _single(H00, H01, dense[s], Z)
        assert np.array_equal(T[:, :, s], alone), "sample %d has other bits than tbk_transmission_from_matrices" % s
        assert np.array_equal(alone_its, count)
    matrices, count = _ensemble(H00, H01, dense, Z)
    assert np.array_equal(matrices, T) and np.array_equal(count, its), "the on-site form has other bits than the expanded diagonal"
    holed = np.array(onsite)
    holed[2] = 0.0
    pristine, _ = _single(H00, H01, np.zeros((M, n * L, n * L)), Z)
    got, _ = _ensemble(H00, H01, holed, Z)
    assert np.array_equal(got[:, :, 2], pristine), "an all-zero sample against the pristine device"
    assert np.array_equal(got[:, :, [0, 1, 3, 4]], T[:, :, [0, 1, 3, 4]])


# ---- 3. the bits of a (k, z, s) depend on nothing else --------------------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", OWN)
def test_bits_do_not_depend_on_groups_chunks_lists_or_neighbours(n, L, M):
    H00, H01, onsite, _, its, _ = _inputs(n, L, M)
    base, _ = _ensemble(H00, H01, onsite, Z)
    for sample_chunk in (0, 1, 2, S):
        for k_chunk in (0, 1, 2):
            T, count = _ensemble(H00, H01, onsite, Z, k_chunk=k_chunk, sample_chunk=sample_chunk)
            assert np.array_equal(T, base), "sample_chunk %d, k_chunk %d changed bits" % (sample_chunk, k_chunk)
            assert np.array_equal(count, its), (sample_chunk, k_chunk)
    again, _ = _ensemble(H00, H01, onsite, Z)
    assert np.array_equal(again, base), "two calls differ"
    order = [3, 0, 4, 2, 1]
    moved, count = _ensemble(H00, H01, onsite[order], Z, sample_chunk=2)
    assert np.array_equal(moved, base[:, :, order]) and np.array_equal(count, its), "a permuted sample list does not permute the outputs"
    for index in (0, 3, S - 1):
        alone, count = _ensemble(H00, H01, onsite[index:index + 1], Z)
        assert np.array_equal(alone[:, :, 0], base[:, :, index]) and np.array_equal(count, its), "a sample alone has other bits"
    moved, count = _ensemble(H00, H01, onsite, Z[order])
    assert np.array_equal(moved, base[:, order]) and np.array_equal(count, its[:, order]), "a reordered energy list changed bits"
    rows = [2, 0]  # the k list reordered and shortened
    fewer, count = _ensemble(H00[rows], H01[rows], onsite, Z, k_chunk=1)
    assert np.array_equal(fewer, base[rows]) and np.array_equal(count, its[rows]), "a point's bits depend on its neighbours"


# ---- 4. the library route ---------------------------------------------------------------------------------------------------------------
def test_library_route_above_64_rows():
    n, L, M = 13, 5, 2
    H00, H01, onsite, want, its, bound = _inputs(n, L, M)
    dense = em.expand(onsite)
    T, count = _ensemble(H00, H01, onsite, Z, k_chunk=2)
    assert np.array_equal(count, its) and np.all(np.abs(T - want) <= 2 * bound)
    same = True
    for s in range(S):
        alone, alone_its = _single(H00, H01, dense[s], Z)
        assert np.all(np.abs(T[:, :, s] - alone) <= 2 * bound[:, :, s]) and np.array_equal(alone_its, its)
        same = same and np.array_equal(T[:, :, s], alone)
    print("N = 65: the ensemble's bits %s those of the single-device library calls" % ("are" if same else "are NOT"))


def _scaled(r_vec, hop):
    """the hoppings scaled so that the norms of the full set add up to 2: the spectrum lies in [-2, 2]"""
    total = sum(np.linalg.norm(m, 2) for m in sm.full_hoppings(r_vec, hop).values())
    return hop * (2.0 / total)


def _synthetic(n, dim, n_r):
    r_vec, hop, pos = syn.dense_model_arrays(n, n_r, syn.MODEL_SEED + 2100 + 10 * n + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, _scaled(r_vec, hop), pos=pos), r_vec


def _reference(model, kpar, axis, L, devices):
    """The model's run on principal layers taken from `Model.hamilton` at the 2 L + 1 samples of every in-plane point."""
    kpar = np.asarray(kpar, dtype=float).reshape(len(kpar), -1)
    pts = np.concatenate([sm.sample_points(kp, axis, L, model.dim) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    pairs = [sm.principal(sm.layers_from_samples(h)) for h in ham]
    H00, H01 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return em.ensemble_function(H00, H01, devices, Z)


def _library_calls(model):
    counter = ctypes.c_int64(0)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), _lib.TBK_CNT_LIBRARY_CALLS, ctypes.byref(counter)))  # pylint: disable=protected-access
    return counter.value


def test_forced_library_route_against_the_own_kernel():
    model, _ = _synthetic(5, 3, 30)  # L = 2 along axis 0: 10 rows
    kpar = np.random.default_rng(14).random((3, 2))
    onsite = np.random.default_rng(16).uniform(-0.5, 0.5, (S, 3, 10))
    want, its, bound = _reference(model, kpar, 0, 2, onsite)
    assert np.all(bound <= 1e-4)
    own = model.transmission_ensemble(kpar, Z, onsite, axis=0)
    assert _library_calls(model) == 0
    model.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    library = model.transmission_ensemble(kpar, Z, onsite, axis=0)
    assert _library_calls(model) == 1
    matrices = model.transmission_ensemble(kpar, Z, em.expand(onsite), axis=0)
    same = all(np.array_equal(model.transmission(kpar, Z, axis=0, device=onsite[s]).transmission, library.transmission[:, :, s]) for s in range(S))
    print("library on request: max|T - own kernel| = %.2e, max|T - model| = %.2e; its bits %s those of the single-device library calls"
          % (np.abs(library.transmission - own.transmission).max(), np.abs(library.transmission - want).max(), "are" if same else "are NOT"))
    for got in (library, matrices):
        assert np.all(np.abs(got.transmission - own.transmission) <= 2 * bound)
        assert np.all(np.abs(got.transmission - want) <= 2 * bound)
        assert np.array_equal(got.iterations, its)


# ---- 5. the cap and a singular matrix are statuses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [2, 20, 40, 70])
def test_a_singular_first_layer_in_one_sample_is_named_exactly(size):
    """tests/test_gpu_transport.py's construction: the last orbital does not couple to the neighbouring layers, so et keeps H00 there
    exactly; V_1 of sample 1 alone (as given: the C interface does not ask for a Hermitian V) puts z[1] on that diagonal element at k
    index 2 alone: column size - 1 of z - D_1 is zero there and nowhere else."""
    z = np.array([0.1 + 0.2j, 0.3 + 0.2j, -0.4 - 0.1j])
    H00 = np.zeros((4, size, size), dtype=np.complex128)
    H00[:] = np.diag(np.linspace(-1.0, 1.0, size))
    H00[:, size - 1, size - 1] = 1.0
    H00[2, size - 1, size - 1] = 0.5
    H01 = np.zeros_like(H00)
    H01[:, 0, 0] = 0.7
    V = np.zeros((3, 2, size, size), dtype=np.complex128)
    V[1, 0, size - 1, size - 1] = z[1] - 0.5  # (exact: 0.3 - 0.5 by Sterbenz, and 0.5 + (0.3 - 0.5) is 0.3 again)
    assert 0.5 + V[1, 0, size - 1, size - 1] == z[1]
    for k_chunk, sample_chunk in ((0, 0), (1, 1), (0, 3), (3, 2)):
        status = _ensemble(H00, H01, V, z, k_chunk=k_chunk, sample_chunk=sample_chunk, check=False)
        print("singular first layer:", _lib.last_error())
        assert status == _lib.TBK_ERR_SINGULAR
        assert "Singular matrix" in _lib.last_error() and "k index 2, energy 1 " in _lib.last_error() and _lib.last_error().endswith("sample 1")
    with pytest.raises(np.linalg.LinAlgError):
        _lib.check(status)
    T, _ = _ensemble(H00, H01, V[[0, 2]], z)  # the other samples are regular
    assert np.all(np.isfinite(T))
    H00[2, size - 1, size - 1] = 1.0
    T, _ = _ensemble(H00, H01, V, z)
    assert np.all(np.isfinite(T))


@pytest.mark.parametrize("n, L, M", [(3, 1, 2), (8, 4, 2), (16, 4, 3), (13, 5, 2)])
def test_the_cap_names_the_first_point_that_reached_it(n, L, M):
    H00, H01, onsite, _, its, _ = _inputs(n, L, M)
    order = [1, 2, 4, 0, 3]  # the slowest energies are not the first of the list
    z, its = Z[order], its[:, order]
    cap = int(its.max()) - 1
    k, zi = [int(x[0]) for x in np.nonzero(its > cap)]  # the first in (k, z) order
    assert (k, zi) != (0, 0)
    for k_chunk, sample_chunk in ((0, 0), (1, 2)):
        status = _ensemble(H00, H01, onsite, z, max_iterations=cap, k_chunk=k_chunk, sample_chunk=sample_chunk, check=False)
        message = _lib.last_error()
        print("cap %d:" % cap, message)
        assert status == _lib.TBK_ERR_NO_CONVERGENCE
        assert "k index %d and energy %d " % (k, zi) in message and "%d iterations" % cap in message
    _ensemble(H00, H01, onsite, z, max_iterations=cap + 1)  # the cap itself is enough


# ---- 6. the argument errors of the C interface ------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_interface():
    H00, H01, onsite = _inputs(3, 1, 2)[:3]
    dense = em.expand(onsite)
    assert _ensemble(H00, None, onsite, Z, check=False) == _lib.TBK_ERR_ARGUMENT and "H01" in _lib.last_error()
    assert _ensemble(H00, H01, onsite, [0.3, 0.1j], check=False) == _lib.TBK_ERR_ARGUMENT and "Im z" in _lib.last_error()
    assert _ensemble(H00, H01, onsite, Z, max_iterations=0, check=False) == _lib.TBK_ERR_ARGUMENT
    assert _ensemble(H00, H01, onsite, Z, sample_chunk=-1, check=False) == _lib.TBK_ERR_ARGUMENT and "sample_chunk" in _lib.last_error()
    assert _ensemble(H00, H01, onsite, Z, k_chunk=-1, check=False) == _lib.TBK_ERR_ARGUMENT and "k_chunk" in _lib.last_error()
    T, its = np.zeros((3, 5, S)), np.zeros((3, 5), dtype=np.int32)
    call = _lib.lib().tbk_transmission_ensemble_from_matrices

    def run(N=3, n_k=3, M=2, n_s=S, V=None, diagonal=onsite, out_its=its, out_T=T, H=(H00, H01)):
        return call(0, N, n_k, _lib.ptr(H[0]), _lib.ptr(H[1]), M, n_s, _lib.ptr(V), _lib.ptr(diagonal), 5, _lib.ptr(Z), 64, 0, 0, _lib.ptr(out_its),
                    _lib.ptr(out_T))

    assert run(V=dense) == _lib.TBK_ERR_ARGUMENT and "exactly one of V and onsite" in _lib.last_error()
    assert run(diagonal=None) == _lib.TBK_ERR_ARGUMENT and "exactly one of V and onsite" in _lib.last_error()
    assert run(out_its=None) == _lib.TBK_ERR_ARGUMENT and run(out_T=None) == _lib.TBK_ERR_ARGUMENT
    for M in (0, 4097):
        assert run(M=M) == _lib.TBK_ERR_ARGUMENT and "1 to 4096" in _lib.last_error()
    for n_s in (0, 4097):
        assert run(n_s=n_s) == _lib.TBK_ERR_ARGUMENT and "n_s must be 1 to 4096" in _lib.last_error()
    assert run(n_k=0) == _lib.TBK_ERR_ARGUMENT
    big = np.zeros((1, 1024, 1024), dtype=np.complex128)
    assert run(N=1024, n_k=1, M=9, n_s=2, V=big, diagonal=None, H=(big, big)) == _lib.TBK_ERR_ARGUMENT and "256 MiB" in _lib.last_error()
    assert run(N=1024, n_k=1, M=4096, n_s=9, diagonal=big, H=(big, big)) == _lib.TBK_ERR_ARGUMENT and "256 MiB" in _lib.last_error()
    assert run(N=1025, n_k=1, M=1, n_s=1, diagonal=big, H=(big, big)) == _lib.TBK_ERR_ARGUMENT and "at most 1024" in _lib.last_error()
    assert run() == _lib.TBK_OK  # the same arguments without a fault


# ---- 7. whole calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, dim, n_r, axis, L, M, form", [(6, 3, 8, 2, 1, 3, "matrices"), (5, 3, 30, 0, 2, 2, "on-site"), (24, 2, 5, 1, 1, 2, "on-site")])
def test_whole_call_has_the_bits_of_transmission_per_sample(n, dim, n_r, axis, L, M, form):
    model, r_vec = _synthetic(n, dim, n_r)
    assert max(abs(int(R[axis])) for R in r_vec) == L
    kpar = np.random.default_rng(31 + n).random((3, dim - 1)) - 0.5
    if form == "matrices":
        devices = np.stack([tm.random_device(n * L, M, 177 + n + s) for s in range(S)])
    else:
        devices = np.random.default_rng(78 + n).uniform(-0.5, 0.5, (S, M, n * L))
    want, its, bound = _reference(model, kpar, axis, L, devices)
    assert np.all(bound <= 1e-4)
    got = model.transmission_ensemble(kpar, Z, devices, axis=axis)
    assert len(got) == 7 and got.layers == L and got.length == M and got.samples == S and np.array_equal(got.z, Z) and np.array_equal(got.k, kpar)
    assert got.transmission.shape == (3, 5, S) and got.transmission.dtype == np.float64
    err = np.abs(got.transmission - want)
    print("dense %d orbitals dim %d axis %d L = %d M = %d, %s: max|T - model| = %.2e (bounds %.2e ... %.2e)"
          % (n, dim, axis, L, M, form, err.max(), 2 * bound.min(), 2 * bound.max()))
    assert np.all(err <= 2 * bound)
    assert np.array_equal(got.iterations, its) and got.iterations.dtype == np.int32
    for s in range(S):
        alone = model.transmission(kpar, Z, axis=axis - dim, device=devices[s])
        assert np.array_equal(alone.transmission, got.transmission[:, :, s]), "sample %d has other bits than Model.transmission" % s
        assert np.array_equal(alone.iterations, got.iterations)
    one = model.transmission_ensemble(kpar[2], Z[1], devices[3:4], axis=axis)
    assert one.transmission.shape == (1, 1, 1) and one.transmission[0, 0, 0] == got.transmission[2, 1, 3]


def test_one_dimensional_wire_splits_the_samples_into_groups():
    """NK = 1 and five energies: five (k, z) for a whole device, so the samples are split into groups -- 75 samples, an uneven last
    group wherever two or more share one -- and every sample keeps the bits of Model.transmission."""
    n, M, samples = 40, 1, 75
    rng = np.random.default_rng(41)
    onsite_block = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    onsite_block = (onsite_block + onsite_block.conj().T) / 2
    hopping = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    scale = np.linalg.norm(onsite_block, 2) + 2 * np.linalg.norm(hopping, 2)
    model = tbmodels_amd.Model(hop={(0,): onsite_block / scale * 2, (1,): hopping / scale * 2}, size=n, dim=1, pos=np.zeros((n, 1)), contains_cc=False)
    devices = rng.uniform(-0.5, 0.5, (samples, M, n))
    got = model.transmission_ensemble(None, Z, devices)
    assert got.transmission.shape == (1, 5, samples) and got.layers == 1 and got.samples == samples and np.all(np.isfinite(got.transmission))
    assert np.array_equal(model.transmission_ensemble(None, Z, devices).transmission, got.transmission), "two calls differ"
    for s in range(samples):
        alone = model.transmission(None, Z, device=devices[s])
        assert np.array_equal(alone.transmission, got.transmission[:, :, s]), "sample %d has other bits than Model.transmission" % s
        assert np.array_equal(alone.iterations, got.iterations)
    with pytest.raises(np.linalg.LinAlgError) as raised:
        model.transmission_ensemble(None, Z, devices, max_iterations=2)
    print("the cap:", raised.value)
    assert "k index 0 and energy 0 " in str(raised.value) and "2 iterations" in str(raised.value)
    after = model.transmission_ensemble(None, Z, devices[:7])  # the same model and handle
    assert np.array_equal(after.transmission, got.transmission[:, :, :7])


def test_csr_twin_two_handles_chunks_and_the_timing_row():
    n, dim, axis, L, M = 6, 3, 2, 1, 3
    model, _ = _synthetic(n, dim, 8)
    kpar = np.random.default_rng(5).random((7, dim - 1))
    onsite = np.random.default_rng(6).uniform(-0.5, 0.5, (S, M, n))
    _, _, bound = _reference(model, kpar, axis, L, onsite)
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    one = model.transmission_ensemble(kpar, Z, onsite)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_transmission_ensemble_timing(model._staged(), ms, ctypes.byref(calls), 1))  # pylint: disable=protected-access
    print("6 orbitals, 7 points, 5 energies, 3 layers, 5 samples: H(k) and layers %.3f ms, decimation and sweeps %.3f ms, output %.3f ms" % (ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_transmission_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0
    _lib.check(_lib.lib().tbk_transmission_ensemble_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0, "the row was not reset"
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    other = sparse.transmission_ensemble(kpar, Z, onsite)
    assert np.all(np.abs(other.transmission - one.transmission) <= 2 * bound), "CSR against dense"
    assert np.array_equal(other.iterations, one.iterations)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.transmission_ensemble(kpar, Z, onsite)
    assert len(twin._handles) == 2  # pylint: disable=protected-access
    chunked = pickle.loads(pickle.dumps(model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 3)
    three = chunked.transmission_ensemble(kpar, Z, onsite)
    for name, other in (("two handles", two), ("chunks of 3 points", three)):  # the bits of a (k, z, s) depend on nothing else
        assert np.array_equal(other.iterations, one.iterations), name
        assert np.array_equal(other.transmission, one.transmission), name + ": other bits than one call"
