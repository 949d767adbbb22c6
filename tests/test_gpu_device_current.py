"""
The bond currents of the device: the CURRENT instantiation of device_green_kernel (csrc/tbk_device_green.hip) against
tools/current_model.py on identical principal layers (`tbk_device_current_from_matrices`), and `Model.device_current` against the model
on `Model.hamilton`.

Bounds (u = 2^-53), none measured on the code under test: current_model.tolerance, per component

    K^L_p: 2 max|H01| (c(F_p) + c(F_{p+1}) + 1) E s(F_p) s(F_{p+1}) gamma_L      J^L_p: 2 max|H_pp| (2 c(F_p) + 1) E s(F_p)^2 gamma_L
    K^R, J^R: C and gamma_R                                                      current_*: N times K's

with E, c, s and gamma of device_model.tolerance (23.5); kernel against model is held to twice it, and it stays at or below 1e-4 in every
case, which is asserted.  The sharper check: for N <= 17 the largest error against the stored mpmath values
(tests/golden/current_mp.npz, `tools/current_model.py --golden`), in units of the bound without E c, is at most 16 max(u, the model's
own).  The identities 1 - 3 of the model's docstring are held on the kernel's outputs to the sum of the bounds of the terms that enter
them.  Every case prints its measured maxima.
"""

import collections
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
import current_model as cm  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

Z = cm.GPU_Z
U = 2.0 ** -53
SHAPES = cm.GPU_CASES
SHARED = ("T", "ldos", "left", "right")
ROWS = ("current_left", "current_right")
BONDS = ("inter_left", "inter_right", "intra_left", "intra_right")
NEW = cm.NAMES
_CACHE = {}


def _model_arrays(results, bounds):
    """the model's outputs, bounds and scales of a [NK][NZ] list as arrays; a bound holds per component of its layer"""
    want = {name: cm.stack(results, name) for name in SHARED + NEW}
    want["its"] = cm.stack(results, "iterations").astype(np.int32)
    device = [[b.device for b in row] for row in bounds]
    bound = {name: cm.stack(device, name) for name in SHARED}
    bound.update({name: cm.stack(bounds, name) for name in NEW})
    scale = {name: cm.stack(bounds, "s_" + name) for name in NEW}
    return want, bound, scale


def _inputs(n, L, M):
    """current_model.gpu_case and the model's results, shared by the cases and never written."""
    key = (n, L, M)
    if key not in _CACHE:
        H00, H01, V = cm.gpu_case(n, L, M)
        results, bounds = cm.device_current_function(H00, H01, V, Z)
        want, bound, scale = _model_arrays(results, bounds)
        for array in [H00, H01, V] + list(want.values()) + list(bound.values()) + list(scale.values()):
            array.setflags(write=False)
        _CACHE[key] = (H00, H01, V, want, bound, scale, results, bounds)
    return _CACHE[key]


def _from_matrices(H00, H01, V, z, *, k_chunk=0, slots=0, bonds=True, max_iterations=64, check=True, drop=()):
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    V = np.ascontiguousarray(V, dtype=np.complex128)
    M = V.shape[0]
    out = {"T": np.full((n_k, len(z)), np.nan), "its": np.full((n_k, len(z)), -1, dtype=np.int32)}
    for name in ("ldos", "left", "right"):
        out[name] = np.full((n_k, len(z), M, N), np.nan)
    for name in ROWS:
        out[name] = np.full((n_k, len(z), M - 1, N), np.nan)
    for name in BONDS:
        out[name] = np.full((n_k, len(z), M - (name[:5] == "inter"), N, N), np.nan) if bonds else None
    for name in drop:
        out[name] = None
    status = _lib.lib().tbk_device_current_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), None if H01 is None else _lib.ptr(np.ascontiguousarray(H01)),
                                                         M, _lib.ptr(V), len(z), _lib.ptr(z), max_iterations, k_chunk, slots, _lib.ptr(out["its"]),
                                                         _lib.ptr(out["T"]), _lib.ptr(out["ldos"]), _lib.ptr(out["left"]), _lib.ptr(out["right"]),
                                                         *[_lib.ptr(out[name]) for name in NEW])
    if check:
        _lib.check(status)
        return out
    return status


def _green_from_matrices(H00, H01, V, z, *, green=False):
    """tbk_device_green_from_matrices on the same inputs: property 5's other side, and C_1 for T'"""
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    V = np.ascontiguousarray(V, dtype=np.complex128)
    M = V.shape[0]
    out = {"T": np.full((n_k, len(z)), np.nan), "its": np.full((n_k, len(z)), -1, dtype=np.int32)}
    for name in ("ldos", "left", "right"):
        out[name] = np.full((n_k, len(z), M, N), np.nan)
    for name in ("G", "F", "C"):
        out[name] = np.full((n_k, len(z), M, N, N), np.nan, dtype=np.complex128) if green else None
    _lib.check(_lib.lib().tbk_device_green_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), _lib.ptr(np.ascontiguousarray(H01)), M, _lib.ptr(V),
                                                         len(z), _lib.ptr(z), 64, 0, 0, _lib.ptr(out["its"]), _lib.ptr(out["T"]), _lib.ptr(out["ldos"]),
                                                         _lib.ptr(out["left"]), _lib.ptr(out["right"]), _lib.ptr(out["G"]), _lib.ptr(out["F"]),
                                                         _lib.ptr(out["C"])))
    return out


def _same(a, b, names=("its",) + SHARED + NEW):
    return all(np.array_equal(a[name], b[name]) for name in names if a[name] is not None and b[name] is not None)


def _errors(got, want, name):
    """the largest error per (k, z, layer) of a matrix or a row, per (k, z) for T"""
    err = np.abs(got[name] - want[name])
    if name == "T":
        return err
    return err.reshape(err.shape[:3] + (-1,)).max(axis=3) if err.size else np.zeros(err.shape[:3])  # (M = 1: no interface)


def _largest(array):
    return float(array.max()) if array.size else 0.0


# ---- 1. the kernel against the model on the same principal layers ---------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", SHAPES)
def test_kernel_matches_the_model(n, L, M):
    H00, H01, V, want, bound, _, _, _ = _inputs(n, L, M)
    ceiling = max(_largest(bound[name]) for name in bound)
    print("(n, L, M) = (%d, %d, %d): largest bound %.2e, iterations %d ... %d" % (n, L, M, ceiling, want["its"].min(), want["its"].max()))
    assert ceiling <= 1e-4
    first = None
    for chunk, slots in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2)):
        got = _from_matrices(H00, H01, V, Z, k_chunk=chunk, slots=slots)
        assert all(np.all(np.isfinite(got[name])) for name in SHARED + NEW)
        assert np.array_equal(got["its"], want["its"]), (n, L, M, chunk, slots)
        if first is None:
            for name in SHARED + NEW:
                assert got[name].shape == want[name].shape, name
                err = _errors(got, want, name)
                print("    %-13s max|kernel - model| = %.2e (largest 2 x bound %.2e)" % (name, _largest(err), 2 * _largest(bound[name])))
                assert np.all(err <= 2 * bound[name]), (n, L, M, name, _largest(err))
            first = got
            assert _same(_from_matrices(H00, H01, V, Z), first), "two calls differ"
        else:
            assert _same(got, first), "k_chunk = %d, slots = %d changed bits" % (chunk, slots)
    plain = _from_matrices(H00, H01, V, Z, bonds=False)
    assert plain["inter_left"] is None and _same(plain, first), "without the bond arrays the rows have other bits"
    # property 5: what device_green_function returns has its bits
    green = _green_from_matrices(H00, H01, V, Z)
    assert all(np.array_equal(green[name], first[name]) for name in ("its",) + SHARED), "the shared outputs differ from tbk_device_green's"


@pytest.mark.parametrize("n, L, M", SHAPES)
def test_identities_hold_on_the_outputs(n, L, M):
    """Properties 1 - 4 on the kernel's outputs; T' from C_1 of tbk_device_green_from_matrices and the model's es, et."""
    H00, H01, V, _, bound, _, results, bounds = _inputs(n, L, M)
    N = n * L
    got = _from_matrices(H00, H01, V, Z)
    last = _green_from_matrices(H00, H01, V, Z, green=True)["C"]
    worst = {}
    Out = collections.namedtuple("Out", ("T", "left", "right") + BONDS)
    for k in range(H00.shape[0]):
        for i, z in enumerate(Z):
            model = results[k][i].green
            out = Out(got["T"][k, i], got["left"][k, i], got["right"][k, i], *[got[name][k, i] for name in BONDS])
            residual = cm.identities(H00[k], H01[k], V, complex(z), out, cm.t_prime(last[k, i, 0], model.es, model.et))
            limit = cm.identity_bounds(complex(z), bounds[k][i], N)
            for name, value in residual.items():
                assert value.shape == limit[name].shape, name
                if value.size:
                    worst[name] = max(worst.get(name, 0.0), float(np.abs(value).max()))
                    assert np.all(np.abs(value) <= limit[name]), (name, k, i, np.abs(value).max(), limit[name].min())
            # property 4: zero where there is no hopping, J antisymmetric
            for side in ("left", "right"):
                K, J = got["inter_" + side][k, i], got["intra_" + side][k, i]
                assert np.all(K[:, H01[k] == 0] == 0.0)
                for p in range(M):
                    assert np.all(J[p][(H00[k] + V[p]) == 0] == 0.0)
                skew = np.abs(J + np.transpose(J, (0, 2, 1))).reshape(M, -1).max(axis=1)
                worst["skew"] = max(worst.get("skew", 0.0), float(skew.max()))
                assert np.all(skew <= 2 * bound["intra_" + side][k, i])
            if M > 1:  # the signs: the left lead's states flow to the right, the right lead's to the left
                assert np.all(got["current_left"][k, i].sum(axis=1) > 0.0) and np.all(got["current_right"][k, i].sum(axis=1) < 0.0)
    print("(n, L, M) = (%d, %d, %d): largest residuals %s" % (n, L, M, ", ".join("%s %.2e" % item for item in sorted(worst.items()))))


def test_no_hopping_no_current():
    """Property 4 on a device whose H01 and H00 + V have zeros: the bond currents there are exact zeros."""
    rng = np.random.default_rng(404)
    N, M = 20, 3
    H00 = np.zeros((2, N, N), dtype=np.complex128)
    H01 = np.zeros_like(H00)
    for k in range(2):
        a = (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) * (rng.random((N, N)) < 0.3)
        H00[k] = (a + a.conj().T) * 0.1
        H01[k] = (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) * (rng.random((N, N)) < 0.3) * 0.2
    V = np.zeros((M, N, N), dtype=np.complex128)
    V[:, np.arange(N), np.arange(N)] = rng.normal(size=(M, N)) * 0.3
    got = _from_matrices(H00, H01, V, Z)
    for k in range(2):
        assert np.count_nonzero(H01[k] == 0) > N and np.count_nonzero(H00[k] == 0) > N
        for side in ("left", "right"):
            assert np.all(got["inter_" + side][k][:, :, H01[k] == 0] == 0.0) and np.any(got["inter_" + side][k] != 0.0)
            for p in range(M):
                assert np.all(got["intra_" + side][k][:, p][:, (H00[k] + V[p]) == 0] == 0.0)
    want = cm.device_current(H00[1], H01[1], V, complex(Z[0]))
    tol = cm.tolerance(H00[1], H01[1], V, complex(Z[0]), want)
    for name in NEW:
        assert np.all(_errors({name: got[name][1:2, 0:1]}, {name: getattr(want, name)[None, None]}, name)[0, 0] <= 2 * getattr(tol, name)), name


@pytest.mark.parametrize("n, L, M", [s for s in SHAPES if s[0] * s[1] <= 17])
def test_kernel_against_mpmath(n, L, M):
    H00, H01, V, model, _, scale, _, _ = _inputs(n, L, M)
    got = _from_matrices(H00, H01, V, Z)
    with np.load(os.path.join(ROOT, "tests", "golden", "current_mp.npz")) as stored:
        assert np.array_equal(stored["Z"], Z)
        for name in NEW:
            ref = stored["%s_%d_%d_%d" % (name, n, L, M)]
            assert ref.shape == model[name].shape
            if not ref.size:
                continue
            size = scale[name].reshape(scale[name].shape + (1,) * (ref.ndim - 3))
            own = (np.abs(model[name] - ref) / size).max()
            mine = (np.abs(got[name] - ref) / size).max()
            print("(n, L, M) = (%d, %d, %d) %-13s: largest |gpu - mp| / scale = %.2e, |model - mp| / scale = %.2e (u = %.2e)" % (n, L, M, name, mine, own, U))
            assert mine <= 16 * max(U, own), name


@pytest.mark.parametrize("n, L, M", [(3, 1, 2), (17, 1, 2), (8, 8, 3), (5, 1, 6)])
def test_bits_of_an_energy_do_not_depend_on_the_list(n, L, M):
    H00, H01, V, want, _, _, _, _ = _inputs(n, L, M)
    base = _from_matrices(H00, H01, V, Z)
    order = [3, 0, 4, 2, 1]
    moved = _from_matrices(H00, H01, V, Z[order])
    assert all(np.array_equal(moved[name], base[name][:, order]) for name in ("its",) + SHARED + NEW), "a reordered list changed bits"
    assert np.array_equal(moved["its"], want["its"][:, order])
    alone = _from_matrices(H00, H01, V, Z[4:5], bonds=False)
    assert all(np.array_equal(alone[name][:, 0], base[name][:, 4]) for name in SHARED + ROWS), "an energy alone has other bits"
    rows = [2, 0]  # the k list reordered and shortened
    fewer = _from_matrices(H00[rows], H01[rows], V, Z, k_chunk=1)
    assert all(np.array_equal(fewer[name], base[name][rows]) for name in SHARED + NEW), "a point's bits depend on its neighbours"


# ---- 2. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_interface():
    H00, H01, V = _inputs(3, 1, 2)[:3]
    assert _from_matrices(H00, None, V, Z, check=False) == _lib.TBK_ERR_ARGUMENT and "H01" in _lib.last_error()
    assert _from_matrices(H00, H01, V, [0.3, 0.1j], check=False) == _lib.TBK_ERR_ARGUMENT and "Im z" in _lib.last_error()
    assert _from_matrices(H00, H01, V, Z, max_iterations=0, check=False) == _lib.TBK_ERR_ARGUMENT
    assert _from_matrices(H00, H01, V, Z, slots=-1, check=False) == _lib.TBK_ERR_ARGUMENT and "slots" in _lib.last_error()
    assert _from_matrices(H00, H01, np.zeros((4097, 3, 3)), Z[:1], check=False) == _lib.TBK_ERR_ARGUMENT and "1 to 4096" in _lib.last_error()
    for drop in (("inter_left",), ("inter_right", "intra_left"), ("intra_right",), ("inter_left", "inter_right", "intra_left")):
        assert _from_matrices(H00, H01, V, Z, check=False, drop=drop) == _lib.TBK_ERR_ARGUMENT and "all be NULL or none" in _lib.last_error(), drop
    for drop in (("current_left",), ("current_right",)):
        assert _from_matrices(H00, H01, V, Z, check=False, drop=drop) == _lib.TBK_ERR_ARGUMENT and "current_left / current_right" in _lib.last_error()
    big = np.zeros((1, 65, 65), dtype=np.complex128)
    assert _from_matrices(big, big, big, Z, check=False) == _lib.TBK_ERR_ARGUMENT and "at most 64" in _lib.last_error()


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------
def _scaled(r_vec, hop):
    """the hoppings scaled so that the norms of the full set add up to 2: the spectrum lies in [-2, 2]"""
    total = sum(np.linalg.norm(m, 2) for m in sm.full_hoppings(r_vec, hop).values())
    return hop * (2.0 / total)


def _synthetic(n, dim, n_r):
    r_vec, hop, pos = syn.dense_model_arrays(n, n_r, syn.MODEL_SEED + 2100 + 10 * n + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, _scaled(r_vec, hop), pos=pos), r_vec


def _layers(model, kpar, axis, L):
    kpar = np.asarray(kpar, dtype=float).reshape(len(kpar), -1)
    pts = np.concatenate([sm.sample_points(kp, axis, L, model.dim) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    pairs = [sm.principal(sm.layers_from_samples(h)) for h in ham]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _as_dict(result):
    out = {"T": result.transmission, "its": result.iterations, "ldos": result.ldos, "left": result.left, "right": result.right,
           "current_left": result.current_left, "current_right": result.current_right}
    bonds = len(result) == 15
    out.update({name: getattr(result, name) if bonds else None for name in BONDS})
    return out


@pytest.mark.parametrize("n, dim, n_r, axis, L, M", [(5, 3, 30, 0, 2, 3), (24, 2, 5, 1, 1, 2)])
def test_whole_call_matches_the_model_on_hamilton(n, dim, n_r, axis, L, M):
    model, r_vec = _synthetic(n, dim, n_r)
    assert max(abs(int(R[axis])) for R in r_vec) == L
    kpar = np.random.default_rng(31 + n).random((3, dim - 1)) - 0.5
    V = tm.random_device(n * L, M, 77 + n)
    H00, H01 = _layers(model, kpar, axis, L)
    want, bound, _ = _model_arrays(*cm.device_current_function(H00, H01, V, Z))
    assert max(_largest(b) for b in bound.values()) <= 1e-4
    result = model.device_current(kpar, Z, axis=axis, device=V, bonds=True)
    assert len(result) == 15 and result.layers == L and result.length == M and np.array_equal(result.z, Z) and np.array_equal(result.k, kpar)
    N = n * L
    assert result.current_left.shape == (3, 5, M - 1, N) and result.current_left.dtype == np.float64
    assert result.inter_right.shape == (3, 5, M - 1, N, N) and result.intra_left.shape == (3, 5, M, N, N) and result.intra_right.dtype == np.float64
    got = _as_dict(result)
    assert np.array_equal(got["its"], want["its"])
    for name in SHARED + NEW:
        err = _errors(got, want, name)
        print("dense %d orbitals dim %d axis %d L = %d M = %d %-13s: max|gpu - model| = %.2e (bound %.2e)" % (n, dim, axis, L, M, name, err.max(),
                                                                                                         2 * bound[name].max()))
        assert np.all(err <= 2 * bound[name]), name
    plain = model.device_current(kpar, Z, axis=axis - dim, device=V)
    assert len(plain) == 11 and _same(_as_dict(plain), got)
    one = model.device_current(kpar[2], Z[1], axis=axis, device=V)
    assert one.current_left.shape == (1, 1, M - 1, N) and np.array_equal(one.current_left[0, 0], result.current_left[2, 1])
    green = model.device_green_function(kpar, Z, axis=axis, device=V)
    assert all(np.array_equal(getattr(green, name), getattr(result, name)) for name in ("iterations", "transmission", "ldos", "left", "right"))
    single = model.device_current(kpar, Z, axis=axis, length=1, bonds=True)
    assert single.current_left.shape == (3, 5, 0, N) and single.inter_left.shape == (3, 5, 0, N, N) and np.all(np.isfinite(single.intra_left))


def test_csr_twin_two_handles_and_chunks():
    n, dim, axis, L, M = 6, 3, 2, 1, 3
    model, _ = _synthetic(n, dim, 8)
    kpar = np.random.default_rng(5).random((7, dim - 1))
    V = tm.random_device(n, M, 3)
    H00, H01 = _layers(model, kpar, axis, L)
    _, bound, _ = _model_arrays(*cm.device_current_function(H00, H01, V, Z))
    one = _as_dict(model.device_current(kpar, Z, device=V, bonds=True))
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    other = _as_dict(sparse.device_current(kpar, Z, device=V, bonds=True))
    assert np.array_equal(other["its"], one["its"])
    for name in SHARED + NEW:
        assert np.all(_errors(other, one, name) <= 2 * bound[name]), "CSR against dense: " + name
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = _as_dict(twin.device_current(kpar, Z, device=V, bonds=True))
    assert len(twin._handles) == 2  # pylint: disable=protected-access
    chunked = pickle.loads(pickle.dumps(model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 3)
    three = _as_dict(chunked.device_current(kpar, Z, device=V, bonds=True))
    for name, other in (("two handles", two), ("chunks of 3 points", three)):  # the bits of a (k, z) depend on nothing else
        assert _same(other, one), name + ": other bits than one call"
    wide = tbmodels_amd.Model(hop={(0, 3): np.eye(24) * 0.1, (1, 0): np.eye(24) * 0.1}, size=24, dim=2, pos=np.zeros((24, 2)), contains_cc=False)
    with pytest.raises(ValueError, match="72 rows: device_current takes at most 64"):
        wide.device_current([[0.1]], Z)
    with pytest.raises(np.linalg.LinAlgError):
        model.device_current(kpar, Z, device=V, max_iterations=2)
    assert _same(_as_dict(model.device_current(kpar, Z, device=V, bonds=True)), one), "the handle after the cap"


def test_device_current_calls_are_timed_on_their_own_row():
    model, _ = _synthetic(24, 2, 5)
    kpar = np.linspace(0.0, 0.5, 6)[:, None]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.device_current(kpar, Z, length=3)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_device_current_timing(model._staged(), ms, ctypes.byref(calls), 1))  # pylint: disable=protected-access
    print("24 orbitals, 6 points, 5 energies, 3 layers: H(k) and layers %.3f ms, decimation and sweeps %.3f ms, output %.3f ms" % (ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_device_green_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0
