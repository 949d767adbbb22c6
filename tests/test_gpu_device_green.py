"""
The layer-resolved Green's functions of the device: device_green_kernel of csrc/tbk_device_green.hip against tools/device_model.py on
identical principal layers (`tbk_device_green_from_matrices`), and `Model.device_green_function` against the model on `Model.hamilton`.

Bounds (u = 2^-53), none measured on the code under test: device_model.tolerance, per component of a block B of layer p

    E c(B) s(B),    E = 8 N u rho (|z| + |H00|_2 + 2 |H01|_2 + max |V_p|_2) / eta (iterations + M + 1)

with rho and iterations of the model's run, c the number of error-carrying factors behind B and s the product of the 2-norms of the
blocks B is formed from; kernel against model is held to twice it, and it stays at or below 1e-4 in every case, which is asserted.  The
sharper check: for N <= 17 the largest error of ldos, left, right and T against the stored mpmath values (tests/golden/device_mp.npz,
`tools/device_model.py --golden`), in units of the case's scale, is at most 16 max(u, the model's own).  Every case prints its measured
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
import device_model as dm  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

Z = dm.GPU_Z
U = 2.0 ** -53
SHAPES = dm.GPU_CASES
FIELDS = ("ldos", "left", "right", "G", "F", "C")
_CACHE = {}


def _model_arrays(results, bounds):
    """the model's outputs and bounds of a [NK][NZ] list as arrays; the bounds of the blocks broadcast over the components"""
    want = {name: dm.stack(results, name) for name in ("T",) + FIELDS}
    want["its"] = dm.stack(results, "iterations").astype(np.int32)
    bound = {name: dm.stack(bounds, name) for name in ("T",) + FIELDS}
    scale = {}
    for name, field in (("ldos", "sG"), ("left", "sL"), ("right", "sR")):
        scale[name] = dm.stack(bounds, field)
    return want, bound, scale


def _inputs(n, L, M):
    """device_model.gpu_case and the model's results, shared by the cases and never written."""
    key = (n, L, M)
    if key not in _CACHE:
        H00, H01, V = dm.gpu_case(n, L, M)
        results, bounds = dm.device_green_function(H00, H01, V, Z)
        want, bound, scale = _model_arrays(results, bounds)
        scale["T"] = np.array([[tm.scale(H00[k], H01[k], complex(z), results[k][i].Q[M - 1]) for i, z in enumerate(Z)] for k in range(dm.GPU_NK)])
        for array in [H00, H01, V] + list(want.values()) + list(bound.values()) + list(scale.values()):
            array.setflags(write=False)
        _CACHE[key] = (H00, H01, V, want, bound, scale)
    return _CACHE[key]


def _from_matrices(H00, H01, V, z, *, k_chunk=0, slots=0, green=False, max_iterations=64, check=True):
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    V = np.ascontiguousarray(V, dtype=np.complex128)
    M = V.shape[0]
    out = {"T": np.full((n_k, len(z)), np.nan), "its": np.full((n_k, len(z)), -1, dtype=np.int32)}
    for name in ("ldos", "left", "right"):
        out[name] = np.full((n_k, len(z), M, N), np.nan)
    for name in ("G", "F", "C"):
        out[name] = np.full((n_k, len(z), M, N, N), np.nan, dtype=np.complex128) if green else None
    status = _lib.lib().tbk_device_green_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), None if H01 is None else _lib.ptr(np.ascontiguousarray(H01)),
                                                       M, _lib.ptr(V), len(z), _lib.ptr(z), max_iterations, k_chunk, slots, _lib.ptr(out["its"]),
                                                       _lib.ptr(out["T"]), _lib.ptr(out["ldos"]), _lib.ptr(out["left"]), _lib.ptr(out["right"]),
                                                       _lib.ptr(out["G"]), _lib.ptr(out["F"]), _lib.ptr(out["C"]))
    if check:
        _lib.check(status)
        return out
    return status


def _same(a, b, names=("T", "its") + FIELDS):
    return all(np.array_equal(a[name], b[name]) for name in names if a[name] is not None and b[name] is not None)


def _errors(got, want, name):
    """the largest error per (k, z, layer) of a block or a row, per (k, z) for T"""
    err = np.abs(got[name] - want[name])
    return err if name == "T" else err.reshape(err.shape[:3] + (-1,)).max(axis=3)


# ---- 1. the kernel against the model on the same principal layers ---------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", SHAPES)
def test_kernel_matches_the_model(n, L, M):
    H00, H01, V, want, bound, _ = _inputs(n, L, M)
    ceiling = max(bound[name].max() for name in bound)
    print("(n, L, M) = (%d, %d, %d): largest bound %.2e, iterations %d ... %d" % (n, L, M, ceiling, want["its"].min(), want["its"].max()))
    assert ceiling <= 1e-4
    first = None
    for chunk, slots in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2)):
        got = _from_matrices(H00, H01, V, Z, k_chunk=chunk, slots=slots, green=True)
        assert all(np.all(np.isfinite(got[name].view(float))) for name in ("T",) + FIELDS)
        assert np.array_equal(got["its"], want["its"]), (n, L, M, chunk, slots)
        if first is None:
            for name in ("T",) + FIELDS:
                err = _errors(got, want, name)
                print("    %-5s max|kernel - model| = %.2e (bounds %.2e ... %.2e)" % (name, err.max(), 2 * bound[name].min(), 2 * bound[name].max()))
                assert np.all(err <= 2 * bound[name]), (n, L, M, name, err.max())
            first = got
            assert _same(_from_matrices(H00, H01, V, Z, green=True), first), "two calls differ"
        else:
            assert _same(got, first), "k_chunk = %d, slots = %d changed bits" % (chunk, slots)
    plain = _from_matrices(H00, H01, V, Z)
    assert plain["G"] is None and _same(plain, first), "without the blocks the rows have other bits"
    # property 3: F_M and T are the transmission's
    T = np.full(first["T"].shape, np.nan)
    P = np.full(first["T"].shape + (n * L, n * L), np.nan, dtype=np.complex128)
    its = np.zeros(T.shape, dtype=np.int32)
    zz, VV = np.ascontiguousarray(Z), np.ascontiguousarray(V)
    _lib.check(_lib.lib().tbk_transmission_from_matrices(0, n * L, H00.shape[0], _lib.ptr(np.ascontiguousarray(H00)), _lib.ptr(np.ascontiguousarray(H01)), M,
                                                         _lib.ptr(VV), len(zz), _lib.ptr(zz), 64, 0, _lib.ptr(its), _lib.ptr(T), _lib.ptr(P)))
    assert np.array_equal(T, first["T"]) and np.array_equal(P, first["F"][:, :, M - 1]) and np.array_equal(its, first["its"])


@pytest.mark.parametrize("n, L, M", [s for s in SHAPES if s[0] * s[1] <= 17])
def test_kernel_against_mpmath(n, L, M):
    H00, H01, V, model, _, scale = _inputs(n, L, M)
    got = _from_matrices(H00, H01, V, Z)
    with np.load(os.path.join(ROOT, "tests", "golden", "device_mp.npz")) as stored:
        assert np.array_equal(stored["Z"], Z)
        for name in ("T", "ldos", "left", "right"):
            ref = stored["%s_%d_%d_%d" % (name, n, L, M)]
            assert ref.shape == model[name].shape
            size = scale[name] if name == "T" else scale[name][..., None]
            own = (np.abs(model[name] - ref) / size).max()
            mine = (np.abs(got[name] - ref) / size).max()
            print("(n, L, M) = (%d, %d, %d) %-5s: largest |gpu - mp| / scale = %.2e, |model - mp| / scale = %.2e (u = %.2e)" % (n, L, M, name, mine, own, U))
            assert mine <= 16 * max(U, own), name


@pytest.mark.parametrize("n, L, M", [(3, 1, 2), (17, 1, 2), (16, 4, 3), (5, 1, 6)])
def test_bits_of_an_energy_do_not_depend_on_the_list(n, L, M):
    H00, H01, V, want, _, _ = _inputs(n, L, M)
    base = _from_matrices(H00, H01, V, Z, green=True)
    order = [3, 0, 4, 2, 1]
    moved = _from_matrices(H00, H01, V, Z[order], green=True)
    assert all(np.array_equal(moved[name], base[name][:, order]) for name in ("T", "its") + FIELDS), "a reordered list changed bits"
    assert np.array_equal(moved["its"], want["its"][:, order])
    for index in (0, 4):
        alone = _from_matrices(H00, H01, V, Z[index:index + 1], green=True)
        assert all(np.array_equal(alone[name][:, 0], base[name][:, index]) for name in ("T",) + FIELDS), "an energy alone has other bits"
    rows = [2, 0]  # the k list reordered and shortened
    fewer = _from_matrices(H00[rows], H01[rows], V, Z, k_chunk=1, green=True)
    assert all(np.array_equal(fewer[name], base[name][rows]) for name in ("T",) + FIELDS), "a point's bits depend on its neighbours"


# ---- 2. the cap and a singular matrix are statuses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", [(3, 1, 2), (8, 4, 2), (16, 4, 3)])
def test_the_cap_names_the_first_point_that_reached_it(n, L, M):
    H00, H01, V, want, _, _ = _inputs(n, L, M)
    order = [1, 2, 4, 0, 3]  # the slowest energies are not the first of the list
    z, its = Z[order], want["its"][:, order]
    cap = int(its.max()) - 1
    k, zi = [int(x[0]) for x in np.nonzero(its > cap)]  # the first in (k, z) order
    assert (k, zi) != (0, 0)
    for chunk in (0, 1):
        status = _from_matrices(H00, H01, V, z, max_iterations=cap, k_chunk=chunk, check=False)
        message = _lib.last_error()
        print("cap %d:" % cap, message)
        assert status == _lib.TBK_ERR_NO_CONVERGENCE
        assert "k index %d and energy %d " % (k, zi) in message and "%d iterations" % cap in message
    with pytest.raises(np.linalg.LinAlgError):
        _lib.check(status)
    _from_matrices(H00, H01, V, z, max_iterations=cap + 1)  # the cap itself is enough


@pytest.mark.parametrize("size", [2, 20, 40])
def test_a_singular_first_layer_is_named_exactly(size):
    """tests/test_gpu_transport.py's construction: the last orbital does not couple to the neighbouring layers, and V_1 puts z[1] on its
    diagonal element at k index 2 alone: column size - 1 of z - D_1 is zero."""
    z = np.array([0.1 + 0.2j, 0.3 + 0.2j, -0.4 - 0.1j])
    H00 = np.zeros((4, size, size), dtype=np.complex128)
    H00[:] = np.diag(np.linspace(-1.0, 1.0, size))
    H00[:, size - 1, size - 1] = 1.0
    H00[2, size - 1, size - 1] = 0.5
    H01 = np.zeros_like(H00)
    H01[:, 0, 0] = 0.7
    V = np.zeros((2, size, size), dtype=np.complex128)
    V[0, size - 1, size - 1] = z[1] - 0.5
    assert 0.5 + V[0, size - 1, size - 1] == z[1]
    for chunk in (0, 1):
        status = _from_matrices(H00, H01, V, z, k_chunk=chunk, check=False)
        print("singular first layer:", _lib.last_error())
        assert status == _lib.TBK_ERR_SINGULAR
        assert "Singular matrix" in _lib.last_error() and "k index 2 and energy 1 " in _lib.last_error()
    H00[2, size - 1, size - 1] = 1.0
    got = _from_matrices(H00, H01, V, z)
    assert np.all(np.isfinite(got["ldos"]))


def test_argument_errors_of_the_c_interface():
    H00, H01, V = _inputs(3, 1, 2)[:3]
    assert _from_matrices(H00, None, V, Z, check=False) == _lib.TBK_ERR_ARGUMENT and "H01" in _lib.last_error()
    assert _from_matrices(H00, H01, V, [0.3, 0.1j], check=False) == _lib.TBK_ERR_ARGUMENT and "Im z" in _lib.last_error()
    assert _from_matrices(H00, H01, V, Z, max_iterations=0, check=False) == _lib.TBK_ERR_ARGUMENT
    assert _from_matrices(H00, H01, V, Z, slots=-1, check=False) == _lib.TBK_ERR_ARGUMENT and "slots" in _lib.last_error()
    T, its, rows = np.zeros((3, 5)), np.zeros((3, 5), dtype=np.int32), np.zeros((3, 5, 2, 3))
    blocks = np.zeros((3, 5, 2, 3, 3), dtype=np.complex128)

    def call(N, n_k, h, M, v, G=None, F=None, C=None):
        return _lib.lib().tbk_device_green_from_matrices(0, N, n_k, _lib.ptr(h), _lib.ptr(h), M, _lib.ptr(v), 5, _lib.ptr(Z), 64, 0, 0, _lib.ptr(its),
                                                         _lib.ptr(T), _lib.ptr(rows), _lib.ptr(rows), _lib.ptr(rows), _lib.ptr(G), _lib.ptr(F), _lib.ptr(C))

    for M in (0, 4097):
        assert call(3, 3, np.ascontiguousarray(H00), M, V) == _lib.TBK_ERR_ARGUMENT and "1 to 4096" in _lib.last_error()
    assert call(3, 3, np.ascontiguousarray(H00), 2, V, G=blocks) == _lib.TBK_ERR_ARGUMENT and "all be NULL or none" in _lib.last_error()
    assert call(3, 3, np.ascontiguousarray(H00), 2, V, F=blocks, C=blocks) == _lib.TBK_ERR_ARGUMENT
    big = np.zeros((1, 65, 65), dtype=np.complex128)
    assert call(65, 1, big, 1, big) == _lib.TBK_ERR_ARGUMENT and "at most 64" in _lib.last_error()
    # (V above 256 MiB and a stack above 1 GiB cannot be reached below 65 rows and 4097 layers: 4096 layers of 64 rows are 256 MiB)


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


def _reference(model, kpar, axis, L, V):
    """The model's run on principal layers taken from `Model.hamilton` at the 2 L + 1 samples of every in-plane point."""
    H00, H01 = _layers(model, kpar, axis, L)
    want, bound, _ = _model_arrays(*dm.device_green_function(H00, H01, V, Z))
    return want, bound, (H00, H01)


def _as_dict(result):
    out = {"T": result.transmission, "its": result.iterations, "ldos": result.ldos, "left": result.left, "right": result.right}
    green = len(result) == 12
    out.update({"G": result.diagonal if green else None, "F": result.first if green else None, "C": result.last if green else None})
    return out


@pytest.mark.parametrize("n, dim, n_r, axis, L, M", [(6, 3, 8, 2, 1, 3), (5, 3, 30, 0, 2, 2), (24, 2, 5, 1, 1, 2)])
def test_whole_call_matches_the_model_on_hamilton(n, dim, n_r, axis, L, M):
    model, r_vec = _synthetic(n, dim, n_r)
    assert max(abs(int(R[axis])) for R in r_vec) == L
    kpar = np.random.default_rng(31 + n).random((3, dim - 1)) - 0.5
    V = tm.random_device(n * L, M, 77 + n)
    want, bound, _ = _reference(model, kpar, axis, L, V)
    assert max(b.max() for b in bound.values()) <= 1e-4
    result = model.device_green_function(kpar, Z, axis=axis, device=V, green=True)
    assert result.layers == L and result.length == M and np.array_equal(result.z, Z) and np.array_equal(result.k, kpar)
    assert result.ldos.shape == (3, 5, M, n * L) and result.ldos.dtype == np.float64 and result.diagonal.shape == (3, 5, M, n * L, n * L)
    assert result.first.dtype == np.complex128 and result.iterations.dtype == np.int32
    got = _as_dict(result)
    assert np.array_equal(got["its"], want["its"])
    for name in ("T",) + FIELDS:
        err = _errors(got, want, name)
        print("dense %d orbitals dim %d axis %d L = %d M = %d %-5s: max|gpu - model| = %.2e (bound %.2e)" % (n, dim, axis, L, M, name, err.max(),
                                                                                                        2 * bound[name].max()))
        assert np.all(err <= 2 * bound[name]), name
    plain = model.device_green_function(kpar, Z, axis=axis - dim, device=V)
    assert len(plain) == 9 and _same(_as_dict(plain), got)
    one = model.device_green_function(kpar[2], Z[1], axis=axis, device=V)
    assert one.ldos.shape == (1, 1, M, n * L) and np.array_equal(one.ldos[0, 0], result.ldos[2, 1])
    trans = model.transmission(kpar, Z, axis=axis, device=V, green=True)
    assert np.array_equal(trans.transmission, result.transmission) and np.array_equal(trans.green, result.first[:, :, M - 1])
    # M pristine layers: zeros against length
    zeros = model.device_green_function(kpar, Z, axis=axis, device=np.zeros((M, n * L, n * L)))
    length = model.device_green_function(kpar, Z, axis=axis, length=M)
    assert length.length == M and _same(_as_dict(zeros), _as_dict(length))


def test_csr_twin_two_handles_chunks_and_the_onsite_form():
    n, dim, axis, L, M = 6, 3, 2, 1, 3
    model, _ = _synthetic(n, dim, 8)
    kpar = np.random.default_rng(5).random((7, dim - 1))
    onsite = np.random.default_rng(6).normal(size=(M, n)) * 0.3
    V = np.zeros((M, n, n), dtype=np.complex128)
    V[:, np.arange(n), np.arange(n)] = onsite
    _, bound, _ = _reference(model, kpar, axis, L, V)
    one = _as_dict(model.device_green_function(kpar, Z, device=V, green=True))
    short = _as_dict(model.device_green_function(kpar, Z, device=onsite, green=True))
    assert _same(short, one), "the (M, N) form has other bits"
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    other = _as_dict(sparse.device_green_function(kpar, Z, device=V, green=True))
    assert np.array_equal(other["its"], one["its"])
    for name in ("T",) + FIELDS:
        assert np.all(_errors(other, one, name) <= 2 * bound[name]), "CSR against dense: " + name
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = _as_dict(twin.device_green_function(kpar, Z, device=V, green=True))
    assert len(twin._handles) == 2  # pylint: disable=protected-access
    chunked = pickle.loads(pickle.dumps(model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 3)
    three = _as_dict(chunked.device_green_function(kpar, Z, device=V, green=True))
    for name, other in (("two handles", two), ("chunks of 3 points", three)):  # the bits of a (k, z) depend on nothing else
        assert _same(other, one), name + ": other bits than one call"
    forced = pickle.loads(pickle.dumps(model))
    forced.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)  # there is no library route: the own kernel
    assert _same(_as_dict(forced.device_green_function(kpar, Z, device=V, green=True)), one)


def test_a_pristine_device_is_the_bulk_and_the_rest_has_the_sign_of_eta():
    n, dim, axis, L, M = 6, 3, 2, 1, 4
    model, _ = _synthetic(n, dim, 8)
    kpar = np.random.default_rng(8).random((3, dim - 1))
    want, bound, (H00, H01) = _reference(model, kpar, axis, L, np.zeros((M, n, n)))
    got = model.device_green_function(kpar, Z, length=M, green=True)
    surface = model.surface_green_function(kpar, Z)
    its, rho = sm.surface_green_function(H00, H01, Z)[3:]
    limit = 2 * bound["G"] + 2 * sm.tolerance(H00, H01, Z, its, rho)[:, :, None]
    err = np.abs(got.diagonal - surface.bulk[:, :, None]).reshape(3, 5, M, -1).max(axis=3)
    print("V = 0: max|G_p - bulk| = %.2e (bounds %.2e ... %.2e)" % (err.max(), limit.min(), limit.max()))
    assert np.all(err <= limit)
    # property 1: ldos - left - right has the sign of Im z, within the bounds
    V = tm.random_device(n, M, 12)
    want, bound, _ = _reference(model, kpar, axis, L, V)
    got = model.device_green_function(kpar, Z, device=V)
    rest = (got.ldos - got.left - got.right) * np.sign(Z.imag)[None, :, None, None]
    slack = 2 * (bound["ldos"] + bound["left"] + bound["right"])[..., None]
    assert np.all(rest >= -slack) and np.all((want["ldos"] - want["left"] - want["right"]) * np.sign(Z.imag)[None, :, None, None] > 0.0)
    assert np.all(rest > 0.0)  # (the rest is eta |G|^2 / pi: far above the bounds at these energies)


def test_errors_and_the_handle_goes_on():
    model, _ = _synthetic(6, 3, 8)
    kpar = np.random.default_rng(9).random((3, 2))
    V = tm.random_device(6, 2, 3)
    with pytest.raises(np.linalg.LinAlgError) as raised:
        model.device_green_function(kpar, Z, device=V, max_iterations=2)
    print("the cap:", raised.value)
    assert "k index 0 and energy 0 " in str(raised.value) and "2 iterations" in str(raised.value)
    want, bound, _ = _reference(model, kpar, 2, 1, V)
    got = _as_dict(model.device_green_function(kpar, Z, device=V))  # the same model and handle
    for name in ("T", "ldos", "left", "right"):
        assert np.all(_errors(got, want, name) <= 2 * bound[name])
    skew = V.copy()
    skew[1, 0, 1] += 1e-9
    for bad in ({"axis": 3}, {"axis": 0.5}, {"max_iterations": 0}, {"max_iterations": 5000}, {"length": 0}, {"length": 1.5}, {"length": 5000},
                {"device": V[0]}, {"device": np.zeros((2, 5))}, {"device": np.zeros((0, 6, 6))}, {"device": skew}, {"device": 1j * np.ones((2, 6))}):
        with pytest.raises(ValueError):
            model.device_green_function(kpar, Z, **bad)
    with pytest.raises(ValueError):
        model.device_green_function(kpar, [0.3, 0.1j])  # a real energy
    wide = tbmodels_amd.Model(hop={(0, 3): np.eye(24) * 0.1, (1, 0): np.eye(24) * 0.1}, size=24, dim=2, pos=np.zeros((24, 2)), contains_cc=False)
    with pytest.raises(ValueError, match="72 rows: device_green_function takes at most 64"):
        wide.device_green_function([[0.1]], Z)
    flat = tbmodels_amd.Model(hop={(1, 0): np.array([[0.5]])}, size=1, dim=2, pos=np.zeros((1, 2)), contains_cc=False)
    with pytest.raises(ValueError, match="no hopping along axis 1"):
        flat.device_green_function([[0.1]], Z)


def test_device_green_calls_are_timed_on_their_own_row():
    model, _ = _synthetic(24, 2, 5)
    kpar = np.linspace(0.0, 0.5, 6)[:, None]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.device_green_function(kpar, Z, length=3)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_device_green_timing(model._staged(), ms, ctypes.byref(calls), 1))  # pylint: disable=protected-access
    print("24 orbitals, 6 points, 5 energies, 3 layers: H(k) and layers %.3f ms, decimation and sweeps %.3f ms, output %.3f ms" % (ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_transmission_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0
