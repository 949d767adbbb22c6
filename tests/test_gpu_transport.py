"""
The Landauer transmission: transmission_kernel of csrc/tbk_surface.hip (and the library route above 64 rows) against
tools/transport_model.py on identical principal layers (`tbk_transmission_from_matrices`), and `Model.transmission` against the model
on `Model.hamilton` and the chain's closed form.

Bounds (u = 2^-53), none measured on the code under test: transport_model.tolerance = 4 eps scale,

    eps   = 8 N u rho (|z| + |H00|_2 + 2 |H01|_2 + max |V_p|_2) / eta (iterations + M + 1)
    scale = N (2 |H01|_2^2 |G_bottom|_2) (2 |H01|_2^2 |G_top|_2) |P_M|_2^2

with rho and iterations of the model's run; kernel against model is held to twice it, and it stays at or below 1e-4 in every case, which
is asserted.  P_M is held componentwise to twice surface_model.tolerance with iterations + M + 1 inversions.  The sharper check: for
N <= 17 the largest |T_gpu - T_mp| / scale of a case is at most 16 max(u, largest |T_model - T_mp| / scale), T_mp from
transport_model.transmission_mp at 60 digits (stored in tests/golden/transport_mp.npz by `tools/transport_model.py --golden`, which
takes a minute: DESIGN.md 22.7 has both columns).  Every case prints its measured maximum.
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
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])  # tests/test_gpu_surface.py's
U = 2.0 ** -53
# (n, L, M): N = 1, 3, 16, 17, 32, 33, 64 (twice): every edge of the templates NP = 16, 32, 64; N = 65: the library route
SHAPES = tm.GPU_CASES
_CACHE = {}


def _inputs(n, L, M):
    """transport_model.gpu_case and the model's results, shared by the cases and never written."""
    key = (n, L, M)
    if key not in _CACHE:
        H00, H01, V = tm.gpu_case(n, L, M)
        T, P, its, rho = tm.transmission_function(H00, H01, V, Z)
        bound, size, gbound = np.empty(T.shape), np.empty(T.shape), np.empty(T.shape)
        for k in range(T.shape[0]):
            for i, z in enumerate(Z):
                size[k, i] = tm.scale(H00[k], H01[k], complex(z), P[k, i])
                bound[k, i] = 4.0 * tm.relative_error(H00[k], H01[k], V, complex(z), its[k, i], rho[k, i]) * size[k, i]
                gbound[k, i] = tm.green_tolerance(H00[k], H01[k], V, complex(z), its[k, i], rho[k, i])
        for array in (H00, H01, V, T, P, its, bound, size, gbound):
            array.setflags(write=False)
        _CACHE[key] = (H00, H01, V, T, P, its, bound, size, gbound)
    return _CACHE[key]


def _from_matrices(H00, H01, V, z, *, k_chunk=0, green=False, max_iterations=64, check=True):
    n_k, N = H00.shape[0], H00.shape[-1]
    z = np.ascontiguousarray(z, dtype=np.complex128)
    V = np.ascontiguousarray(V, dtype=np.complex128)
    T = np.full((n_k, len(z)), np.nan)
    G = np.full((n_k, len(z), N, N), np.nan, dtype=np.complex128) if green else None
    its = np.full((n_k, len(z)), -1, dtype=np.int32)
    status = _lib.lib().tbk_transmission_from_matrices(0, N, n_k, _lib.ptr(np.ascontiguousarray(H00)), None if H01 is None else _lib.ptr(np.ascontiguousarray(H01)),
                                                       V.shape[0], _lib.ptr(V), len(z), _lib.ptr(z), max_iterations, k_chunk, _lib.ptr(its), _lib.ptr(T),
                                                       _lib.ptr(G))
    if check:
        _lib.check(status)
        return T, its, G
    return status


# ---- 1. the kernel against the model on the same principal layers ---------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", SHAPES)
def test_kernel_matches_the_model(n, L, M):
    H00, H01, V, want, P, its, bound, _, gbound = _inputs(n, L, M)
    print("(n, L, M) = (%d, %d, %d): bounds %.2e ... %.2e, T up to %.3f, iterations %d ... %d" % (n, L, M, bound.min(), bound.max(), want.max(),
                                                                                               its.min(), its.max()))
    assert np.all(bound <= 1e-4), bound.max()
    first = None
    for chunk in (0, 1, 2):
        T, count, G = _from_matrices(H00, H01, V, Z, k_chunk=chunk, green=True)
        assert np.all(np.isfinite(T)) and np.all(np.isfinite(G.view(float)))
        err = np.abs(T - want)
        gerr = np.abs(G - P).reshape(T.shape + (-1,)).max(axis=2)
        print("    chunk %d: max|T - model| = %.2e, max|P_M - model| = %.2e (bounds %.2e ... %.2e)" % (chunk, err.max(), gerr.max(), 2 * gbound.min(),
                                                                                                     2 * gbound.max()))
        assert np.all(err <= 2 * bound), (n, L, M, chunk, err, bound)
        assert np.all(gerr <= 2 * gbound), (n, L, M, chunk, gerr, gbound)
        assert np.array_equal(count, its), (n, L, M, chunk, count, its)
        if first is None:
            first = (T, G)
            again = _from_matrices(H00, H01, V, Z, k_chunk=chunk, green=True)
            assert np.array_equal(again[0], T) and np.array_equal(again[2], G), "two calls differ"
        else:
            assert np.array_equal(T, first[0]) and np.array_equal(G, first[1]), "the chunk changed bits"
    plain, count, none = _from_matrices(H00, H01, V, Z)
    assert none is None and np.array_equal(count, its)
    assert np.array_equal(plain, first[0]), "green=False has other bits"


@pytest.mark.parametrize("n, L, M", [s for s in SHAPES if s[0] * s[1] <= 17])
def test_kernel_against_mpmath(n, L, M):
    H00, H01, V, model, _, _, _, size, _ = _inputs(n, L, M)
    with np.load(os.path.join(ROOT, "tests", "golden", "transport_mp.npz")) as stored:
        T_mp = stored["T_%d_%d_%d" % (n, L, M)]
        assert np.array_equal(stored["Z"], Z)
    assert T_mp.shape == model.shape
    T, _, _ = _from_matrices(H00, H01, V, Z)
    own = (np.abs(model - T_mp) / size).max()
    got = (np.abs(T - T_mp) / size).max()
    print("(n, L, M) = (%d, %d, %d): largest |T_gpu - T_mp| / scale = %.2e, |T_model - T_mp| / scale = %.2e (u = %.2e)" % (n, L, M, got, own, U))
    assert got <= 16 * max(U, own)


@pytest.mark.parametrize("n, L, M", [(3, 1, 2), (17, 1, 2), (16, 4, 3), (13, 5, 2)])
def test_bits_of_an_energy_do_not_depend_on_the_list(n, L, M):
    H00, H01, V, _, _, its, _, _, _ = _inputs(n, L, M)
    base, _, base_g = _from_matrices(H00, H01, V, Z, green=True)
    order = [3, 0, 4, 2, 1]
    moved, count, moved_g = _from_matrices(H00, H01, V, Z[order], green=True)
    assert np.array_equal(moved, base[:, order]) and np.array_equal(moved_g, base_g[:, order]), "a reordered list changed bits"
    assert np.array_equal(count, its[:, order])
    for index in (0, 4):
        alone, _, _ = _from_matrices(H00, H01, V, Z[index:index + 1])
        assert np.array_equal(alone[:, 0], base[:, index]), "an energy alone has other bits"
    rows = [2, 0]  # the k list reordered and shortened
    fewer, _, _ = _from_matrices(H00[rows], H01[rows], V, Z, k_chunk=1)
    assert np.array_equal(fewer, base[rows]), "a point's bits depend on its neighbours"


# ---- 2. the cap and a singular matrix are statuses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, L, M", [(3, 1, 2), (8, 4, 2), (16, 4, 3), (13, 5, 2)])
def test_the_cap_names_the_first_point_that_reached_it(n, L, M):
    H00, H01, V, _, _, its, _, _, _ = _inputs(n, L, M)
    order = [1, 2, 4, 0, 3]  # the slowest energies are not the first of the list
    z, its = Z[order], its[:, order]
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


@pytest.mark.parametrize("size", [2, 20, 40, 70])
def test_a_singular_first_layer_is_named_exactly(size):
    """The last orbital does not couple to the neighbouring layers, so et keeps H00 there exactly; V_1 (as given: the C interface does
    not ask for a Hermitian V) puts z[1] on that diagonal element at k index 2 alone: column size - 1 of z - D_1 is zero."""
    z = np.array([0.1 + 0.2j, 0.3 + 0.2j, -0.4 - 0.1j])
    H00 = np.zeros((4, size, size), dtype=np.complex128)
    H00[:] = np.diag(np.linspace(-1.0, 1.0, size))
    H00[:, size - 1, size - 1] = 1.0
    H00[2, size - 1, size - 1] = 0.5
    H01 = np.zeros_like(H00)
    H01[:, 0, 0] = 0.7
    V = np.zeros((2, size, size), dtype=np.complex128)
    V[0, size - 1, size - 1] = z[1] - 0.5  # (exact: 0.3 - 0.5 by Sterbenz, and 0.5 + (0.3 - 0.5) is 0.3 again)
    assert 0.5 + V[0, size - 1, size - 1] == z[1]
    for chunk in (0, 1):
        status = _from_matrices(H00, H01, V, z, k_chunk=chunk, check=False)
        print("singular first layer:", _lib.last_error())
        assert status == _lib.TBK_ERR_SINGULAR
        assert "Singular matrix" in _lib.last_error() and "k index 2 and energy 1 " in _lib.last_error()
    H00[2, size - 1, size - 1] = 1.0
    T, _, _ = _from_matrices(H00, H01, V, z)
    assert np.all(np.isfinite(T))


def test_argument_errors_of_the_c_interface():
    H00, H01, V = _inputs(3, 1, 2)[:3]
    assert _from_matrices(H00, None, V, Z, check=False) == _lib.TBK_ERR_ARGUMENT and "H01" in _lib.last_error()
    assert _from_matrices(H00, H01, V, [0.3, 0.1j], check=False) == _lib.TBK_ERR_ARGUMENT and "Im z" in _lib.last_error()
    assert _from_matrices(H00, H01, V, Z, max_iterations=0, check=False) == _lib.TBK_ERR_ARGUMENT
    T, its = np.zeros((3, 5)), np.zeros((3, 5), dtype=np.int32)
    for M in (0, 4097):
        status = _lib.lib().tbk_transmission_from_matrices(0, 3, 3, _lib.ptr(H00), _lib.ptr(H01), M, _lib.ptr(V), 5, _lib.ptr(Z), 64, 0, _lib.ptr(its),
                                                           _lib.ptr(T), None)
        assert status == _lib.TBK_ERR_ARGUMENT and "1 to 4096" in _lib.last_error()
    big = np.zeros((1, 1024, 1024), dtype=np.complex128)
    status = _lib.lib().tbk_transmission_from_matrices(0, 1024, 1, _lib.ptr(big), _lib.ptr(big), 17, _lib.ptr(big), 5, _lib.ptr(Z), 64, 0, _lib.ptr(its),
                                                       _lib.ptr(T), None)
    assert status == _lib.TBK_ERR_ARGUMENT and "256 MiB" in _lib.last_error()
    status = _lib.lib().tbk_transmission_from_matrices(0, 1025, 1, _lib.ptr(big), _lib.ptr(big), 1, _lib.ptr(big), 5, _lib.ptr(Z), 64, 0, _lib.ptr(its),
                                                       _lib.ptr(T), None)
    assert status == _lib.TBK_ERR_ARGUMENT and "at most 1024" in _lib.last_error()


# ---- 3. whole calls -------------------------------------------------------------------------------------------------------------------
def _scaled(r_vec, hop):
    """the hoppings scaled so that the norms of the full set add up to 2: the spectrum lies in [-2, 2]"""
    total = sum(np.linalg.norm(m, 2) for m in sm.full_hoppings(r_vec, hop).values())
    return hop * (2.0 / total)


def _synthetic(n, dim, n_r):
    r_vec, hop, pos = syn.dense_model_arrays(n, n_r, syn.MODEL_SEED + 2100 + 10 * n + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, _scaled(r_vec, hop), pos=pos), r_vec


def _reference(model, kpar, axis, L, V):
    """The model's run on principal layers taken from `Model.hamilton` at the 2 L + 1 samples of every in-plane point."""
    kpar = np.asarray(kpar, dtype=float).reshape(len(kpar), -1)
    pts = np.concatenate([sm.sample_points(kp, axis, L, model.dim) for kp in kpar])
    ham = model.hamilton(pts, convention=2).reshape(len(kpar), 2 * L + 1, model.size, model.size)
    pairs = [sm.principal(sm.layers_from_samples(h)) for h in ham]
    H00, H01 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    T, P, its, rho = tm.transmission_function(H00, H01, V, Z)
    bound = np.array([[tm.tolerance(H00[k], H01[k], V, complex(z), its[k, i], rho[k, i], P[k, i]) for i, z in enumerate(Z)] for k in range(len(kpar))])
    gbound = np.array([[tm.green_tolerance(H00[k], H01[k], V, complex(z), its[k, i], rho[k, i]) for i, z in enumerate(Z)] for k in range(len(kpar))])
    return T, (P, gbound), its, bound


@pytest.mark.parametrize("n, dim, n_r, axis, L, M", [(6, 3, 8, 2, 1, 3), (5, 3, 30, 0, 2, 2), (24, 2, 5, 1, 1, 2)])
def test_whole_call_matches_the_model_on_hamilton(n, dim, n_r, axis, L, M):
    model, r_vec = _synthetic(n, dim, n_r)
    assert max(abs(int(R[axis])) for R in r_vec) == L
    kpar = np.random.default_rng(31 + n).random((3, dim - 1)) - 0.5
    V = tm.random_device(n * L, M, 77 + n)
    want, P, its, bound = _reference(model, kpar, axis, L, V)
    assert np.all(bound <= 1e-4)
    got = model.transmission(kpar, Z, axis=axis, device=V, green=True)
    assert got.layers == L and got.length == M and np.array_equal(got.z, Z) and np.array_equal(got.k, kpar)
    assert got.transmission.shape == (3, 5) and got.transmission.dtype == np.float64 and got.green.shape == (3, 5, n * L, n * L)
    err = np.abs(got.transmission - want)
    print("dense %d orbitals dim %d axis %d L = %d M = %d: max|T - model| = %.2e (bounds %.2e ... %.2e)" % (n, dim, axis, L, M, err.max(), 2 * bound.min(),
                                                                                                          2 * bound.max()))
    assert np.all(err <= 2 * bound)
    assert np.array_equal(got.iterations, its) and got.iterations.dtype == np.int32
    assert np.all(np.abs(got.green - P[0]).reshape(3, 5, -1).max(axis=2) <= 2 * P[1])
    plain = model.transmission(kpar, Z, axis=axis - dim, device=V)
    assert len(plain) == 6 and np.array_equal(plain.transmission, got.transmission)
    one = model.transmission(kpar[2], Z[1], axis=axis, device=V)
    assert one.transmission.shape == (1, 1) and one.transmission[0, 0] == got.transmission[2, 1]
    # M pristine layers: zeros against length
    zeros = model.transmission(kpar, Z, axis=axis, device=np.zeros((M, n * L, n * L)))
    length = model.transmission(kpar, Z, axis=axis, length=M)
    assert length.length == M and np.array_equal(zeros.transmission, length.transmission)


def test_csr_twin_two_handles_chunks_and_the_onsite_form():
    n, dim, axis, L, M = 6, 3, 2, 1, 3
    model, _ = _synthetic(n, dim, 8)
    kpar = np.random.default_rng(5).random((7, dim - 1))
    onsite = np.random.default_rng(6).normal(size=(M, n)) * 0.3
    V = np.zeros((M, n, n), dtype=np.complex128)
    V[:, np.arange(n), np.arange(n)] = onsite
    _, _, _, bound = _reference(model, kpar, axis, L, V)
    one = model.transmission(kpar, Z, device=V, green=True)
    short = model.transmission(kpar, Z, device=onsite, green=True)
    assert np.array_equal(short.transmission, one.transmission) and np.array_equal(short.green, one.green), "the (M, N) form has other bits"
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    other = sparse.transmission(kpar, Z, device=V)
    assert np.all(np.abs(other.transmission - one.transmission) <= 2 * bound), "CSR against dense"
    assert np.array_equal(other.iterations, one.iterations)
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.transmission(kpar, Z, device=V, green=True)
    assert len(twin._handles) == 2  # pylint: disable=protected-access
    chunked = pickle.loads(pickle.dumps(model))
    chunked.set_option(_lib.TBK_OPT_K_CHUNK, 3)
    three = chunked.transmission(kpar, Z, device=V, green=True)
    for name, other in (("two handles", two), ("chunks of 3 points", three)):  # the bits of a (k, z) depend on nothing else
        assert np.array_equal(other.iterations, one.iterations), name
        assert np.array_equal(other.transmission, one.transmission) and np.array_equal(other.green, one.green), name + ": other bits than one call"


def _library_calls(model):
    counter = ctypes.c_int64(0)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), _lib.TBK_CNT_LIBRARY_CALLS, ctypes.byref(counter)))  # pylint: disable=protected-access
    return counter.value


def test_forced_library_route_against_the_own_kernel():
    model, _ = _synthetic(5, 3, 30)  # L = 2 along axis 0: 10 rows
    kpar = np.random.default_rng(14).random((3, 2))
    V = tm.random_device(10, 3, 15)
    want, P, its, bound = _reference(model, kpar, 0, 2, V)
    own = model.transmission(kpar, Z, axis=0, device=V)
    assert _library_calls(model) == 0
    model.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    library = model.transmission(kpar, Z, axis=0, device=V, green=True)
    assert _library_calls(model) == 1
    print("library on request: max|T - own kernel| = %.2e, max|T - model| = %.2e" % (np.abs(library.transmission - own.transmission).max(),
                                                                                     np.abs(library.transmission - want).max()))
    assert np.all(np.abs(library.transmission - own.transmission) <= 2 * bound)
    assert np.all(np.abs(library.transmission - want) <= 2 * bound)
    assert np.array_equal(library.iterations, its)
    assert np.all(np.abs(library.green - P[0]).reshape(3, 5, -1).max(axis=2) <= 2 * P[1])


def test_chain_closed_form():
    t_hop, t_plane, eps = 0.8, 0.3, 0.6
    model = tbmodels_amd.Model(hop={(0, 1): np.array([[t_hop]]), (1, 0): np.array([[t_plane]])}, size=1, dim=2, pos=np.zeros((1, 2)),
                               contains_cc=False)
    kpar = np.array([[0.0], [0.17], [0.5]])
    got = model.transmission(kpar, Z, device=[[eps]])
    assert got.layers == 1 and got.length == 1
    _, _, _, bound = _reference(model, kpar, 1, 1, np.full((1, 1, 1), eps, dtype=complex))
    worst = 0.0
    for k in range(3):
        for i, z in enumerate(Z):
            want = tm.chain_closed_form(complex(z), t_hop, t_plane, kpar[k, 0], eps)
            g_s, g_b = sm.chain_closed_form(complex(z), t_hop, t_plane, kpar[k, 0])
            zeta = z - 2 * t_plane * np.cos(2 * np.pi * kpar[k, 0])
            d_g = 64 * U * (abs(zeta) ** 2 + 4 * t_hop ** 2) / abs(1 / g_b) / (2 * t_hop ** 2)  # the closed form's rounding (test_transport_model.py)
            gamma, G = 2 * t_hop ** 2 * abs(g_s.imag), abs(1.0 / (zeta - eps - 2 * t_hop ** 2 * g_s))
            own = d_g * 4 * t_hop ** 2 * (gamma * G ** 2 + gamma ** 2 * G ** 3) + 16 * U * want
            err = abs(got.transmission[k, i] - want)
            assert err <= 2 * bound[k, i] + own < 1e-9, (k, i, err)
            worst = max(worst, err)
    print("chain with an impurity: max|T - closed form| = %.2e" % worst)


def test_errors_and_the_handle_goes_on():
    model, _ = _synthetic(6, 3, 8)
    kpar = np.random.default_rng(9).random((3, 2))
    V = tm.random_device(6, 2, 3)
    with pytest.raises(np.linalg.LinAlgError) as raised:
        model.transmission(kpar, Z, device=V, max_iterations=2)
    print("the cap:", raised.value)
    assert "k index 0 and energy 0 " in str(raised.value) and "2 iterations" in str(raised.value)
    want, _, _, bound = _reference(model, kpar, 2, 1, V)
    got = model.transmission(kpar, Z, device=V)  # the same model and handle
    assert np.all(np.abs(got.transmission - want) <= 2 * bound)
    skew = V.copy()
    skew[1, 0, 1] += 1e-9
    for bad in ({"axis": 3}, {"axis": 0.5}, {"max_iterations": 0}, {"max_iterations": 5000}, {"length": 0}, {"length": 1.5}, {"length": 5000},
                {"device": V[0]}, {"device": np.zeros((2, 5))}, {"device": np.zeros((0, 6, 6))}, {"device": skew}, {"device": 1j * np.ones((2, 6))}):
        with pytest.raises(ValueError):
            model.transmission(kpar, Z, **bad)
    with pytest.raises(ValueError):
        model.transmission(kpar, [0.3, 0.1j])  # a real energy
    flat = tbmodels_amd.Model(hop={(1, 0): np.array([[0.5]])}, size=1, dim=2, pos=np.zeros((1, 2)), contains_cc=False)
    with pytest.raises(ValueError, match="no hopping along axis 1"):
        flat.transmission([[0.1]], Z)


def test_transmission_calls_are_timed_on_their_own_row():
    model, _ = _synthetic(24, 2, 5)
    kpar = np.linspace(0.0, 0.5, 6)[:, None]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.transmission(kpar, Z, length=3)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_transmission_timing(model._staged(), ms, ctypes.byref(calls), 1))  # pylint: disable=protected-access
    print("24 orbitals, 6 points, 5 energies, 3 layers: H(k) and layers %.3f ms, decimation and sweep %.3f ms, output %.3f ms" % (ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_surface_timing(model._staged(), ms, ctypes.byref(calls), 0))  # pylint: disable=protected-access
    assert calls.value == 0
