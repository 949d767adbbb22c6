"""
The dressed lattice Green's function: green_invert_kernel of csrc/tbk_green.hip (and the library route above 64 orbitals) with the
density matrix's phase, Fourier and reduce kernels against tools/dyson_model.py on identical H and Sigma, and
`Model.green_function(self_energy=...)` against numpy.linalg.inv on `Model.hamilton` of the mesh and against its properties.

Bounds (u = 2^-53), none measured on the code under test: dyson_model.tolerance, per energy

    max_k 8 n u rho kappa_2(A) ||A^-1||_2 + 4 (NK + 32) u max_k ||A^-1||_2

with rho the growth factor of the model's elimination (for the library route too: it held, see 20.5), kappa_2 and ||A^-1||_2 from
numpy on the reference A.  The inputs are causal -- Sigma = S - i sign(Im z) Gamma, S Hermitian, Gamma positive semidefinite -- so
||A^-1|| <= 1 / |Im z| and with |Im z| >= 0.05 the bound stays below 1e-9, which is asserted.  A comparison of two computed results is
bounded by the sum of their bounds; against the undressed call that call's documented bound (green_model.whole_call_tolerance) is the
second one.  Every case prints its measured maximum.
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
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import dyson_model  # noqa: E402  pylint: disable=wrong-import-position
import green_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

# both signs of Im z, |Im z| in {0.05, 0.5}; NZ = 5: a ragged last tile (test_gpu_green.py's Z)
Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])
ETA = 0.05
_CACHE = {}


def _vectors(mesh, n_r, seed):
    """test_gpu_green.py's: from three on, the last two are the first one shifted by whole mesh periods and a duplicate."""
    dim = len(mesh)
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, size=(max(1, n_r - 2), dim)).astype(np.int64)
    if n_r < 3:
        return base[:n_r], None, None
    shift = np.array([(-1) ** d * (d + 1) * mesh[d] for d in range(dim)], dtype=np.int64)
    twin = min(1, len(base) - 1)
    R = np.concatenate([base, (base[0] + shift)[None, :], base[twin][None, :]])
    return np.ascontiguousarray(R), (0, n_r - 2), (twin, n_r - 1)


def _inputs(mesh, n):
    """Causal H and Sigma(Z) of dyson_model.causal_case, shared by the cases and never written."""
    key = ("in", mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        H, sigma = dyson_model.causal_case(n, n_k, Z, 8100 + 37 * n_k + n)
        for array in (H, sigma):
            array.setflags(write=False)
        _CACHE[key] = (H, sigma)
    return _CACHE[key]


def _from_matrices(mesh, H, z, sigma, R, k_chunk=0, z_tile=0):
    n = H.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    R = np.ascontiguousarray(R, dtype=np.int64)
    z = np.ascontiguousarray(z, dtype=np.complex128)
    sigma = np.ascontiguousarray(sigma, dtype=np.complex128)
    out = np.full((len(R), len(z), n, n), np.nan + 0j, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_green_dressed_from_matrices(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(H), k_chunk, z_tile, len(z), _lib.ptr(z),
                                                          _lib.ptr(sigma), len(R), _lib.ptr(R), _lib.ptr(out)))
    return out


def _check(got, want, bound, what):
    """max over everything but the energy axis against the per-energy bound"""
    err = np.abs(got - want).max(axis=(0, 2, 3))
    print("%s: max|difference| per energy %s (bounds %s)" % (what, " ".join("%.2e" % e for e in err), " ".join("%.2e" % b for b in bound)))
    assert np.all(np.isfinite(got.view(float))), what
    assert np.all(bound < 1e-9), (what, bound)
    assert np.all(err <= bound), (what, err, bound)


def _model_reference(mesh, n):
    """The model's G at the 17 vectors (the smaller sets are their prefixes' twins: computed per set below), rho and the bound."""
    key = ("ref", mesh, n)
    if key not in _CACHE:
        H, sigma = _inputs(mesh, n)
        sets = {n_r: _vectors(mesh, n_r, 5300 + n_r) for n_r in (1, 3, 17)}
        every = np.concatenate([sets[n_r][0] for n_r in (1, 3, 17)])
        G, rho = dyson_model.dressed_green_function(H, mesh, Z, sigma, every)
        bound = dyson_model.tolerance(H, Z, sigma, rho)
        _CACHE[key] = (sets, {1: G[0:1], 3: G[1:4], 17: G[4:21]}, bound)
    return _CACHE[key]


# ---- 1. the kernels against the model on the same H and Sigma ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 16, 17, 32, 33, 64])
def test_kernels_match_the_model(n):
    for mesh in ((4, 4), (3, 5), (2, 3, 4)):
        H, sigma = _inputs(mesh, n)
        sets, wants, bound = _model_reference(mesh, n)
        for n_r in (1, 3, 17):
            R, shifted, duplicate = sets[n_r]
            first = None
            for chunk in (0, 5, 1):
                got = _from_matrices(mesh, H, Z, sigma, R, chunk)
                _check(got, wants[n_r], bound, "mesh %s n = %d NR = %d chunk %d" % (mesh, n, n_r, chunk))
                if shifted:
                    assert np.array_equal(got[shifted[0]], got[shifted[1]]), (mesh, n, n_r, chunk, "a whole mesh period changed bits")
                    assert np.array_equal(got[duplicate[0]], got[duplicate[1]]), (mesh, n, n_r, chunk, "a duplicate differs")
                if first is None:
                    first = got
                    assert np.array_equal(got, _from_matrices(mesh, H, Z, sigma, R, chunk)), (mesh, n, n_r, "two calls differ")
                    for z_tile in (1, 2):
                        assert np.array_equal(got, _from_matrices(mesh, H, Z, sigma, R, chunk, z_tile)), (mesh, n, n_r, z_tile, "the tile changed bits")


@pytest.mark.parametrize("n", [3, 17, 64])
def test_bits_of_an_energy_do_not_depend_on_the_list(n):
    mesh = (2, 3, 4)
    H, sigma = _inputs(mesh, n)
    R = _vectors(mesh, 3, 5303)[0]
    base = _from_matrices(mesh, H, Z, sigma, R)
    order = [3, 0, 4, 2, 1]
    assert np.array_equal(_from_matrices(mesh, H, Z[order], sigma[order], R), base[:, order]), "a reordered list changed bits"
    for index in (0, 4):  # first and last of the list, alone
        alone = _from_matrices(mesh, H, Z[index:index + 1], sigma[index:index + 1], R)
        assert np.array_equal(alone[:, 0], base[:, index]), "an energy alone has other bits"
    moved = [4, 1, 2, 3, 0]  # the first energy placed last and the last first
    again = _from_matrices(mesh, H, Z[moved], sigma[moved], R, 0, 2)
    assert np.array_equal(again[:, 4], base[:, 0]) and np.array_equal(again[:, 0], base[:, 4])


def _off_diagonal_case(n):
    """Sigma = 40 X, X the exchange of the two halves of the orbitals, H with its diagonal removed and z = +-1e-8 i: the diagonal of
    z - H - Sigma is 1e-8 and its natural pivots sit n / 2 away from it.  Causal (S = 40 X Hermitian, Gamma = 0, Im z != 0); A is
    well conditioned (kappa ~ 1.1, ||A^-1|| ~ 1 / 38: numpy's figures on A go into the bound, not 1 / |Im z|)."""
    mesh = (3, 4)
    H = np.array(_inputs(mesh, n)[0])
    H[:, np.arange(n), np.arange(n)] = 0.0
    half = n // 2
    X = np.zeros((n, n))
    X[np.arange(half), np.arange(half) + half] = 1.0
    X[np.arange(half) + half, np.arange(half)] = 1.0
    z = np.array([1e-8j, -1e-8j])
    sigma = np.ascontiguousarray(np.broadcast_to(40.0 * X + 0j, (2, n, n)))
    return mesh, H, z, sigma


@pytest.mark.parametrize("n", [16, 34, 64])
def test_pivoting_far_from_the_diagonal(n):
    mesh, H, z, sigma = _off_diagonal_case(n)
    R = np.array([[0, 0], [1, -2], [2, 1]], dtype=np.int64)
    want, rho = dyson_model.dressed_green_function(H, mesh, z, sigma, R)
    bound = dyson_model.tolerance(H, z, sigma, rho)
    ref = dyson_model.direct(H, mesh, z, sigma, R)
    # first: the model WITHOUT pivoting violates the bound on this input (pivots of 1e-8 under elements of 40)
    try:
        unpivoted = dyson_model.dressed_green_function(H, mesh, z, sigma, R, pivoting=False)[0]
        err_np = np.abs(unpivoted - ref).max(axis=(0, 2, 3))
    except np.linalg.LinAlgError:
        err_np = np.full(len(z), np.inf)
    print("n = %d without pivoting: %s (bounds %s)" % (n, err_np, bound))
    assert np.any(err_np > bound), "row order alone passes: the case does not test pivoting"
    _check(want, ref, bound, "n = %d model against direct" % n)
    _check(_from_matrices(mesh, H, z, sigma, R), want, bound, "n = %d kernel against the model" % n)


@pytest.mark.parametrize("n", [65, 80])
def test_library_route_above_the_templates(n):
    mesh = (3, 4)
    H, sigma = _inputs(mesh, n)
    R = _vectors(mesh, 3, 5303)[0]
    rho = dyson_model.dressed_green_function(H, mesh, Z, sigma, R[:1])[1]
    bound = dyson_model.tolerance(H, Z, sigma, rho)
    for chunk in (0, 5):
        got = _from_matrices(mesh, H, Z, sigma, R, chunk)
        _check(got, dyson_model.direct(H, mesh, Z, sigma, R), bound, "n = %d chunk %d library route against direct" % (n, chunk))
    assert np.array_equal(got[0], got[2])  # the shifted twin


# ---- 2. whole calls ------------------------------------------------------------------------------------------------------------------
def _synthetic(n, dim, plus=None):
    r_vec, hop, pos = syn.dense_model_arrays(n, 5, syn.MODEL_SEED + 2000 + 10 * n + dim, dim=dim)
    hop = 2.0 * hop
    if plus is not None:
        hop[0] = hop[0] + plus / 2  # (the packed R = 0 block is half of the on-site matrix)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def _sigma_for(n, seed):
    return dyson_model.causal_case(n, 1, Z, seed)[1]


def _whole_reference(model, mesh, key):
    if key not in _CACHE:
        kpts = dos_model.mesh_kpoints(mesh)
        ham = np.ascontiguousarray(model.hamilton(kpts, convention=2))
        ham.setflags(write=False)
        _CACHE[key] = ham
    return _CACHE[key]


def _undressed_bound(model, mesh, ham, z, eta):
    eig, vec = model.eigh(dos_model.mesh_kpoints(mesh))
    eig, vec = np.array(eig), np.array(vec)
    r_vec, _ = model.packed_hop()
    return green_model.whole_call_tolerance(ham, eig, vec, eta, green_model.resolvent(ham, mesh, z, r_vec))


@pytest.mark.parametrize("n, mesh", [(8, (4, 4)), (8, (2, 3, 4)), (24, (4, 4)), (24, (2, 3, 4))])
def test_whole_call(n, mesh):
    model = _synthetic(n, len(mesh))
    ham = _whole_reference(model, mesh, ("ham", n, mesh))
    sigma = _sigma_for(n, 8800 + n)
    r_vec, _ = model.packed_hop()
    rho = dyson_model.dressed_green_function(ham, mesh, Z, sigma, r_vec[:1])[1]
    bound = dyson_model.tolerance(ham, Z, sigma, rho)
    result = model.green_function(mesh, Z, self_energy=sigma)
    assert isinstance(result, tbmodels_amd.GreenFunction) and np.array_equal(result.R, r_vec) and np.array_equal(result.z, Z)
    assert result.G.shape == (len(r_vec), len(Z), n, n) and result.G.dtype == np.complex128
    # (H(k) of the call and of Model.hamilton may come from different chunkings: the same few roundings, inside the bound)
    _check(result.G, dyson_model.direct(ham, mesh, Z, sigma, r_vec), bound, "n = %d %s against direct" % (n, mesh))
    assert np.array_equal(result.G, model.green_function(mesh, Z, self_energy=sigma).G)
    # Sigma = 0 against the undressed call
    zero = np.zeros_like(sigma)
    rho0 = dyson_model.dressed_green_function(ham, mesh, Z, zero, r_vec[:1])[1]
    plain = model.green_function(mesh, Z)
    both = dyson_model.tolerance(ham, Z, zero, rho0) + _undressed_bound(model, mesh, ham, Z, ETA)
    _check(model.green_function(mesh, Z, self_energy=zero).G, plain.G, both, "n = %d %s Sigma = 0 against the undressed call" % (n, mesh))
    # Sigma = s 1 against the undressed call at z - s (Im s of the sign opposite to Im z: |Im (z - s)| >= |Im z|)
    s = np.array([0.2 - 0.1j, -0.3 + 0.2j, 0.1 - 0.3j, 0.4 + 0.01j, -0.2j])
    scalar = np.ascontiguousarray(s[:, None, None] * np.eye(n)[None])
    rho_s = dyson_model.dressed_green_function(ham, mesh, Z, scalar, r_vec[:1])[1]
    both = dyson_model.tolerance(ham, Z, scalar, rho_s) + _undressed_bound(model, mesh, ham, Z - s, ETA)
    _check(model.green_function(mesh, Z, self_energy=scalar).G, model.green_function(mesh, Z - s).G, both,
           "n = %d %s Sigma = s 1 against z - s" % (n, mesh))
    # Sigma = S Hermitian against the undressed call of the model with S on site
    rng = np.random.default_rng(8900 + n)
    S = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    S = 0.1 * (S + S.conj().T)
    const = np.ascontiguousarray(np.broadcast_to(S, (len(Z), n, n)))
    shifted = _synthetic(n, len(mesh), plus=S)
    ham_s = np.ascontiguousarray(shifted.hamilton(dos_model.mesh_kpoints(mesh), convention=2))
    rho_c = dyson_model.dressed_green_function(ham, mesh, Z, const, r_vec[:1])[1]
    both = dyson_model.tolerance(ham, Z, const, rho_c) + _undressed_bound(shifted, mesh, ham_s, Z, ETA)
    _check(model.green_function(mesh, Z, self_energy=const).G, shifted.green_function(mesh, Z).G, both,
           "n = %d %s Sigma = S against the model with S on site" % (n, mesh))
    # G(R, conj z; Sigma^H) = G(-R, z; Sigma)^H
    sigma_h = np.ascontiguousarray(np.conj(np.transpose(sigma, (0, 2, 1))))
    rho_h = dyson_model.dressed_green_function(ham, mesh, np.conj(Z), sigma_h, r_vec[:1])[1]
    both = bound + dyson_model.tolerance(ham, np.conj(Z), sigma_h, rho_h)
    mirror = model.green_function(mesh, np.conj(Z), R=-r_vec, self_energy=sigma_h).G
    _check(mirror, np.conj(np.transpose(result.G, (0, 1, 3, 2))), both, "n = %d %s conjugation symmetry" % (n, mesh))


def test_dyson_equation_over_the_dual_cell():
    n, mesh = 8, (4, 4)
    model = _synthetic(n, 2)
    ham = _whole_reference(model, mesh, ("ham", n, mesh))
    sigma = _sigma_for(n, 8800 + n)
    r_vec, hop = model.packed_hop()
    torus = green_model.torus_hoppings(mesh, r_vec, hop)
    cell = np.array([[i, j] for i in range(4) for j in range(4)], dtype=np.int64)
    G = model.green_function(mesh, Z, R=cell, self_energy=sigma).G
    rho = dyson_model.dressed_green_function(ham, mesh, Z, sigma, cell[:1])[1]
    bound = dyson_model.tolerance(ham, Z, sigma, rho)
    worst = 0.0
    for zi, z in enumerate(Z):
        for vec in cell:
            total = np.zeros((n, n), dtype=complex)
            for rp, vecp in enumerate(cell):
                diff = np.mod(vec - vecp, mesh)
                kernel = -torus[rp] + ((z * np.eye(n) - sigma[zi]) if not vecp.any() else 0)
                total += kernel @ G[diff[0] * 4 + diff[1], zi]
            worst = max(worst, np.abs(total - (np.eye(n) if not vec.any() else 0)).max())
    # 16 products of the kernel's blocks with G, every element of G within its bound: n ||kernel||_2 bound each
    norm = sum(np.linalg.norm(t, 2) for t in torus) + np.abs(Z).max() + max(np.linalg.norm(s, 2) for s in sigma)
    limit = norm * n * bound.max()
    print("Dyson equation over the dual cell of %s: max residual %.2e (bound %.2e)" % (mesh, worst, limit))
    assert worst <= limit < 1e-8


def test_csr_twin_two_handles_and_the_real_axis():
    n, mesh = 8, (2, 3, 4)
    model = _synthetic(n, 3)
    ham = _whole_reference(model, mesh, ("ham", n, mesh))
    sigma = _sigma_for(n, 8800 + n)
    r_vec, _ = model.packed_hop()
    rho = dyson_model.dressed_green_function(ham, mesh, Z, sigma, r_vec[:1])[1]
    bound = dyson_model.tolerance(ham, Z, sigma, rho)
    one = model.green_function(mesh, Z, self_energy=sigma)
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    _check(sparse.green_function(mesh, Z, self_energy=sigma).G, one.G, bound, "CSR against dense")
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.green_function(mesh, Z, self_energy=sigma)
    assert len(twin._handles) == 2
    _check(two.G, one.G, bound, "two handles against one")
    # real energies: Sigma's anti-Hermitian part -0.2 1 is the only broadening (||A^-1|| <= 1 / 0.2)
    rng = np.random.default_rng(8950)
    S = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    real_z = np.array([-0.7, 0.0, 0.45])
    dressed = np.ascontiguousarray(np.broadcast_to(0.1 * (S + S.conj().T) - 0.2j * np.eye(n), (3, n, n)))
    rho_r = dyson_model.dressed_green_function(ham, mesh, real_z, dressed, r_vec[:1])[1]
    got = model.green_function(mesh, real_z, self_energy=dressed)
    assert np.array_equal(got.z, real_z.astype(complex))
    _check(got.G, dyson_model.direct(ham, mesh, real_z, dressed, r_vec), dyson_model.tolerance(ham, real_z, dressed, rho_r), "real z")
    with pytest.raises(ValueError):
        model.green_function(mesh, real_z)
    # one energy and one matrix
    single = model.green_function(mesh, 0.45, self_energy=dressed[2], R=[0, 0, 0])
    assert single.G.shape == (1, 1, n, n)
    assert np.array_equal(single.G[0, 0], model.green_function(mesh, real_z, self_energy=dressed, R=[0, 0, 0]).G[0, 2])


# ---- 3. a singular matrix is a status, the undressed call keeps its bits, timing ------------------------------------------------------
def test_singular_input_raises_and_the_handle_goes_on():
    eps = np.array([0.5, -0.25, 1.0])
    model = tbmodels_amd.Model(on_site=list(eps), size=3, dim=2, pos=np.zeros((3, 2)))
    mesh = (3, 2)
    z = np.array([0.1 + 0.1j, 0.3 + 0.2j, -0.4 - 0.1j])
    sigma = np.zeros((3, 3, 3), dtype=complex)
    sigma[1] = z[1] * np.eye(3) - np.diag(eps)  # z 1 - H - Sigma = 0 exactly at energy 1, at every mesh point
    with pytest.raises(np.linalg.LinAlgError) as raised:
        model.green_function(mesh, z, self_energy=sigma)
    print("singular input:", raised.value)
    assert "energy 1 " in str(raised.value) and "mesh point (0, 0)" in str(raised.value) and "Singular matrix" in str(raised.value)
    sigma[1] = 0.0
    again = model.green_function(mesh, z, self_energy=sigma, R=[[0, 0]])  # the same model and handle
    want = np.array([np.diag(1.0 / (zz - eps)) for zz in z])
    assert np.abs(again.G[0] - want).max() <= 4 * (6 + 32) * 2.0 ** -53 / 0.1 + 8 * 3 * 2.0 ** -53 * 100  # diagonal A: rho = 1, kappa ||A^-1|| <= 100
    # the same through the kernels alone: one (k, z) singular in the middle of a chunk
    H, sg = _inputs((4, 4), 17)
    bad = np.array(sg)
    bad[3] = Z[3] * np.eye(17) - H[6]
    out = np.zeros((1, 5, 17, 17), dtype=np.complex128)
    mesh32, R0 = np.array([4, 4], dtype=np.int32), np.zeros((1, 2), dtype=np.int64)
    status = _lib.lib().tbk_green_dressed_from_matrices(0, 2, _lib.ptr(mesh32), 17, _lib.ptr(H), 0, 0, 5, _lib.ptr(Z), _lib.ptr(bad), 1, _lib.ptr(R0),
                                                        _lib.ptr(out))
    assert status == _lib.TBK_ERR_SINGULAR and "mesh point (1, 2)" in _lib.last_error() and "energy 3 " in _lib.last_error(), _lib.last_error()


def test_the_undressed_call_keeps_its_bits():
    model, mesh = _synthetic(8, 2), (4, 4)
    got = model.green_function(mesh, Z, self_energy=None)
    r_vec, _ = model.packed_hop()
    vectors = np.ascontiguousarray(r_vec, dtype=np.int64)
    direct = np.empty_like(got.G)
    mesh32 = np.array(mesh, dtype=np.int32)
    _lib.check(_lib.lib().tbk_green_function(model._staged(), _lib.ptr(mesh32), len(Z), _lib.ptr(Z), len(vectors), _lib.ptr(vectors), _lib.ptr(direct)))
    assert np.array_equal(got.G, direct)


def test_dressed_calls_are_timed_on_their_own_row_and_the_library_route_is_counted():
    n, mesh = 24, (4, 4)
    model = _synthetic(n, 2)
    sigma = _sigma_for(n, 8800 + n)
    ham = _whole_reference(model, mesh, ("ham", n, mesh))
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    own = model.green_function(mesh, Z, self_energy=sigma)
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_green_dressed_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("n = 24 (4, 4), 5 energies: phase table %.3f ms, inversions %.3f ms, contractions %.3f ms" % (ms[0], ms[1], ms[2]))
    assert calls.value == 1 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_green_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 0  # the undressed family counts its own calls
    # the library route on request: the same quantity within the bound
    counter = ctypes.c_int64(0)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), _lib.TBK_CNT_LIBRARY_CALLS, ctypes.byref(counter)))
    before = counter.value
    model.set_option(_lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER)
    library = model.green_function(mesh, Z, self_energy=sigma)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), _lib.TBK_CNT_LIBRARY_CALLS, ctypes.byref(counter)))
    assert counter.value == before + 1
    r_vec, _ = model.packed_hop()
    rho = dyson_model.dressed_green_function(ham, mesh, Z, sigma, r_vec[:1])[1]
    _check(library.G, own.G, 2 * dyson_model.tolerance(ham, Z, sigma, rho), "library route against the own kernel")
