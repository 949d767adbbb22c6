"""
The projector kernel of csrc/tbk_green.hip with the density matrix's phase, Fourier and reduce kernels against tools/green_model.py
on identical (E, U), and `Model.green_function` against the resolvent numpy.linalg.inv(z - H(k)) and against its properties.

Bounds (u = 2^-53, eta = min |Im z| of the call), none measured on the code under test:

  kernels against the model: green_tolerance(NK, n, eta) = 4 (NK n + 32) u / eta per component -- an element of G is a sum of NK n
      terms whose moduli add up to at most 1 / eta; the 32 covers the roundings of g, the complex multiplies and sincospi.
  whole call against the resolvent: twice max_k (||U U^H - 1|| + ||H U - U E|| ||U|| / eta) / eta, evaluated from `Model.eigh` and
      `Model.hamilton` of the same mesh (the call's own eigenvectors may come from another chunking, hence the factor 2), plus
      green_tolerance, plus 4 n u ||G_ref|| for the reference's inverse (green_model.whole_call_tolerance).  With |Im z| >= 0.05
      this stays below 1e-9, which the tests assert.
  G(R, conj z) = G(-R, z)^H: twice green_tolerance.  The spectral sum from `eigenval_array`: n green_tolerance plus n times the
      eigenvalue term 2 max_k ||H U - U E|| ||U|| / eta^2.  CSR against dense, two handles against one: green_tolerance.
Every case prints its measured maximum.
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
import green_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

# both signs of Im z, |Im z| in {0.05, 0.5}; 0.3: inside the real range [-2, 2] of the random spectra; NZ = 5: a ragged last tile
Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])
ETA = 0.05
_CACHE = {}


def _eigensystem(mesh, n):
    """Random E in [-2, 2] and random unitary U, shared by the cases and never written."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(7100 + 37 * n_k + n)
        eig = np.sort(rng.uniform(-2.0, 2.0, (n_k, n)), axis=-1)
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        for array in (eig, U):
            array.setflags(write=False)
        _CACHE[key] = (eig, U)
    return _CACHE[key]


def _vectors(mesh, n_r, seed):
    """n_r vectors from {-3 .. 3}^dim; from three on, the last two are the first one shifted by whole mesh periods and a duplicate
    of the second (of the first when there is no second)."""
    dim = len(mesh)
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, size=(max(1, n_r - 2), dim)).astype(np.int64)
    if n_r < 3:
        return base[:n_r], None, None
    shift = np.array([(-1) ** d * (d + 1) * mesh[d] for d in range(dim)], dtype=np.int64)
    twin = min(1, len(base) - 1)
    R = np.concatenate([base, (base[0] + shift)[None, :], base[twin][None, :]])
    return np.ascontiguousarray(R), (0, n_r - 2), (twin, n_r - 1)


def _from_eigensystem(mesh, eig, U, z, R, k_chunk=0, z_tile=0):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    R = np.ascontiguousarray(R, dtype=np.int64)
    z = np.ascontiguousarray(z, dtype=np.complex128)
    out = np.full((len(R), len(z), n, n), np.nan + 0j, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_green_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), k_chunk, z_tile, len(z),
                                                     _lib.ptr(z), len(R), _lib.ptr(R), _lib.ptr(out)))
    return out


def _plan(rows, n_orb, n_r, n_z, z_tile=0, k_chunk=0):
    out = (ctypes.c_int64 * 7)()
    _lib.check(_lib.lib().tbk_green_plan(rows, n_orb, n_r, n_z, z_tile, k_chunk, out))
    return dict(zip(("nr_pad", "slices", "kps", "z_tile", "tiles", "k_chunk", "template"), out))


def _kernel_case(mesh, n, n_r, chunks=(0, 5, 1)):
    eig, U = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    R, shifted, duplicate = _vectors(mesh, n_r, 5300 + n_r)
    want = green_model.green_function(eig, U, mesh, Z, R)
    bound, worst = green_model.green_tolerance(n_k, n, ETA), 0.0
    first = None
    for chunk in chunks:
        got = _from_eigensystem(mesh, eig, U, Z, R, chunk)
        err = np.abs(got - want).max()
        worst = max(worst, err)
        assert np.all(np.isfinite(got.view(float))) and err <= bound, (mesh, n, n_r, chunk, err, bound)
        if shifted:
            assert np.array_equal(got[shifted[0]], got[shifted[1]]), (mesh, n, n_r, chunk, "a whole mesh period changed bits")
            assert np.array_equal(got[duplicate[0]], got[duplicate[1]]), (mesh, n, n_r, chunk, "a duplicate differs")
        if first is None:
            first = got
            assert np.array_equal(got, _from_eigensystem(mesh, eig, U, Z, R, chunk)), (mesh, n, n_r, "two calls differ")
            for z_tile in (1, 2):
                assert np.array_equal(got, _from_eigensystem(mesh, eig, U, Z, R, chunk, z_tile)), (mesh, n, n_r, z_tile, "the tile changed bits")
    return worst, bound, first


# ---- 1. the kernels against the model on the same (E, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16, 17, 33, 64, 65])
def test_kernels_match_the_model_on_2x3x2(n):
    mesh = (2, 3, 2)
    plan = _plan(12, n, 33, len(Z))
    assert plan["slices"] == 1 and plan["template"] == (1 if n <= 16 else 4) and plan["z_tile"] == 4 and plan["tiles"] == 2
    for n_r in (1, 5, 16, 17, 33):
        worst, bound, _ = _kernel_case(mesh, n, n_r)
        print("mesh %s n = %d NR = %d: max|G - model| = %.3e (bound %.3e)" % (mesh, n, n_r, worst, bound))


@pytest.mark.parametrize("mesh", [(3, 4), (1, 5)])
def test_kernels_match_the_model_in_two_dimensions(mesh):
    worst, bound, _ = _kernel_case(mesh, 9, 17)
    print("mesh %s n = 9 NR = 17: max|G - model| = %.3e (bound %.3e)" % (mesh, worst, bound))


def test_sliced_contraction_matches_the_model_and_the_plan():
    mesh, n, n_r = (4, 4, 4), 8, 33
    plan = _plan(64, n, n_r, len(Z))
    dm = (ctypes.c_int64 * 3)()
    _lib.check(_lib.lib().tbk_dm_plan(64, n, n_r, dm))
    print("plan of 64 points, 8 orbitals, 33 vectors, 5 energies:", plan)
    assert [plan["nr_pad"], plan["slices"], plan["kps"]] == list(dm)  # the density matrix's slices, whatever the energies
    assert plan["slices"] > 1 and plan["kps"] % 4 == 0 and plan["nr_pad"] == 48 and plan["k_chunk"] == 64
    assert _plan(64, n, n_r, 1)["z_tile"] == 1 and _plan(64, n, n_r, 64, 2)["tiles"] == 32 and _plan(64, n, n_r, 64, 9)["z_tile"] == 4
    assert _plan(64, n, n_r, 5, 0, 24)["k_chunk"] == 24
    worst, bound, first = _kernel_case(mesh, n, n_r, chunks=(0, 5, 1, 24))  # 5 and 24: chunks that end inside a slice and inside a group
    print("mesh %s n = %d NR = %d, %d slices: max|G - model| = %.3e (bound %.3e)" % (mesh, n, n_r, plan["slices"], worst, bound))
    # the plan's own numbers, given explicitly, are what 0 / 0 did
    eig, U = _eigensystem(mesh, n)
    R = _vectors(mesh, n_r, 5300 + n_r)[0]
    assert np.array_equal(first, _from_eigensystem(mesh, eig, U, Z, R, plan["k_chunk"], plan["z_tile"]))


@pytest.mark.parametrize("mesh, n", [((2, 3, 2), 9), ((2, 3, 2), 33), ((4, 4, 4), 8)])
def test_bits_of_an_energy_do_not_depend_on_the_list(mesh, n):
    eig, U = _eigensystem(mesh, n)
    R = _vectors(mesh, 5, 5305)[0]
    base = _from_eigensystem(mesh, eig, U, Z, R)
    order = [3, 0, 4, 2, 1]
    again = _from_eigensystem(mesh, eig, U, Z[order], R)
    assert np.array_equal(again, base[:, order]), "a reordered list changed bits"
    doubled = _from_eigensystem(mesh, eig, U, np.concatenate([Z, Z[1:2], Z[:1]]), R, 0, 2)
    assert np.array_equal(doubled[:, :5], base) and np.array_equal(doubled[:, 5], base[:, 1]) and np.array_equal(doubled[:, 6], base[:, 0])
    for index in (0, 4):
        alone = _from_eigensystem(mesh, eig, U, Z[index:index + 1], R)
        assert np.array_equal(alone[:, 0], base[:, index]), "an energy alone has other bits"


def test_phase_reduction_near_the_ends_of_the_integers():
    mesh, n = (2, 3, 2), 3
    eig, U = _eigensystem(mesh, n)
    R = np.array([[1, -2, 3], [1 + 2 * 2 ** 30, -2 - 3 * (2 ** 31 // 3), 3 + 2 * (2 ** 30 - 1)], [1 - 2 * 2 ** 30, -2, 3 - 2 ** 31],
                  [1 + 2 * 2 ** 61, -2 - 3 * 2 ** 61, 3], [1 - 2 ** 63, -2, 3]], dtype=np.int64)
    got = _from_eigensystem(mesh, eig, U, Z, R)
    for other in got[1:]:
        assert np.array_equal(got[0], other)


# ---- 2. whole calls ------------------------------------------------------------------------------------------------------------------
def _silicon():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])


def _dense9(dim):
    r_vec, hop, pos = syn.dense_model_arrays(9, 6, syn.MODEL_SEED + 1400 + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


def _reference(model, mesh, key):
    """H(k), E, U of the mesh from the existing calls, the resolvent at the stored vectors and its whole-call bound: once per model."""
    if key not in _CACHE:
        kpts = dos_model.mesh_kpoints(mesh)
        ham = np.array(model.hamilton(kpts, convention=2))
        eig, vec = model.eigh(kpts)
        eig, vec = np.array(eig), np.array(vec)
        r_vec, _ = model.packed_hop()
        ref = green_model.resolvent(ham, mesh, Z, r_vec)
        bound = green_model.whole_call_tolerance(ham, eig, vec, ETA, ref)
        resid = max(np.linalg.norm(h @ u - u * e[None, :], 2) * np.linalg.norm(u, 2) for h, e, u in zip(ham, eig, vec))
        for array in (ref,):
            array.setflags(write=False)
        _CACHE[key] = (ref, bound, resid)
    return _CACHE[key]


@pytest.mark.parametrize("name, mesh", [("silicon", (2, 3, 2)), ("dense9_2d", (3, 4)), ("dense9_3d", (2, 3, 2))])
def test_whole_call_is_the_resolvent(name, mesh):
    model = _silicon() if name == "silicon" else _dense9(len(mesh))
    n, n_k = model.size, int(np.prod(mesh))
    ref, bound, resid = _reference(model, mesh, (name, mesh))
    tol = green_model.green_tolerance(n_k, n, ETA)
    result = model.green_function(mesh, Z)
    assert isinstance(result, tbmodels_amd.GreenFunction)
    r_vec, _ = model.packed_hop()
    assert result.R.dtype == np.int64 and np.array_equal(result.R, r_vec) and np.array_equal(result.z, Z) and result.z.dtype == np.complex128
    assert result.G.shape == (len(r_vec), len(Z), n, n) and result.G.dtype == np.complex128
    err = np.abs(result.G - ref).max()
    print("%s %s, %d vectors: max|G - resolvent| = %.3e (bound %.3e)" % (name, mesh, len(r_vec), err, bound))
    assert bound < 1e-9 and err <= bound
    assert np.array_equal(result.G, model.green_function(mesh, Z).G)  # the same call again: the same bits
    # G(R, conj z) = G(-R, z)^H
    mirror = model.green_function(mesh, np.conj(Z), R=-r_vec).G
    err_h = np.abs(mirror - np.conj(np.transpose(result.G, (0, 1, 3, 2)))).max()
    print("%s %s: max|G(R, conj z) - G(-R, z)^H| = %.3e (bound %.3e)" % (name, mesh, err_h, 2 * tol))
    assert err_h <= 2 * tol
    # one vector, one energy; the spectral sum from the eigenvalue path
    origin = model.green_function(mesh, Z[0], R=[0] * len(mesh))
    assert origin.G.shape == (1, 1, n, n) and origin.R.shape == (1, len(mesh)) and origin.z.shape == (1,)
    eig = np.array(model.eigenval_array(dos_model.mesh_kpoints(mesh)))
    lorentz = float(np.sum((ETA / np.pi) / ((Z[0].real - eig) ** 2 + ETA ** 2))) / n_k
    got = -np.trace(origin.G[0, 0]).imag / np.pi
    bound_s = n * tol + n * 2 * resid / ETA ** 2
    print("%s %s: spectral sum %.12g, from eigenval_array %.12g (bound %.3e)" % (name, mesh, got, lorentz, bound_s))
    assert abs(got - lorentz) <= bound_s
    # TBK_OPT_K_CHUNK = 5
    model.set_option(_lib.TBK_OPT_K_CHUNK, 5)
    err_c = np.abs(model.green_function(mesh, Z).G - ref).max()
    print("%s %s, chunks of 5: max|G - resolvent| = %.3e (bound %.3e)" % (name, mesh, err_c, bound))
    assert err_c <= bound


def test_csr_twin_and_two_handles():
    model, mesh = _silicon(), (2, 3, 2)
    ref, bound, _ = _reference(model, mesh, ("silicon", mesh))
    tol = green_model.green_tolerance(12, model.size, ETA)
    one = model.green_function(mesh, Z)
    sparse = pickle.loads(pickle.dumps(model))
    sparse.set_sparse()
    csr = sparse.green_function(mesh, Z)
    err = np.abs(csr.G - one.G).max()
    print("silicon, CSR against dense: %.3e (bound %.3e)" % (err, tol))
    assert err <= tol and np.abs(csr.G - ref).max() <= bound
    twin = pickle.loads(pickle.dumps(model))
    twin.devices = [0, 0]
    two = twin.green_function(mesh, Z)
    assert len(twin._handles) == 2
    err = np.abs(two.G - one.G).max()
    print("silicon, two handles against one: %.3e (bound %.3e)" % (err, tol))
    assert err <= tol and np.abs(two.G - ref).max() <= bound


# ---- 3. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    model.green_function((4, 4, 4), Z)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_green_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    dm_ms, dm_calls = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_dm_timing(model._staged(), dm_ms, ctypes.byref(dm_calls), 0))
    assert dm_calls.value == 0  # the density matrix counts its own calls
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    model.green_function((4, 4, 4), Z)
    _lib.check(_lib.lib().tbk_green_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 5 energies: %d calls, phase table %.3f ms, projectors %.3f ms, contraction %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    _lib.check(_lib.lib().tbk_green_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 0 and list(ms) == [0.0, 0.0, 0.0]


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U = _eigensystem((2, 3, 2), 9)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    zero = np.array([2, 0, 2], dtype=np.int32)
    R = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    z2 = np.array([0.1 + 0.2j, -0.3j])
    out = np.zeros((2, 2, 9, 9), dtype=np.complex128)
    real_axis, nan_z, inf_z = np.array([0.1 + 0.2j, 0.5 + 0j]), np.array([complex(np.nan, 1.0), 1j]), np.array([1j, complex(0.0, np.inf)])
    many = np.full(4097, 1j)

    def call(dim=3, mesh_=mesh, n_orb=9, eig_=eig, U_=U, chunk=0, tile=0, n_z=2, z_=z2, n_r=2, R_=R, out_=out):
        return lib.tbk_green_from_eigensystem(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(U_), chunk, tile, n_z, _lib.ptr(z_), n_r,
                                              _lib.ptr(R_), _lib.ptr(out_))

    assert call() == _lib.TBK_OK
    bad = [call(dim=1), call(dim=4), call(mesh_=zero), call(mesh_=None), call(eig_=None), call(U_=None), call(R_=None), call(out_=None),
           call(z_=None), call(n_orb=0), call(chunk=-1), call(tile=-1), call(n_r=0), call(n_r=-3), call(n_z=0), call(n_z=4097, z_=many),
           call(z_=real_axis), call(z_=nan_z), call(z_=inf_z)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    assert "Im z" in _lib.last_error() or "finite" in _lib.last_error()
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 7)()
    out8 = np.zeros((2, 2, 8, 8), dtype=np.complex128)
    m32, pz, pr, po = _lib.ptr(mesh), _lib.ptr(z2), _lib.ptr(R), _lib.ptr(out8)
    # a k.p handle: tbk_kdotp holds the tbk_model of its dense pipeline as its first member (csrc/tbk_internal.h)
    kp = tbmodels_amd.KdotpModel({(0, 0, 0): np.eye(2, dtype=complex), (1, 0, 0): np.array([[0, 1], [1, 0]], dtype=complex)})
    core = ctypes.c_void_p(ctypes.c_void_p.from_address(kp._staged().value).value)
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)
    line = one_d._staged_all()[0]
    out2 = np.zeros((2, 2, 2, 2), dtype=np.complex128)
    bad = [lib.tbk_green_function(None, m32, 2, pz, 2, pr, po), lib.tbk_green_function(handle, None, 2, pz, 2, pr, po),
           lib.tbk_green_function(handle, m32, 0, pz, 2, pr, po), lib.tbk_green_function(handle, m32, 4097, _lib.ptr(many), 2, pr, po),
           lib.tbk_green_function(handle, m32, 2, None, 2, pr, po), lib.tbk_green_function(handle, m32, 2, _lib.ptr(real_axis), 2, pr, po),
           lib.tbk_green_function(handle, m32, 2, _lib.ptr(nan_z), 2, pr, po), lib.tbk_green_function(handle, m32, 2, pz, 0, pr, po),
           lib.tbk_green_function(handle, m32, 2, pz, 2, None, po), lib.tbk_green_function(handle, m32, 2, pz, 2, pr, None),
           lib.tbk_green_function(handle, _lib.ptr(zero), 2, pz, 2, pr, po), lib.tbk_green_function(core, m32, 2, pz, 2, pr, _lib.ptr(out2)),
           lib.tbk_green_function(line, m32, 2, pz, 2, pr, _lib.ptr(out2)),
           lib.tbk_green_function_multi(twice, 2, m32, 2, pz, 2, pr, po), lib.tbk_green_function_multi(None, 1, m32, 2, pz, 2, pr, po),
           lib.tbk_green_timing(None, ms, ctypes.byref(calls), 0), lib.tbk_green_timing(handle, None, ctypes.byref(calls), 0),
           lib.tbk_green_timing(handle, ms, None, 0), lib.tbk_green_plan(0, 8, 2, 1, 0, 0, plan), lib.tbk_green_plan(64, 0, 2, 1, 0, 0, plan),
           lib.tbk_green_plan(64, 8, 0, 1, 0, 0, plan), lib.tbk_green_plan(64, 8, 2, 0, 0, 0, plan), lib.tbk_green_plan(64, 8, 2, 4097, 0, 0, plan),
           lib.tbk_green_plan(64, 8, 2, 1, -1, 0, plan), lib.tbk_green_plan(64, 8, 2, 1, 0, -1, plan), lib.tbk_green_plan(64, 8, 2, 1, 0, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    _lib.check(lib.tbk_green_timing(handle, ms, ctypes.byref(calls), 0))
    assert calls.value == 0  # none of the refused calls reached the device
    with pytest.raises(ValueError):
        one_d.green_function((4,), 1j)
    with pytest.raises(ValueError):
        model.green_function((2, 2, 2), 0.5)
    with pytest.raises(ValueError):
        model.green_function((2, 2, 2), [1j, complex(np.nan, 1.0)])
