"""
tools/device_model.py, the NumPy statement of the layer-resolved Green's functions of the device, on the CPU: the
blocks G_p, F_p, C_p against the blocks of the dense block-tridiagonal inverse and against the same sweeps in mpmath at 60 digits, the
four properties of the model's docstring, the chain with one impurity against its closed-form local G, the argument errors, the C
signatures and the stored mpmath reference of the GPU cases.

Bounds (u = 2^-53), none measured on the code under test: device_model.tolerance, per component of a block B of layer p

    E c(B) s(B),    E = 8 N u rho (|z| + |H00|_2 + 2 |H01|_2 + max |V_p|_2) / eta (iterations + M + 1)      (transport_model's eps)

with c the number of error-carrying factors behind B and s the product of the 2-norms of the blocks B is formed from.
The GPU cases' bounds stay at or below 22.5's ceiling of 1e-4, which is asserted here for all of them.  Every case prints its measured
maximum.
"""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tbmodels_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import device_model as dm  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])  # tests/test_gpu_surface.py's
U = 2.0 ** -53
CASES = [(1, 1, 1), (3, 1, 4), (4, 2, 3), (6, 1, 1), (6, 1, 5)]
SMALL = [(1, 1, 1), (3, 1, 4), (4, 2, 3)]  # mpmath on these
_CACHE = {}


def _case(n, L, M):
    """One in-plane point: layers, a random Hermitian device of norm 0.5, the model's run at the five energies and its bounds."""
    key = (n, L, M)
    if key not in _CACHE:
        _, H00, H01 = tm.random_case(n, L, 1, 6100 + 37 * n + L)
        V = tm.random_device(n * L, M, 6200 + 37 * n + M)
        results, bounds = dm.device_green_function(H00, H01, V, Z)
        for array in (H00, H01, V):
            array.setflags(write=False)
        _CACHE[key] = (H00[0], H01[0], V, results[0], bounds[0])
    return _CACHE[key]


def _dense_own(H00, H01, V, z):
    """numpy's inversion of the (M N) x (M N) matrix, per component: |A^-1| <= 1 / eta, kappa <= (|z| + |H|) / eta"""
    size = np.linalg.norm(H00, 2) + 2 * np.linalg.norm(H01, 2) + max(np.linalg.norm(v, 2) for v in V)
    return 8 * V.shape[0] * H00.shape[0] * U * (abs(z) + size) / z.imag ** 2


def _layer_max(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


@pytest.mark.parametrize("n, L, M", CASES)
def test_blocks_against_the_dense_inverse(n, L, M):
    H00, H01, V, results, bounds = _case(n, L, M)
    worst = 0.0
    for z, r, tol in zip(Z, results, bounds):
        G, F, C, _ = dm.device_dense(H00, H01, V, complex(z))
        own = _dense_own(H00, H01, V, z)
        for name, got, want, limit in (("G", r.G, G, tol.G), ("F", r.F, F, tol.F), ("C", r.C, C, tol.C)):
            err = _layer_max(got - want)
            worst = max(worst, err.max())
            assert np.all(err <= limit + own), (name, z, err, limit)
    print("(n, L, M) = (%d, %d, %d): max|block - dense| = %.2e" % (n, L, M, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("n, L, M", SMALL)
def test_model_against_mpmath(n, L, M):
    H00, H01, V, results, bounds = _case(n, L, M)
    worst = 0.0
    for z, r, tol in zip(Z, results, bounds):
        T, G, F, C, ldos, left, right = dm.device_mp(H00, H01, V, complex(z))
        assert abs(r.T - T) <= tol.T
        for name, got, want, limit, scale in (("G", r.G, G, tol.G, tol.sG), ("F", r.F, F, tol.F, tol.sF), ("C", r.C, C, tol.C, tol.sC),
                                              ("ldos", r.ldos, ldos, tol.ldos, tol.sG), ("left", r.left, left, tol.left, tol.sL),
                                              ("right", r.right, right, tol.right, tol.sR)):
            err = _layer_max(got - want)
            assert np.all(err <= limit), (name, z, err, limit)
            worst = max(worst, (err / scale).max())
    print("(n, L, M) = (%d, %d, %d): largest |model - mpmath| / scale = %.2e (u = %.2e)" % (n, L, M, worst, U))


@pytest.mark.parametrize("n, L, M", CASES)
def test_property_1_the_rest_is_eta_times_the_squared_rows(n, L, M):
    H00, H01, V, results, bounds = _case(n, L, M)
    for z, r, tol in zip(Z, results, bounds):
        rows = dm.device_dense(H00, H01, V, complex(z))[3]
        want = z.imag / np.pi * (np.abs(rows) ** 2).sum(axis=2)
        rest = r.ldos - r.left - r.right
        own = 2 * _dense_own(H00, H01, V, z) * np.abs(rows).sum(axis=2) * abs(z.imag) / np.pi
        limit = (tol.ldos + tol.left + tol.right)[:, None] + own
        assert np.all(np.abs(rest - want) <= limit), (z, np.abs(rest - want).max(), limit.min())
        assert np.all(rest * np.sign(z.imag) > 0.0), "the sign of Im z"


@pytest.mark.parametrize("n, L, M", [(3, 1, 4), (4, 2, 3), (6, 1, 5)])
def test_property_2_a_pristine_device_is_the_bulk(n, L, M):
    H00, H01, V = _case(n, L, M)[:3]
    worst = 0.0
    for z in Z:
        r = dm.device_green(H00, H01, np.zeros_like(V), complex(z))
        tol = dm.tolerance(H00, H01, np.zeros_like(V), complex(z), r)
        _, _, bulk, its, rho = sm.decimate(H00, H01, complex(z))
        limit = tol.G + sm.tolerance(H00[None], H01[None], z, its, rho)[0, 0]
        err = _layer_max(r.G - bulk[None])
        worst = max(worst, err.max())
        assert np.all(err <= limit), (z, err, limit)
    print("(n, L, M) = (%d, %d, %d), V = 0: max|G_p - bulk| = %.2e" % (n, L, M, worst))


@pytest.mark.parametrize("n, L, M", CASES)
def test_property_3_the_forward_sweep_has_the_bits_of_the_transmission(n, L, M):
    H00, H01, V, results, _ = _case(n, L, M)
    for z, r in zip(Z, results):
        T, P, its, rho = tm.transmission(H00, H01, V, complex(z))
        assert r.T == T and np.array_equal(r.F[M - 1], P) and r.iterations == its and r.rho == rho


def test_chain_with_an_impurity_against_the_closed_form():
    t_hop, t_plane = 1.0, 0.3
    full = {(0, 1): np.array([[t_hop]]), (0, -1): np.array([[t_hop]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    worst = 0.0
    for kpar in (0.0, 0.17, 0.5):
        H00, H01 = sm.principal(sm.layers_direct(full, 1, [kpar], 1))
        for eta in (0.05, 0.5):
            for energy in (-3.1, -1.2, 0.4, 1.9, 2.8):
                for eps in (0.0, 0.7, -2.5):
                    z = energy + 1j * eta
                    V = np.full((1, 1, 1), eps, dtype=np.complex128)
                    r = dm.device_green(H00, H01, V, z)
                    want = dm.chain_closed_form(z, t_hop, t_plane, kpar, eps)
                    # the closed form's own rounding: g_s as in test_surface_model.py, carried through 1 / (zeta - eps - 2 t^2 g_s)
                    _, g_b = sm.chain_closed_form(z, t_hop, t_plane, kpar)
                    zeta = z - 2 * t_plane * np.cos(2 * np.pi * kpar)
                    d_g = 64 * U * (abs(zeta) ** 2 + 4 * t_hop ** 2) / abs(1 / g_b) / (2 * t_hop ** 2)
                    own = d_g * 2 * t_hop ** 2 * abs(want) ** 2 + 16 * U * abs(want)
                    bound = dm.tolerance(H00, H01, V, z, r).G[0] + own
                    assert abs(r.G[0, 0, 0] - want) <= bound < 1e-9, (kpar, z, eps)
                    assert abs(r.ldos[0, 0] + want.imag / np.pi) <= bound
                    worst = max(worst, abs(r.G[0, 0, 0] - want))
    print("chain with an impurity: max|G - closed form| = %.2e" % worst)


def test_argument_errors():
    H00, H01, V = _case(3, 1, 4)[:3]
    with pytest.raises(ValueError, match="H01"):
        dm.device_green(H00, None, V, 0.3 + 0.1j)
    for bad in (V[0], V[:, :2, :2], np.zeros((0, 3, 3))):
        with pytest.raises(ValueError, match="V must have shape"):
            dm.device_green(H00, H01, bad, 0.3 + 0.1j)
    with pytest.raises(np.linalg.LinAlgError, match="no convergence"):
        dm.device_green(H00, H01, V, complex(Z[0]), max_iterations=2)
    with pytest.raises(np.linalg.LinAlgError, match="Singular"):
        dm.device_green(np.diag([0.25, 0.5 + 0j]), np.zeros((2, 2)), np.diag([0.25 + 0.125j, 0.0])[None], 0.5 + 0.125j)


def test_signature_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_device_green_from_matrices": 20, "tbk_device_green": 18, "tbk_device_green_multi": 19, "tbk_device_green_timing": 4}
    for name, count in counts.items():
        found = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert found, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        declared = [" ".join(part.split()) for part in found.group(1).split(",")]
        assert len(declared) == len(argtypes) == count, (name, declared)
        for text, ctype in zip(declared, argtypes):
            if "*" in text:
                assert ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer), (name, text)  # pylint: disable=protected-access
            else:
                assert ctype is kinds[text.split()[0]], (name, text)


def test_bounds_of_the_gpu_cases_stay_under_the_ceiling():
    """every bound tests/test_gpu_device_green.py holds the kernel to twice of, for the cases up to 33 rows (the two 64-row cases take
    the model a few seconds each and assert the same there)"""
    for n, L, M in dm.GPU_CASES:
        if n * L > 33:
            continue
        H00, H01, V = dm.gpu_case(n, L, M)
        _, bounds = dm.device_green_function(H00, H01, V, dm.GPU_Z)
        worst = max(float(np.max(getattr(t, name))) for row in bounds for t in row for name in ("T", "G", "F", "C", "ldos", "left", "right"))
        print("(n, L, M) = (%d, %d, %d): largest bound %.2e" % (n, L, M, worst))
        assert worst <= 1e-4


def test_stored_mpmath_reference_of_the_gpu_cases():
    """tests/golden/device_mp.npz (`python tools/device_model.py --golden`) is what device_mp gives: two small cases in full."""
    with np.load(os.path.join(ROOT, "tests", "golden", "device_mp.npz")) as stored:
        assert np.array_equal(stored["Z"], dm.GPU_Z) and np.array_equal(dm.GPU_Z, Z)
        small = [c for c in dm.GPU_CASES if c[0] * c[1] <= 17]
        assert sorted(k for k in stored.files if k != "Z") == sorted("%s_%d_%d_%d" % ((name,) + c) for c in small for name in ("T", "ldos", "left", "right"))
        for n, L, M in ((1, 1, 1), (3, 1, 2)):
            H00, H01, V = dm.gpu_case(n, L, M)
            tag = "_%d_%d_%d" % (n, L, M)
            assert stored["ldos" + tag].shape == (dm.GPU_NK, len(Z), M, n * L)
            for k in range(dm.GPU_NK):
                for i, z in enumerate(Z):
                    T, _, _, _, ldos, left, right = dm.device_mp(H00[k], H01[k], V, complex(z))
                    assert stored["T" + tag][k, i] == T
                    assert np.array_equal(stored["ldos" + tag][k, i], ldos) and np.array_equal(stored["left" + tag][k, i], left)
                    assert np.array_equal(stored["right" + tag][k, i], right)
