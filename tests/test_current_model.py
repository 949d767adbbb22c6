"""
tools/current_model.py, the NumPy statement of the bond currents of the device, on the CPU: K, J and the row sums
against an independent route through the dense block-tridiagonal inverse and against the same lines in mpmath at 60 digits, the
properties 1 - 4 of the model's docstring as identities, the limit eta -> 0 on a chain, the argument errors, the C signatures, the
bounds of the GPU cases and the stored mpmath reference.

Bounds (u = 2^-53), none measured on the code under test: current_model.tolerance, per component

    K^L_p: 2 max|H01| (c(F_p) + c(F_{p+1}) + 1) E s(F_p) s(F_{p+1}) gamma_L      J^L_p: 2 max|H_pp| (2 c(F_p) + 1) E s(F_p)^2 gamma_L

with E, c, s, gamma of device_model.tolerance; K^R, J^R with C and gamma_R; current_* N times K's.  The identities hold on exact
quantities; on the model's they are held to the sum of the bounds of the terms that enter them.  Every case prints its measured maximum.
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
import current_model as cm  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])  # tests/test_gpu_surface.py's
U = 2.0 ** -53
CASES = [(1, 1, 1), (3, 1, 4), (4, 2, 3), (6, 1, 5)]
SMALL = [(1, 1, 1), (3, 1, 4), (4, 2, 3)]  # mpmath on these
_CACHE = {}


def _case(n, L, M):
    """One in-plane point: layers, a random Hermitian device of norm 0.5, the model's run at the five energies and its bounds."""
    key = (n, L, M)
    if key not in _CACHE:
        _, H00, H01 = tm.random_case(n, L, 1, 6100 + 37 * n + L)
        V = tm.random_device(n * L, M, 6200 + 37 * n + M)
        results, bounds = cm.device_current_function(H00, H01, V, Z)
        for array in (H00, H01, V):
            array.setflags(write=False)
        _CACHE[key] = (H00[0], H01[0], V, results[0], bounds[0])
    return _CACHE[key]


def _layer_max(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def _dense_own(H00, H01, V, z, tol, name):
    """the dense route's own error: numpy's inversion of the (M N) x (M N) matrix errs by 8 M N u kappa relative to |A^-1| <= 1 / eta
    in each of the two blocks of a bond current, so by that fraction of the bond's scale over the scales of its blocks, 1 / eta each"""
    size = np.linalg.norm(H00, 2) + 2 * np.linalg.norm(H01, 2) + max(np.linalg.norm(v, 2) for v in V)
    rel = 8 * V.shape[0] * H00.shape[0] * U * (abs(z) + size) / abs(z.imag)
    N = H00.shape[0]
    hop = float(np.abs(H01).max()) if name.startswith(("inter", "current")) else max(float(np.abs(H00 + v).max()) for v in V)
    gamma = 2 * np.linalg.norm(H01, 2) ** 2 / abs(z.imag)
    return 3 * rel * 2 * hop * gamma / z.imag ** 2 * (N if name.startswith("current") else 1)


@pytest.mark.parametrize("n, L, M", CASES)
def test_currents_against_the_dense_inverse(n, L, M):
    H00, H01, V, results, bounds = _case(n, L, M)
    worst = 0.0
    for z, r, tol in zip(Z, results, bounds):
        dense = cm.current_dense(H00, H01, V, complex(z))
        for index, name in enumerate(cm.NAMES):
            got = getattr(r, name)
            assert got.shape == dense[index].shape == ((M - (name[:5] != "intra"), n * L) + (() if name.startswith("current") else (n * L,)))
            if got.size:
                err = _layer_max(got - dense[index])
                worst = max(worst, err.max())
                assert np.all(err <= getattr(tol, name) + _dense_own(H00, H01, V, z, tol, name)), (name, z, err)
    print("(n, L, M) = (%d, %d, %d): max|model - dense| = %.2e" % (n, L, M, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("n, L, M", SMALL)
def test_model_against_mpmath(n, L, M):
    pytest.importorskip("mpmath")
    H00, H01, V, results, bounds = _case(n, L, M)
    worst = 0.0
    for z, r, tol in zip(Z, results, bounds):
        ref = cm.current_mp(H00, H01, V, complex(z))
        for index, name in enumerate(cm.NAMES):
            got = getattr(r, name)
            assert got.shape == ref[index].shape
            if got.size:
                err = _layer_max(got - ref[index])
                assert np.all(err <= getattr(tol, name)), (name, z, err)
                worst = max(worst, (err / getattr(tol, "s_" + name)).max())
    print("(n, L, M) = (%d, %d, %d): largest |model - mpmath| / scale = %.2e (u = %.2e)" % (n, L, M, worst, U))
    assert worst <= 64 * U


@pytest.mark.parametrize("n, L, M", CASES + [(5, 1, 6), (8, 2, 3)])
def test_properties_1_to_4_as_identities(n, L, M):
    H00, H01, V, results, bounds = _case(n, L, M)
    N = n * L
    worst = 0.0
    for z, r, tol in zip(Z, results, bounds):
        residual = cm.identities(H00, H01, V, complex(z), r, cm.t_prime(r.green.C[0], r.green.es, r.green.et))
        limit = cm.identity_bounds(complex(z), tol, N)
        assert residual["left"].shape == (M - 1,) and residual["right"].shape == (M - 1,) and residual["orbital_left"].shape == (max(M - 2, 0), N)
        for name, value in residual.items():
            assert value.shape == limit[name].shape, name
            if value.size:
                worst = max(worst, float(np.abs(value).max()))
                assert np.all(np.abs(value) <= limit[name]), (name, z, value, limit[name])
        for K, J, bound in ((r.inter_left, r.intra_left, tol.intra_left), (r.inter_right, r.intra_right, tol.intra_right)):
            assert np.all(K[:, H01 == 0] == 0.0)
            for p in range(M):
                assert np.all(J[p][(H00 + V[p]) == 0] == 0.0)
            assert np.all(_layer_max(J + np.transpose(J, (0, 2, 1))) <= 2 * bound)
        if M > 1:  # K^L flows to the right lead, K^R to the left
            assert np.all(r.current_left.sum(axis=1) > 0.0) and np.all(r.current_right.sum(axis=1) < 0.0)
    print("(n, L, M) = (%d, %d, %d): largest residual of the identities %.2e" % (n, L, M, worst))
    assert worst < 1e-13  # (the issue's own run: 7e-16)


def test_zero_pattern_of_a_sparse_device():
    rng = np.random.default_rng(11)
    N, M = 6, 3
    a = (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) * (rng.random((N, N)) < 0.4)
    H00 = (a + a.conj().T) * 0.2
    H01 = (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) * (rng.random((N, N)) < 0.4) * 0.3
    V = np.zeros((M, N, N), dtype=np.complex128)
    V[:, np.arange(N), np.arange(N)] = rng.normal(size=(M, N)) * 0.3
    assert np.count_nonzero(H01 == 0) > 6 and np.count_nonzero(H00 == 0) > 6
    r = cm.device_current(H00, H01, V, 0.2 + 0.05j)
    for K, J in ((r.inter_left, r.intra_left), (r.inter_right, r.intra_right)):
        assert np.all(K[:, H01 == 0] == 0.0) and np.any(K != 0.0)
        for p in range(M):
            assert np.all(J[p][(H00 + V[p]) == 0] == 0.0)


def test_every_interface_carries_T_as_eta_shrinks():
    """the chain with impurities: sum K^L_p - T = 4 pi eta sum_{q > p} left[q] -> 0, linearly in eta; the right lead's mirror it"""
    t_hop, t_plane = 1.0, 0.3
    full = {(0, 1): np.array([[t_hop]]), (0, -1): np.array([[t_hop]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    H00, H01 = sm.principal(sm.layers_direct(full, 1, [0.17], 1))
    V = np.array([0.0, 0.8, -0.4, 0.0, 0.3]).reshape(5, 1, 1).astype(np.complex128)
    previous = None
    for eta in (1e-2, 1e-3, 1e-4, 1e-5):
        r = cm.device_current(H00, H01, V, 0.4 + 1j * eta, max_iterations=200)
        gap_l = np.abs(r.current_left.sum(axis=1) - r.T).max()
        gap_r = np.abs(-r.current_right.sum(axis=1) - r.T).max()
        print("eta = %.0e: T = %.9f, max|sum K^L_p - T| = %.2e, max|-sum K^R_p - T| = %.2e" % (eta, r.T, gap_l, gap_r))
        assert 0.1 < r.T < 1.0
        assert gap_l <= 4 * np.pi * eta * np.abs(r.left).sum() + 1e-12 and gap_l < 40 * eta and gap_r < 40 * eta
        if previous is not None:
            assert gap_l < 0.2 * previous
        previous = gap_l


def test_argument_errors():
    H00, H01, V = _case(3, 1, 4)[:3]
    with pytest.raises(ValueError, match="H01"):
        cm.device_current(H00, None, V, 0.3 + 0.1j)
    for bad in (V[0], V[:, :2, :2], np.zeros((0, 3, 3))):
        with pytest.raises(ValueError, match="V must have shape"):
            cm.device_current(H00, H01, bad, 0.3 + 0.1j)
    with pytest.raises(np.linalg.LinAlgError, match="no convergence"):
        cm.device_current(H00, H01, V, complex(Z[0]), max_iterations=2)
    with pytest.raises(np.linalg.LinAlgError, match="Singular"):
        cm.device_current(np.diag([0.25, 0.5 + 0j]), np.zeros((2, 2)), np.diag([0.25 + 0.125j, 0.0])[None], 0.5 + 0.125j)
    single = cm.device_current(H00, H01, V[:1], 0.3 + 0.1j)
    assert single.current_left.shape == (0, 3) and single.inter_right.shape == (0, 3, 3) and single.intra_left.shape == (1, 3, 3)


def test_signature_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_device_current_from_matrices": 23, "tbk_device_current": 21, "tbk_device_current_multi": 22, "tbk_device_current_timing": 4}
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
    # the green family's arguments with G, F, C replaced by the six current arrays
    for name in ("_from_matrices", "", "_multi"):
        green, current = _lib.SIGNATURES["tbk_device_green" + name][1], _lib.SIGNATURES["tbk_device_current" + name][1]
        assert current[:len(green) - 3] == green[:-3] and len(current) == len(green) + 3


def test_bounds_of_the_gpu_cases_stay_under_the_ceiling():
    """every bound tests/test_gpu_device_current.py holds the kernel to twice of, for the cases up to 33 rows (the 64-row cases take
    the model a few seconds each and assert the same there)"""
    for n, L, M in cm.GPU_CASES:
        if n * L > 33:
            continue
        H00, H01, V = cm.gpu_case(n, L, M)
        _, bounds = cm.device_current_function(H00, H01, V, cm.GPU_Z)
        worst = max([float(np.max(getattr(t.device, name))) for row in bounds for t in row for name in ("T", "ldos", "left", "right")]
                    + [float(np.max(getattr(t, name))) for row in bounds for t in row for name in cm.NAMES if getattr(t, name).size])
        print("(n, L, M) = (%d, %d, %d): largest bound %.2e" % (n, L, M, worst))
        assert worst <= 1e-4


def test_stored_mpmath_reference_of_the_gpu_cases():
    """tests/golden/current_mp.npz (`python tools/current_model.py --golden`) is what current_mp gives: two small cases in full."""
    pytest.importorskip("mpmath")
    with np.load(os.path.join(ROOT, "tests", "golden", "current_mp.npz")) as stored:
        assert np.array_equal(stored["Z"], cm.GPU_Z) and np.array_equal(cm.GPU_Z, Z)
        small = [c for c in cm.GPU_CASES if c[0] * c[1] <= 17]
        assert sorted(k for k in stored.files if k != "Z") == sorted("%s_%d_%d_%d" % ((name,) + c) for c in small for name in cm.NAMES)
        for n, L, M in ((1, 1, 3), (3, 1, 2)):
            H00, H01, V = cm.gpu_case(n, L, M)
            tag = "_%d_%d_%d" % (n, L, M)
            assert stored["current_left" + tag].shape == (cm.GPU_NK, len(Z), M - 1, n * L)
            assert stored["intra_right" + tag].shape == (cm.GPU_NK, len(Z), M, n * L, n * L)
            for k in range(cm.GPU_NK):
                for i, z in enumerate(Z):
                    ref = cm.current_mp(H00[k], H01[k], V, complex(z))
                    for index, name in enumerate(cm.NAMES):
                        assert np.array_equal(stored[name + tag][k, i], ref[index]), name
