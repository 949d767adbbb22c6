"""
tools/transport_model.py, the NumPy statement of the Landauer transmission, on the CPU: the sweep against the
dense block-tridiagonal inverse, against the same sweep in mpmath at 60 digits, the chain with one impurity against its closed form
at finite eta, the channel count of pristine crystals, P_M against the dense inverse's block, a growing barrier, the argument errors
and the C signatures.

Bounds (u = 2^-53), none measured on the code under test: transport_model.tolerance = 4 eps scale with

    eps   = 8 N u rho (|z| + |H00|_2 + 2 |H01|_2 + max |V_p|_2) / eta (iterations + M + 1)
    scale = N (2 |H01|_2^2 |G_bottom|_2) (2 |H01|_2^2 |G_top|_2) |P_M|_2^2

Every case prints its measured maximum.
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
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])  # tests/test_gpu_surface.py's
U = 2.0 ** -53
CASES = [(1, 1, 1), (3, 1, 4), (4, 2, 3), (6, 1, 1)]
_CACHE = {}


def _case(n, L, M):
    """One in-plane point: layers, a random Hermitian device of norm 0.5 and the model's run at the five energies; never written."""
    key = (n, L, M)
    if key not in _CACHE:
        _, H00, H01 = tm.random_case(n, L, 1, 5100 + 37 * n + L)
        V = tm.random_device(n * L, M, 5200 + 37 * n + M)
        T, P, its, rho = tm.transmission_function(H00, H01, V, Z)
        bound = np.array([tm.tolerance(H00[0], H01[0], V, complex(z), its[0, i], rho[0, i], P[0, i]) for i, z in enumerate(Z)])
        size = np.array([tm.scale(H00[0], H01[0], complex(z), P[0, i]) for i, z in enumerate(Z)])
        for array in (H00, H01, V, T, P, its, rho, bound, size):
            array.setflags(write=False)
        _CACHE[key] = (H00[0], H01[0], V, T[0], P[0], its[0], rho[0], bound, size)
    return _CACHE[key]


def _dense_own(H00, H01, V, z):
    """numpy's inversion of the (M N) x (M N) matrix, per component: |A^-1| <= 1 / eta, kappa <= (|z| + |H|) / eta"""
    size = np.linalg.norm(H00, 2) + 2 * np.linalg.norm(H01, 2) + max(np.linalg.norm(v, 2) for v in V)
    return 8 * V.shape[0] * H00.shape[0] * U * (abs(z) + size) / z.imag ** 2


@pytest.mark.parametrize("n, L, M", CASES)
def test_sweep_against_the_dense_inverse(n, L, M):
    H00, H01, V, T, P, _, rho, bound, _ = _case(n, L, M)
    for i, z in enumerate(Z):
        T_dense, P_dense, G = tm.transmission_dense(H00, H01, V, complex(z))
        print("N = %d M = %d z = %s: T = %.12f, |T - dense| = %.2e (bound %.2e)" % (n * L, M, z, T[i], abs(T[i] - T_dense), bound[i]))
        assert abs(T[i] - T_dense) <= bound[i]
        # P_M is block (M, 1) of the dense inverse
        limit = tm.green_tolerance(H00, H01, V, complex(z), _case(n, L, M)[5][i], rho[i]) + _dense_own(H00, H01, V, z)
        err = np.abs(P[i] - P_dense).max()
        print("    max|P_M - G[M, 1]| = %.2e (bound %.2e)" % (err, limit))
        assert err <= limit
        assert G.shape == (M * n * L, M * n * L) and np.array_equal(P_dense, G[-n * L:, :n * L])


@pytest.mark.parametrize("n, L, M", CASES)
def test_model_against_mpmath(n, L, M):
    H00, H01, V, T, P, its, _, bound, size = _case(n, L, M)
    worst = 0.0
    for i, z in enumerate(Z):
        T_mp, P_mp = tm.transmission_mp(H00, H01, V, complex(z))
        assert abs(T[i] - T_mp) <= bound[i], (i, T[i], T_mp, bound[i])
        assert np.abs(P[i] - P_mp).max() <= tm.green_tolerance(H00, H01, V, complex(z), its[i], _case(n, L, M)[6][i])
        worst = max(worst, abs(T[i] - T_mp) / size[i])
    print("(n, L, M) = (%d, %d, %d): largest |T - T_mp| / scale = %.2e (u = %.2e); bounds %.2e ... %.2e, T up to %.3f"
          % (n, L, M, worst, U, bound.min(), bound.max(), T.max()))


def test_chain_with_an_impurity_against_the_closed_form():
    """Finite eta only: at eta -> 0 the decimation itself loses 1 / eta^2, which is no property of the sweep."""
    t_hop, t_plane = 1.0, 0.3
    full = {(0, 1): np.array([[t_hop]]), (0, -1): np.array([[t_hop]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    worst = 0.0
    for kpar in (0.0, 0.17, 0.5):
        H00, H01 = sm.principal(sm.layers_direct(full, 1, [kpar], 1))
        for eta in (0.05, 0.5):
            for energy in (-3.1, -1.2, 0.4, 1.9, 2.8):  # the band is 2 t' cos(2 pi k) + [-2, 2]: inside and outside
                for eps in (0.0, 0.7, -2.5):
                    z = energy + 1j * eta
                    V = np.full((1, 1, 1), eps, dtype=np.complex128)
                    T, P, its, rho = tm.transmission(H00, H01, V, z)
                    want = tm.chain_closed_form(z, t_hop, t_plane, kpar, eps)
                    # the closed form's own rounding: g_s as in test_surface_model.py, carried through Gamma^2 |G|^2
                    g_s, g_b = sm.chain_closed_form(z, t_hop, t_plane, kpar)
                    zeta = z - 2 * t_plane * np.cos(2 * np.pi * kpar)
                    d_g = 64 * U * (abs(zeta) ** 2 + 4 * t_hop ** 2) / abs(1 / g_b) / (2 * t_hop ** 2)
                    gamma, G = 2 * t_hop ** 2 * abs(g_s.imag), abs(1.0 / (zeta - eps - 2 * t_hop ** 2 * g_s))
                    own = d_g * 4 * t_hop ** 2 * (gamma * G ** 2 + gamma ** 2 * G ** 3) + 16 * U * want
                    bound = tm.tolerance(H00, H01, V, z, its, rho, P) + own
                    assert abs(T - want) <= bound < 1e-9, (kpar, z, eps, T, want, bound)
                    assert 0.0 <= T <= 1.0 + bound
                    worst = max(worst, abs(T - want))
    print("chain with an impurity: max|T - closed form| = %.2e" % worst)


@pytest.mark.parametrize("n, L, seed, M", [(3, 1, 1, 4), (4, 2, 2, 3), (6, 1, 3, 1)])
def test_pristine_crystal_counts_its_channels(n, L, seed, M):
    layers, H00, H01 = tm.random_case(n, L, 1, seed)
    V = np.zeros((M, n * L, n * L), dtype=np.complex128)
    counts = []
    for energy in (-0.8, 0.1, 0.9):
        T = tm.transmission(H00[0], H01[0], V, energy + 1e-6j)[0]
        want = tm.channels(layers[0], energy)
        print("n = %d L = %d M = %d E = %+.1f: T = %.6f, %d right-moving bands" % (n, L, M, energy, T, want))
        assert abs(T - want) <= 1e-3
        counts.append(want)
    assert max(counts) >= 1
    # the spectrum lies in [-2, 2]: E = 3 is in a gap
    T = tm.transmission(H00[0], H01[0], V, 3.0 + 1e-6j)[0]
    print("    E = +3.0: T = %.2e" % T)
    assert tm.channels(layers[0], 3.0) == 0 and abs(T) < 1e-11


def test_a_growing_barrier_closes_the_chain():
    H00, H01 = np.array([[0.0 + 0j]]), np.array([[1.0 + 0j]])
    z = 0.4 + 0.05j
    for M, heights in ((1, (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 32.0)), (3, (3.0, 4.0, 8.0, 32.0))):  # (M = 3: above the band, no resonances)
        T = [tm.transmission(H00, H01, np.full((M, 1, 1), h, dtype=np.complex128), z)[0] for h in heights]
        print("M = %d, heights %s: T = %s" % (M, heights, ["%.3e" % t for t in T]))
        assert all(a > b > 0.0 for a, b in zip(T, T[1:]))
        assert T[-1] < 1e-2 ** M


def test_conjugate_energy_is_the_exchange_of_the_leads():
    """G(conj z) = G(z)^H, so T at conj(z) is the transmission from the other side: that of the reversed stack (H01 -> H01^H, the
    layers in reverse order) at z.  (At finite eta the two directions differ: eta absorbs inside the device.)"""
    H00, H01, V, _, _, _, _, bound, _ = _case(4, 2, 3)
    for i, z in enumerate(Z):
        back = tm.transmission(H00, H01.conj().T.copy(), V[::-1], complex(z))[0]
        conj = tm.transmission(H00, H01, V, complex(np.conj(z)))[0]
        print("z = %s: |T(conj z) - T(reversed stack)| = %.2e (bound %.2e)" % (z, abs(conj - back), 2 * bound[i]))
        assert abs(conj - back) <= 2 * bound[i]


def test_argument_errors():
    H00, H01, V = _case(3, 1, 4)[:3]
    with pytest.raises(ValueError, match="H01"):
        tm.transmission(H00, None, V, 0.3 + 0.1j)
    for bad in (V[0], V[:, :2, :2], np.zeros((0, 3, 3))):
        with pytest.raises(ValueError, match="V must have shape"):
            tm.transmission(H00, H01, bad, 0.3 + 0.1j)
    with pytest.raises(np.linalg.LinAlgError, match="no convergence"):
        tm.transmission(H00, H01, V, complex(Z[0]), max_iterations=2)
    with pytest.raises(np.linalg.LinAlgError, match="Singular"):  # z - D_1 has a zero: no lead broadening without H01
        tm.transmission(np.diag([0.25, 0.5 + 0j]), np.zeros((2, 2)), np.diag([0.25 + 0.125j, 0.0])[None], 0.5 + 0.125j)
    es, et, its, rho = tm.lead_terms(H00, H01, complex(Z[0]))
    b, t, _, count, _ = sm.decimate(H00, H01, complex(Z[0]))
    assert count == its and rho >= 1.0
    one = Z[0] * np.eye(3)
    assert np.array_equal(b, sm._invert(one - es)[0]) and np.array_equal(t, sm._invert(one - et)[0])  # pylint: disable=protected-access


def test_signature_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_transmission_from_matrices": 14, "tbk_transmission": 13, "tbk_transmission_multi": 14, "tbk_transmission_timing": 4}
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


def test_stored_mpmath_reference_of_the_gpu_cases():
    """tests/golden/transport_mp.npz (`python tools/transport_model.py --golden`) is what transmission_mp gives: the two small cases
    in full, one (k, z) of a 16-row case (mpmath takes two seconds per point there)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "transport_mp.npz")) as stored:
        assert np.array_equal(stored["Z"], tm.GPU_Z) and np.array_equal(tm.GPU_Z, Z)
        assert sorted(k for k in stored.files if k != "Z") == sorted("T_%d_%d_%d" % c for c in tm.GPU_CASES if c[0] * c[1] <= 17)
        for (n, L, M), points in (((1, 1, 1), None), ((3, 1, 2), None), ((8, 2, 3), [(1, 3)])):
            H00, H01, V = tm.gpu_case(n, L, M)
            T_mp = stored["T_%d_%d_%d" % (n, L, M)]
            assert T_mp.shape == (tm.GPU_NK, len(Z))
            for k, i in points or [(k, i) for k in range(tm.GPU_NK) for i in range(len(Z))]:
                assert T_mp[k, i] == tm.transmission_mp(H00[k], H01[k], V, complex(Z[i]))[0], (n, L, M, k, i)
