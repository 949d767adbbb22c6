"""
tools/surface_model.py, the NumPy statement of the surface Green's function, on the CPU: against the same
iteration in mpmath at 60 digits, the closed form of the chain, a finite slab, the fixed points of the decimation, the discrete
Fourier extraction of the principal layers, the conjugation symmetry, L = 0, the stopping rule, and the C signatures.

Bounds (u = 2^-53), none measured on the code under test: surface_model.tolerance,

    8 N u rho (|z| + |H00|_2 + 2 |H01|_2) / eta^2 (iterations + 1)

with rho the growth factor of the model's eliminations.  With |Im z| >= 0.05 and spectra in [-2, 2] it stays below 1e-8, which is
asserted.  Every case prints its measured maximum.
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

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j, 2.6 + 0.5j, 0.4 - 0.05j, 0.5j])  # test_gpu_dyson.py's
U = 2.0 ** -53
_CACHE = {}


def _case(n, L, n_k=2):
    key = (n, L, n_k)
    if key not in _CACHE:
        layers, H00, H01 = sm.random_case(n, L, n_k, 4100 + 37 * n + L)
        bottom, top, bulk, its, rho = sm.surface_green_function(H00, H01, Z)
        bound = sm.tolerance(H00, H01, Z, its, rho)
        for array in (layers, H00, H01, bottom, top, bulk, its, bound):
            if array is not None:
                array.setflags(write=False)
        _CACHE[key] = (layers, H00, H01, bottom, top, bulk, its, rho, bound)
    return _CACHE[key]


@pytest.mark.parametrize("n, L, energies", [(3, 2, (0, 1, 2, 3, 4)), (1, 1, (0, 1, 4)), (8, 2, (0, 3)), (6, 4, (0,))])
def test_model_against_mpmath(n, L, energies):
    _, H00, H01, bottom, top, bulk, its, _, bound = _case(n, L)
    for i in energies:
        ref = sm.decimate_mp(H00[0], H01[0], complex(Z[i]))
        err = max(np.abs(got[0, i] - want).max() for got, want in zip((bottom, top, bulk), ref))
        print("N = %d z = %s: %d iterations, max|model - mpmath| = %.2e (bound %.2e)" % (n * L, Z[i], its[0, i], err, bound[0, i]))
        assert bound[0, i] < 1e-8
        assert err <= bound[0, i]
        assert 1 <= its[0, i] <= 17


@pytest.mark.parametrize("n, L", [(3, 2), (8, 2)])
def test_model_against_mpmath_close_to_the_axis(n, L):
    """eta = 1e-3: the bound is no longer small, and still dominates (the last two rows)."""
    _, H00, H01 = _case(n, L)[:3]
    z = 0.3 + 1e-3j
    got = sm.decimate(H00[0], H01[0], z)
    bound = sm.tolerance(H00[:1], H01[:1], z, got[3], got[4])[0, 0]
    err = max(np.abs(a - b).max() for a, b in zip(got[:3], sm.decimate_mp(H00[0], H01[0], z)))
    print("N = %d z = %s: %d iterations, max|model - mpmath| = %.2e (bound %.2e)" % (n * L, z, got[3], err, bound))
    assert err <= bound and 12 <= got[3] <= 31


def test_the_stopping_rule_changes_no_bit():
    """Running alpha and beta down to exact zero gives the bits of the rule."""
    for n, L in ((1, 1), (3, 2), (8, 2)):
        _, H00, H01, bottom, top, bulk, its, _, _ = _case(n, L)
        for k in range(H00.shape[0]):
            for i, z in enumerate(Z):
                b, t, m, longer, _ = sm.decimate(H00[k], H01[k], complex(z), to_zero=True, max_iterations=400)
                assert longer >= its[k, i]
                assert np.array_equal(b, bottom[k, i]) and np.array_equal(t, top[k, i]) and np.array_equal(m, bulk[k, i]), (n, L, k, i)


def test_chain_closed_form():
    t_hop, t_plane = 1.0, 0.3
    full = {(0, 1): np.array([[t_hop]]), (0, -1): np.array([[t_hop]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    assert sm.layer_count(full, 1) == 1
    for kpar in (0.0, 0.17, 0.5):
        H00, H01 = sm.principal(sm.layers_direct(full, 1, [kpar], 1))
        for z in list(Z) + [1.9 + 0.05j, -2.3 - 0.05j]:
            bottom, top, bulk, its, rho = sm.decimate(H00, H01, complex(z))
            gs, gb = sm.chain_closed_form(complex(z), t_hop, t_plane, kpar)
            zeta = z - 2 * t_plane * np.cos(2 * np.pi * kpar)
            # the closed form's own rounding: the root of a difference, then a difference
            own = 64 * U * (abs(zeta) ** 2 + 4 * t_hop ** 2) / abs(1 / gb) / (2 * t_hop ** 2)
            bound = sm.tolerance(H00[None], H01[None], z, its, rho)[0, 0] + own
            err = max(abs(bottom[0, 0] - gs), abs(top[0, 0] - gs), abs(bulk[0, 0] - gb))
            print("chain k = %.2f z = %s: %d iterations, max|G - closed form| = %.2e (bound %.2e)" % (kpar, z, its, err, bound))
            assert bound < 1e-8 and err <= bound
            assert gs.imag * z.imag < 0


def _slab(H00, H01, z, count):
    N = H00.shape[0]
    H = np.zeros((count * N, count * N), dtype=np.complex128)
    for p in range(count):
        H[p * N:(p + 1) * N, p * N:(p + 1) * N] = H00
        if p + 1 < count:
            H[p * N:(p + 1) * N, (p + 1) * N:(p + 2) * N] = H01
            H[(p + 1) * N:(p + 2) * N, p * N:(p + 1) * N] = H01.conj().T
    return np.linalg.inv(z * np.eye(count * N) - H)


@pytest.mark.parametrize("n, L", [(1, 1), (3, 2)])
def test_finite_slab(n, L):
    _, H00, H01, bottom, top, _, _, _, bound = _case(n, L)
    N = n * L
    for i in (1, 2, 4):  # |Im z| = 0.5
        G60, G120 = _slab(H00[0], H01[0], Z[i], 60), _slab(H00[0], H01[0], Z[i], 120)
        # the reference's own error.  Its finite size: the error falls geometrically with the length, so the slab of 120 layers is
        # no farther from the limit than from the slab of 60, and the slab of 60 at most twice their distance.  numpy's inversion:
        # |A^-1| <= 1 / eta, kappa <= (|z| + 2) / eta
        own = 2 * max(np.abs(G60[:N, :N] - G120[:N, :N]).max(), np.abs(G60[-N:, -N:] - G120[-N:, -N:]).max())
        own += 8 * 120 * N * U * (abs(Z[i]) + 2) / 0.25
        err_b = np.abs(bottom[0, i] - G60[:N, :N]).max()
        err_t = np.abs(top[0, i] - G60[-N:, -N:]).max()
        print("slab of 60 layers N = %d z = %s: max|bottom - corner| = %.2e, max|top - corner| = %.2e (bound %.2e)"
              % (N, Z[i], err_b, err_t, bound[0, i] + own))
        assert max(err_b, err_t) <= bound[0, i] + own < 1e-8


@pytest.mark.parametrize("n, L", [(1, 1), (3, 2), (8, 2)])
def test_fixed_points(n, L):
    _, H00, H01, bottom, top, bulk, _, _, bound = _case(n, L)
    N = n * L
    for k in range(H00.shape[0]):
        b = np.linalg.norm(H01[k], 2)
        for i, z in enumerate(Z):
            one = z * np.eye(N)
            sig_b = H01[k] @ bottom[k, i] @ H01[k].conj().T
            sig_t = H01[k].conj().T @ top[k, i] @ H01[k]
            res_b = np.abs(bottom[k, i] - np.linalg.inv(one - H00[k] - sig_b)).max()
            res_t = np.abs(top[k, i] - np.linalg.inv(one - H00[k] - sig_t)).max()
            res_m = np.abs(bulk[k, i] - np.linalg.inv(one - H00[k] - sig_b - sig_t)).max()
            # F(G) = (z - H00 - H01 G H01^H)^-1 has |F'| <= |H01|^2 / eta^2 at a causal G: an error d of G leaves a residual of at most
            # (1 + |H01|^2 / eta^2) d, and the evaluation of F adds one more inversion's error (two self-energies for the bulk)
            limit = (3 + 2 * b * b / Z[i].imag ** 2) * bound[k, i]
            print("N = %d k %d z = %s: fixed-point residuals %.2e %.2e %.2e (bound %.2e)" % (N, k, z, res_b, res_t, res_m, limit))
            assert max(res_b, res_t, res_m) <= limit


def test_layers_from_samples_match_the_direct_sum():
    rng = np.random.default_rng(12)
    n, dim = 3, 3
    r_vec = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 2], [1, -1, 1], [0, 0, 2], [1, 1, -2]])
    hop = rng.normal(size=(len(r_vec), n, n)) + 1j * rng.normal(size=(len(r_vec), n, n))
    hop[0] = (hop[0] + hop[0].conj().T) / 4
    full = sm.full_hoppings(r_vec, hop)
    total = sum(np.abs(m).max() for m in full.values())
    for axis, L in ((2, 2), (0, 1), (1, 1)):
        assert sm.layer_count(full, axis) == L
        for kpar in ([0.0, 0.0], [0.13, -0.41]):
            direct = sm.layers_direct(full, axis, kpar, L)
            pts = sm.sample_points(kpar, axis, L, dim)
            samples = np.array([sum(np.exp(2j * np.pi * np.dot(p, R)) * m for R, m in full.items()) for p in pts])
            got = sm.layers_from_samples(samples)
            err = np.abs(got - direct).max()
            bound = 8 * (2 * L + 3) * U * total * len(full)
            print("axis %d L = %d k = %s: max|H_m (Fourier) - H_m (direct)| = %.2e (bound %.2e)" % (axis, L, kpar, err, bound))
            assert err <= bound
            assert np.abs(direct[::-1] - np.conj(np.transpose(direct, (0, 2, 1)))).max() <= 4 * U * total  # H_{-m} = H_m^H
            # a longer principal layer than needed: the extra H_m vanish
            more = sm.layers_direct(full, axis, kpar, L + 1)
            assert np.all(more[0] == 0) and np.all(more[-1] == 0) and np.array_equal(more[1:-1], direct)


def test_principal_layers_block_order():
    layers = np.arange(5, dtype=float)[:, None, None] * np.ones((5, 2, 2)) + 0j  # H_m = (m + 2) everywhere, L = 2
    H00, H01 = sm.principal(layers)
    assert H00.shape == (4, 4)
    assert H00[0, 0] == 2 and H00[0, 2] == 3 and H00[2, 0] == 1          # H_0 on the diagonal, H_{+1} above, H_{-1} below
    assert H01[0, 0] == 4 and H01[2, 0] == 3 and H01[2, 2] == 4 and H01[0, 2] == 0   # H_2, H_1; nothing above the diagonal
    assert sm.principal(layers[2:3])[1] is None


@pytest.mark.parametrize("n, L", [(1, 1), (3, 2)])
def test_conjugate_energy_gives_the_adjoint(n, L):
    _, H00, H01, bottom, top, bulk, _, _, bound = _case(n, L)
    for i, z in enumerate(Z):
        b, t, m, its, rho = sm.decimate(H00[1], H01[1], complex(np.conj(z)))
        limit = bound[1, i] + sm.tolerance(H00[1:2], H01[1:2], np.conj(z), its, rho)[0, 0]
        err = max(np.abs(x - y[1, i].conj().T).max() for x, y in ((b, bottom), (t, top), (m, bulk)))
        print("N = %d z = %s: max|G(conj z) - G(z)^H| = %.2e (bound %.2e)" % (n * L, z, err, limit))
        assert err <= limit


def test_no_hopping_between_layers():
    layers, H00, H01 = sm.random_case(4, 0, 2, 5)
    assert H01 is None and H00.shape == (2, 4, 4) and layers.shape == (2, 1, 4, 4)
    bottom, top, bulk, its, rho = sm.surface_green_function(H00, None, Z)
    bound = sm.tolerance(H00, None, Z, its, rho)
    assert np.all(its == 0)
    assert np.array_equal(bottom, top) and np.array_equal(bottom, bulk)
    for i, z in enumerate(Z):
        err = np.abs(bottom[:, i] - np.linalg.inv(z * np.eye(4) - H00)).max()
        assert err <= bound[:, i].min() < 1e-8


def test_the_cap_and_singular_input_raise():
    _, H00, H01, _, _, _, its, _, _ = _case(3, 2)
    assert its[0, 0] > 2
    with pytest.raises(np.linalg.LinAlgError, match="no convergence"):
        sm.decimate(H00[0], H01[0], complex(Z[0]), max_iterations=2)
    with pytest.raises(np.linalg.LinAlgError, match="Singular"):
        sm.decimate(np.diag([0.3, 0.3 + 0.2j]), None, 0.3 + 0.2j)


def test_signature_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_surface_from_matrices": 14, "tbk_surface_green": 13, "tbk_surface_green_multi": 14, "tbk_surface_timing": 4}
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
