"""
tools/ensemble_model.py, the NumPy statement of the transmission of an ensemble of devices, on the CPU: the
ensemble against `transport_model.transmission` per sample bit for bit in both forms of the devices, the argument errors of
`Model.transmission_ensemble` (raised before any device work), the four C signatures, and the bounds of the GPU cases.

The bound per sample is transport_model.tolerance (u = 2^-53), not measured on the code under test; the GPU cases of
tests/test_gpu_ensemble.py must keep it at or below 1e-4.
"""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ensemble_model as em  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

Z = tm.GPU_Z


@pytest.mark.parametrize("n, L, M, S", [(1, 1, 1, 3), (3, 1, 2, 4), (4, 2, 3, 3), (6, 1, 4, 2)])
def test_ensemble_has_the_bits_of_the_single_device_model(n, L, M, S):
    _, H00, H01 = tm.random_case(n, L, 1, 5100 + 37 * n + L)
    N = n * L
    onsite = np.random.default_rng(5300 + n).uniform(-0.5, 0.5, (S, M, N))
    matrices = np.stack([tm.random_device(N, M, 5400 + 7 * n + s) for s in range(S)])
    expanded = em.expand(onsite)
    assert expanded.shape == (S, M, N, N) and np.array_equal(expanded[1, 0].diagonal(), onsite[1, 0])
    assert np.count_nonzero(expanded) == np.count_nonzero(onsite)
    for z in Z:
        for devices, dense in ((onsite, expanded), (matrices, matrices), (expanded, expanded)):
            T, P, its, rho = em.transmission_ensemble(H00[0], H01[0], devices, complex(z))
            assert T.shape == (S,) and P.shape == (S, N, N) and rho.shape == (S,)
            for s in range(S):
                want, want_p, want_its, want_rho = tm.transmission(H00[0], H01[0], dense[s], complex(z))
                assert T[s] == want and np.array_equal(P[s], want_p) and its == want_its and rho[s] == want_rho, (n, L, M, s, z)
    # the other samples and their order change nothing
    T, _, _, _ = em.transmission_ensemble(H00[0], H01[0], onsite, complex(Z[0]))
    order = np.arange(S)[::-1]
    assert np.array_equal(em.transmission_ensemble(H00[0], H01[0], onsite[order], complex(Z[0]))[0], T[order])
    assert em.transmission_ensemble(H00[0], H01[0], onsite[-1:], complex(Z[0]))[0][0] == T[-1]


def test_model_argument_errors():
    _, H00, H01 = tm.random_case(3, 1, 1, 11)
    with pytest.raises(ValueError, match="must be real"):
        em.expand(1j * np.ones((2, 2, 3)))
    for bad in (np.zeros((2, 3)), np.zeros((2, 2, 4)), np.zeros((2, 2, 3, 4)), np.zeros((0, 2, 3)), np.zeros((2, 0, 3, 3))):
        with pytest.raises(ValueError, match="devices must have shape"):
            em.transmission_ensemble(H00[0], H01[0], bad, 0.3 + 0.1j)
    with pytest.raises(np.linalg.LinAlgError):
        em.transmission_ensemble(H00[0], H01[0], np.zeros((2, 2, 3)), complex(Z[0]), max_iterations=2)


def test_argument_errors_come_before_any_device_work():
    """Every one of these is raised from the arguments alone: the test runs without a GPU."""
    rng = np.random.default_rng(3)
    hop = {(0, 0, 1): rng.normal(size=(2, 2)) * 0.3, (1, 0, 0): rng.normal(size=(2, 2)) * 0.2, (0, 1, 0): rng.normal(size=(2, 2)) * 0.2}
    model = tbmodels_amd.Model(hop=hop, size=2, dim=3, pos=np.zeros((2, 3)), contains_cc=False)
    kpar = np.array([[0.1, 0.2], [0.3, -0.4]])
    good = np.zeros((3, 2, 2))
    hermitian = np.zeros((3, 2, 2, 2), dtype=np.complex128)
    skew = hermitian.copy()
    skew[:, :, 0, 0] = 1.0
    skew[2, 1, 0, 1] += 1e-9
    nan, inf = good.copy(), hermitian.copy()
    nan[1, 1, 0] = np.nan
    inf[0, 0, 1, 1] = np.inf
    shapes = (np.zeros((2, 2)), np.zeros(2), np.zeros((3, 2, 3)), np.zeros((3, 2, 3, 3)), np.zeros((3, 2, 2, 3)), np.zeros((0, 2, 2)),
              np.zeros((3, 0, 2)), np.zeros((0, 2, 2, 2)), np.zeros((3, 0, 2, 2)), np.zeros((1, 3, 2, 2, 2)))
    for bad in shapes:
        with pytest.raises(ValueError, match=r"\(S, M, 2\) or \(S, M, 2, 2\)"):
            model.transmission_ensemble(kpar, Z, bad)
    with pytest.raises(ValueError, match="must be real"):
        model.transmission_ensemble(kpar, Z, good + 0j)
    with pytest.raises(ValueError, match="not Hermitian"):
        model.transmission_ensemble(kpar, Z, skew)
    for bad in (nan, inf):
        with pytest.raises(ValueError, match="finite"):
            model.transmission_ensemble(kpar, Z, bad)
    for bad in (np.zeros((4097, 1, 2)), np.zeros((1, 4097, 2)), np.zeros((4097, 1, 2, 2)), np.zeros((1, 4097, 2, 2))):
        with pytest.raises(ValueError, match="at most 4096 samples, 4096 layers"):
            model.transmission_ensemble(kpar, Z, bad)
    with pytest.raises(ValueError, match="256 MiB"):
        model.transmission_ensemble(kpar, Z, np.zeros((4096, 1025, 2, 2), dtype=np.complex128))  # 64 bytes more than 256 MiB
    for bad in ({"axis": 3}, {"axis": 0.5}, {"max_iterations": 0}, {"max_iterations": 5000}):
        with pytest.raises(ValueError):
            model.transmission_ensemble(kpar, Z, good, **bad)
    with pytest.raises(ValueError):
        model.transmission_ensemble(kpar, [0.3, 0.1j], good)  # a real energy
    with pytest.raises(ValueError):
        model.transmission_ensemble(kpar[:, :1], Z, good)
    flat = tbmodels_amd.Model(hop={(1, 0): np.array([[0.5]])}, size=1, dim=2, pos=np.zeros((1, 2)), contains_cc=False)
    with pytest.raises(ValueError, match="no hopping along axis 1"):
        flat.transmission_ensemble([[0.1]], Z, np.zeros((2, 1, 1)))
    assert tbmodels_amd._model.TransmissionEnsemble._fields == ("k", "z", "layers", "length", "samples", "iterations", "transmission")  # pylint: disable=protected-access


def test_signature_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_transmission_ensemble_from_matrices": 16, "tbk_transmission_ensemble": 14, "tbk_transmission_ensemble_multi": 15,
              "tbk_transmission_ensemble_timing": 4}
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
    # tbk_transmission's arguments with (n_s, V, onsite) for V and without G
    for name in ("", "_multi"):
        single, ensemble = _lib.SIGNATURES["tbk_transmission" + name][1], _lib.SIGNATURES["tbk_transmission_ensemble" + name][1]
        at = len(single) - 7  # the position of V
        assert ensemble[:at] == single[:at] and ensemble[at + 3:] == single[at + 1:-1]
        assert ensemble[at] is ctypes.c_int64 and ensemble[at + 1] is ctypes.c_void_p and ensemble[at + 2] is ctypes.c_void_p


@pytest.mark.parametrize("n, L, M", em.GPU_CASES)
def test_bounds_of_the_gpu_cases_stay_under_the_ceiling(n, L, M):
    """every bound tests/test_gpu_ensemble.py holds the kernel to twice of"""
    H00, H01, onsite = em.gpu_case(n, L, M)
    assert H00.shape == (3, n * L, n * L) and onsite.shape == (5, M, n * L) and np.all(np.abs(onsite) <= 0.5)
    leads = tm.gpu_case(n, L, M)
    assert np.array_equal(H00, leads[0]) and np.array_equal(H01, leads[1])
    _, its, bound = em.ensemble_function(H00, H01, onsite, Z)
    print("(n, L, M) = (%d, %d, %d): N = %d, iterations %d ... %d, largest bound %.1e" % (n, L, M, n * L, its.min(), its.max(), bound.max()))
    assert bound.shape == (3, 5, 5) and np.all(bound > 0.0)
    assert bound.max() <= 1e-4
