"""
tools/channels_model.py, the NumPy statement of the transmission eigenvalues, on the CPU: the pivoted Cholesky
and the one-sided Jacobi against NumPy, the channels against an independent dense route and against the transmission they sum to,
the pristine crystals, the bounds and sweep counts of every GPU input, the four C signatures and the argument errors of
`Model.transmission_channels` (raised before any device work).

Bounds (u = 2^-53), none measured on the code under test: the Cholesky reconstructs B within (N + 1) u |B|_2; the Jacobi agrees with
numpy.linalg.svd within 16 N u sigma_max (in the singular values); the channels agree with the dense route within
channels_model.tolerance and sum to T within transport_model.tolerance.  tests/test_gpu_channels.py holds the kernel
to twice channels_model.tolerance, which must stay at or below 1e-4, and the kernel's cap of the sweeps is at least twice what the
model needs on every input of that file.
"""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import channels_model as cm  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

U = cm.U_ROUND
Z = cm.GPU_Z


def _psd(N, rank, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(N, rank)) + 1j * rng.normal(size=(N, rank))
    B = a @ a.conj().T
    return (B + B.conj().T) / 2


@pytest.mark.parametrize("N, rank", [(1, 1), (2, 2), (3, 3), (3, 1), (16, 16), (17, 9), (33, 33), (64, 64), (64, 40)])
def test_pivoted_cholesky_reconstructs_psd_matrices(N, rank):
    B = _psd(N, rank, 100 + 7 * N + rank)
    L, perm, r = cm.pivoted_cholesky(B)
    err = np.linalg.norm(L @ L.conj().T - B, 2)
    print("N = %d, rank %d: found %d, |L L^H - B| = %.2e (bound %.2e)" % (N, rank, r, err, (N + 1) * U * np.linalg.norm(B, 2)))
    assert err <= (N + 1) * U * np.linalg.norm(B, 2)
    assert rank <= r <= N and len(set(perm[:r])) == r and np.all(perm[r:] == -1)
    if rank < N:
        assert r < N, "a deficient matrix was factored at full rank"
    untouched = np.setdiff1d(np.arange(N), perm[:r])
    assert np.all(L[:, untouched] == 0.0), "the columns no step took are exactly zero"
    for j in range(r):  # row perm[j] is zero in the columns of the later steps: a permuted triangle
        assert np.all(L[perm[j], perm[j + 1:r]] == 0.0)
    diagonal = np.array([L[perm[j], perm[j]] for j in range(r)])
    assert np.all(diagonal.imag == 0.0) and np.all(diagonal.real > 0.0) and np.all(np.diff(diagonal.real) <= 0.0)


def test_pivoted_cholesky_of_an_exactly_zero_row_and_column():
    B = _psd(5, 5, 3)
    B[2, :] = 0.0
    B[:, 2] = 0.0
    L, perm, r = cm.pivoted_cholesky(B)
    assert r == 4 and 2 not in perm[:r]
    assert np.all(L[2, :] == 0.0) and np.all(L[:, 2] == 0.0)
    assert np.linalg.norm(L @ L.conj().T - B, 2) <= 6 * U * np.linalg.norm(B, 2)
    L, perm, r = cm.pivoted_cholesky(np.zeros((4, 4)))
    assert r == 0 and np.all(L == 0.0) and np.all(perm == -1)
    ties = np.eye(3) * 2.0  # equal diagonals: the lowest index first
    assert list(cm.pivoted_cholesky(ties)[1]) == [0, 1, 2]


def test_round_robin_meets_every_pair_once():
    for NP in (16, 32, 64, 66):
        seen = set()
        for r in range(NP - 1):
            p, q = cm.round_pairs(NP, r)
            assert len(p) == NP // 2 and np.all(p < q) and len(set(p) | set(q)) == NP, "the pairs of a round are disjoint"
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == NP * (NP - 1) // 2


@pytest.mark.parametrize("N", [1, 2, 3, 16, 17, 64])
def test_hestenes_agrees_with_the_svd(N):
    rng = np.random.default_rng(200 + N)
    for graded in (False, True):
        t = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
        if graded:
            t = t * np.logspace(0, -12, N)[None, :]
        values, sweeps = cm.hestenes(t)
        want = np.linalg.svd(t, compute_uv=False)
        err = np.abs(np.sqrt(values) - want).max()
        print("N = %d%s: %d sweeps, max|sigma - svd| = %.2e (bound %.2e)" % (N, " graded" if graded else "", sweeps, err, 16 * N * U * want[0]))
        assert values.shape == (N,) and np.all(values >= 0.0) and np.all(np.diff(values) <= 0.0)
        assert err <= 16 * N * U * want[0]
        assert sweeps <= cm.MAX_SWEEPS // 2


def test_hestenes_keeps_zero_columns_and_raises_at_its_cap():
    rng = np.random.default_rng(9)
    t = rng.normal(size=(17, 17)) + 1j * rng.normal(size=(17, 17))
    t[:, [2, 5, 16]] = 0.0
    values, _ = cm.hestenes(t)
    assert np.all(values[14:] == 0.0) and np.all(values[:14] > 0.0)
    want = np.linalg.svd(t, compute_uv=False)
    assert np.abs(np.sqrt(values) - want).max() <= 16 * 17 * U * want[0]
    assert np.all(cm.hestenes(np.zeros((3, 3)))[0] == 0.0)
    with pytest.raises(np.linalg.LinAlgError, match="channel iteration"):
        cm.hestenes(rng.normal(size=(16, 16)), max_sweeps=2)


@pytest.mark.parametrize("n, L, M", cm.GPU_CASES)
def test_channels_against_the_dense_route_and_the_transmission(n, L, M):
    """the GPU cases themselves, three points and five energies: N = 1, 3, 16, 17, 32, 33, 64, 64"""
    H00, H01, V = cm.gpu_case(n, L, M)
    assert H00.shape == (cm.GPU_NK, n * L, n * L) and cm.GPU_NK == 3 and len(Z) == 5
    for k in range(cm.GPU_NK):
        for z in Z:  # both signs of Im z
            values, T, its, rho, P, sweeps, ranks = cm.channels(H00[k], H01[k], V, complex(z))
            bound = cm.tolerance(H00[k], H01[k], V, complex(z), its, rho, P, sweeps)
            bound_t = tm.tolerance(H00[k], H01[k], V, complex(z), its, rho, P)
            dense = cm.channels_dense(H00[k], H01[k], V, complex(z))
            assert values.shape == (n * L,) and ranks == (n * L, n * L)
            assert np.abs(values - dense).max() <= bound, (n, L, M, k, z, np.abs(values - dense).max(), bound)
            assert abs(values.sum() - T) <= bound_t, (values.sum(), T, bound_t)
            assert T == tm.transmission(H00[k], H01[k], V, complex(z))[0]
            assert np.all(values >= 0.0) and np.all(values <= 1.0 + bound) and np.all(np.diff(values) <= 0.0)
            assert cm.noise(values) == (values * (1.0 - values)).sum()


def test_channels_mp_agrees_with_the_model():
    pytest.importorskip("mpmath")
    _, H00, H01 = tm.random_case(3, 1, 1, 6300)
    V = tm.random_device(3, 2, 6301)
    for z in (Z[0], Z[1]):
        values, _, its, rho, P, sweeps, _ = cm.channels(H00[0], H01[0], V, complex(z))
        exact = cm.channels_mp(H00[0], H01[0], V, complex(z), digits=40)
        assert np.abs(values - exact).max() <= cm.tolerance(H00[0], H01[0], V, complex(z), its, rho, P, sweeps)


def test_golden_file_matches_the_model_within_its_bound():
    data = np.load(os.path.join(ROOT, "tests", "golden", "channels_mp.npz"))
    assert np.array_equal(data["Z"], Z)
    for n, L, M in cm.GPU_CASES:
        if n * L > 17:
            continue
        H00, H01, V = cm.gpu_case(n, L, M)
        values, _, _, bound, _, _ = cm.channels_function(H00, H01, V, Z)
        exact = data["Tn_%d_%d_%d" % (n, L, M)]
        assert exact.shape == values.shape
        assert np.all(np.abs(values - exact).max(axis=-1) <= bound), (n, L, M)


def test_open_channels_of_pristine_crystals():
    """the crystals of `transport_model.main` at eta = 1e-6: the T_n above 1/2 are the right-moving bands"""
    for (n, L, seed), M in (((3, 1, 1), 4), ((4, 2, 2), 3), ((6, 1, 3), 1)):
        layers, h00, h01 = tm.random_case(n, L, 1, seed)
        V = np.zeros((M, n * L, n * L), dtype=np.complex128)
        for E in (-0.8, 0.1, 0.9, 3.0):
            values = cm.channels(h00[0], h01[0], V, E + 1e-6j)[0]
            want = tm.channels(layers[0], E)
            print("n = %d L = %d M = %d E = %+.1f: %d channels, T_n = %s" % (n, L, M, E, want, np.array2string(values, precision=6)))
            assert int(np.count_nonzero(values > 0.5)) == want
            assert np.all(values[:want] > 1.0 - 1e-3) and np.all(values[want:] < 1e-3)


def _model_inputs():
    """the principal layers of the whole-call cases of tests/test_gpu_channels.py, summed directly from the hoppings"""
    out = []
    t, t_plane = 1.0, 0.3
    full = {(0, 1): np.array([[t]]), (0, -1): np.array([[t]]), (1, 0): np.array([[t_plane]]), (-1, 0): np.array([[t_plane]])}
    for kp in (0.17, -0.4, 0.05):
        H00, H01 = sm.principal(sm.layers_direct(full, 1, [kp], 1))
        out.append(("chain", H00, H01, np.array([[[0.7]], [[-0.3]]], dtype=np.complex128)))
    r_vec, hop, _ = syn.dense_model_arrays(6, 8, syn.MODEL_SEED + 2100 + 10 * 6 + 3, dim=3)
    full = sm.full_hoppings(r_vec, hop)
    total = sum(np.linalg.norm(m, 2) for m in full.values())
    full = {R: m * (2.0 / total) for R, m in full.items()}
    kpar = np.random.default_rng(31 + 6).random((3, 2)) - 0.5
    for kp in kpar:
        H00, H01 = sm.principal(sm.layers_direct(full, 2, kp, 1))
        for s in range(2):
            out.append(("synthetic", H00, H01, tm.random_device(6, 3, 177 + 6 + s)))
    return out


def test_bounds_and_sweeps_of_every_gpu_input():
    """what tests/test_gpu_channels.py asserts of the kernel, of the model alone: tolerance <= 1e-4 and sweeps <= cap / 2"""
    worst_sweeps, worst_bound, count = 0, 0.0, 0
    inputs = list(cm.gpu_inputs()) + [(label, H00, H01, V, complex(z)) for label, H00, H01, V in _model_inputs() for z in Z]
    for label, H00, H01, V, z in inputs:
        values, _, its, rho, P, sweeps, ranks = cm.channels(H00, H01, V, z)
        bound = cm.tolerance(H00, H01, V, z, its, rho, P, sweeps)
        assert bound <= 1e-4, (label, z, bound)
        assert sweeps <= cm.MAX_SWEEPS // 2, (label, z, sweeps)
        assert np.all(values >= 0.0) and np.all(values <= 1.0 + bound)
        if label.startswith("deficient"):
            N, live = H00.shape[0], 2 if label.endswith("cross") else 1
            assert min(ranks) >= live and max(ranks) <= 3 and np.all(values[:live] > 0.0), (label, z, ranks, values)
            assert np.all(values[min(ranks):] == 0.0) and np.all(values[3:] == 0.0), (label, z, ranks, values)
            if live == 1:
                assert min(ranks) == 1
            assert np.abs(values - cm.channels_dense(H00, H01, V, z)).max() <= bound
        worst_sweeps, worst_bound, count = max(worst_sweeps, sweeps), max(worst_bound, bound), count + 1
    print("%d inputs: at most %d sweeps (the cap is %d), the largest bound %.1e" % (count, worst_sweeps, cm.MAX_SWEEPS, worst_bound))
    with open(os.path.join(ROOT, "tbmodels_amd", "csrc", "tbk_channels.hip")) as handle:
        found = re.search(r"constexpr int CHAN_MAX_SWEEPS = (\d+);", handle.read())
    assert found and int(found.group(1)) == cm.MAX_SWEEPS, "the kernel's cap is the model's"
    assert cm.MAX_SWEEPS >= 2 * worst_sweeps


def test_signature_table_matches_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_transmission_channels_from_matrices": 17, "tbk_transmission_channels": 15, "tbk_transmission_channels_multi": 16,
              "tbk_transmission_channels_timing": 4}
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
    # tbk_transmission_ensemble's arguments and channels behind them
    for name in ("_from_matrices", "", "_multi"):
        ensemble, channels = _lib.SIGNATURES["tbk_transmission_ensemble" + name][1], _lib.SIGNATURES["tbk_transmission_channels" + name][1]
        assert channels[:-1] == ensemble and channels[-1] is ctypes.c_void_p
    assert _lib.SIGNATURES["tbk_transmission_channels_timing"] == _lib.SIGNATURES["tbk_transmission_ensemble_timing"]


def test_argument_errors_come_before_any_device_work():
    """Every one of these is raised from the arguments alone: the test runs without a GPU."""
    rng = np.random.default_rng(3)
    hop = {(0, 0, 1): rng.normal(size=(2, 2)) * 0.3, (1, 0, 0): rng.normal(size=(2, 2)) * 0.2, (0, 1, 0): rng.normal(size=(2, 2)) * 0.2}
    model = tbmodels_amd.Model(hop=hop, size=2, dim=3, pos=np.zeros((2, 3)), contains_cc=False)
    kpar = np.array([[0.1, 0.2], [0.3, -0.4]])
    with pytest.raises(ValueError, match="not both"):
        model.transmission_channels(kpar, Z, device=np.zeros((2, 2)), devices=np.zeros((3, 2, 2)))
    skew = np.zeros((2, 2, 2), dtype=np.complex128)
    skew[:, 0, 0] = 1.0
    skew[1, 0, 1] += 1e-9
    with pytest.raises(ValueError, match="not Hermitian"):
        model.transmission_channels(kpar, Z, device=skew)
    with pytest.raises(ValueError, match="not Hermitian"):
        model.transmission_channels(kpar, Z, devices=skew[None])
    with pytest.raises(ValueError, match="must be real"):
        model.transmission_channels(kpar, Z, devices=np.zeros((3, 2, 2)) + 0j)
    with pytest.raises(ValueError, match=r"\(S, M, 2\) or \(S, M, 2, 2\)"):
        model.transmission_channels(kpar, Z, devices=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="device must have shape"):
        model.transmission_channels(kpar, Z, device=np.zeros((3, 2, 2, 2)))
    for bad in ({"length": 0}, {"length": 1.5}, {"axis": 3}, {"max_iterations": 0}, {"max_iterations": 5000}):
        with pytest.raises(ValueError):
            model.transmission_channels(kpar, Z, **bad)
    with pytest.raises(ValueError):
        model.transmission_channels(kpar, [0.3, 0.1j])  # a real energy
    wide_hop = {(0, 1): np.eye(65) * 0.5}
    wide = tbmodels_amd.Model(hop=wide_hop, size=65, dim=2, pos=np.zeros((65, 2)), contains_cc=False)
    for how in ({}, {"device": np.zeros((1, 65))}, {"devices": np.zeros((2, 1, 65))}):
        with pytest.raises(ValueError, match="65 rows: transmission_channels takes at most 64"):
            wide.transmission_channels([[0.1]], Z, **how)
    flat = tbmodels_amd.Model(hop={(1, 0): np.array([[0.5]])}, size=1, dim=2, pos=np.zeros((1, 2)), contains_cc=False)
    for how in ({}, {"devices": np.zeros((2, 1, 1))}):
        with pytest.raises(ValueError, match="no hopping along axis 1"):
            flat.transmission_channels([[0.1]], Z, **how)
    assert tbmodels_amd._model.TransmissionChannels._fields == (  # pylint: disable=protected-access
        "k", "z", "layers", "length", "samples", "iterations", "transmission", "channels", "noise")
