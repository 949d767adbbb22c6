"""
The NumPy statement of the transport distribution (tools/tdf_model.py) and the host step from Sigma(E) to
transport coefficients (tbmodels_amd/transport.py), without a GPU: the weights against a triple loop and under changes of gauge, the
tetrahedron method's sum rule, positivity, the square lattice against a fine sum, H (+) H, the scales, the Sommerfeld limits of
`transport_coefficients`, and the new entry points' signatures and argument errors.
"""

import inspect
import os
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import optics_model  # noqa: E402  pylint: disable=wrong-import-position
import tdf_model  # noqa: E402  pylint: disable=wrong-import-position

U_ROUND = 2.0 ** -53


def _random_system(n_k, n, dim, seed, pair=True):
    """Ascending bands with an exactly degenerate pair (1, 2), a random unitary U and a random Hermitian D^a per axis."""
    rng = np.random.default_rng(seed)
    E = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
    if pair and n >= 3:
        E[:, 2] = E[:, 1]
    U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
    D = rng.normal(size=(n_k, dim, n, n)) + 1j * rng.normal(size=(n_k, dim, n, n))
    return E, U, (D + D.conj().transpose(0, 1, 3, 2)) / 2.0


def _norms(D):
    return np.sqrt((np.abs(D) ** 2).sum(axis=(-1, -2))).max(axis=0)


def _model_of(r_vec, hop, mesh, dim):
    """(E, U, D) of a packed model on the mesh by numpy.linalg.eigh."""
    k = optics_model.mesh_kpoints(mesh)
    H = np.zeros((len(k),) + hop.shape[1:], dtype=complex)
    for R, mat in zip(r_vec, hop):
        H += np.exp(2j * np.pi * (k @ R.astype(float)))[:, None, None] * mat[None]
    H = H + H.conj().transpose(0, 2, 1)
    E, U = np.linalg.eigh(H)
    return E, U, optics_model.derivatives(r_vec, hop, k)


# ---- 1. the weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_weights_against_a_triple_loop_and_the_gauge(dim):
    n_k, n, delta = 4, 5, 1e-8
    E, U, D = _random_system(n_k, n, dim, 30 + dim)
    got = tdf_model.weights(E, U, D, delta)
    want = np.zeros((n_k, dim, dim, n))
    for k in range(n_k):
        V = [U[k].conj().T @ D[k, a] @ U[k] for a in range(dim)]
        for a in range(dim):
            for c in range(dim):
                for b in range(n):
                    for q in range(n):
                        if abs(E[k, b] - E[k, q]) <= delta:
                            want[k, a, c, b] += (V[a][b, q] * np.conj(V[c][b, q])).real
    tol = 2.0 * tdf_model.weight_tolerance(n, float((_norms(D).sum())))
    assert np.abs(got - want).max() <= tol
    # the channels and the polarization step give the same tensor
    ch = tdf_model.channels(E, U, D, delta)
    assert ch.shape == (n_k, dim * (dim + 1) // 2, n) and ch.min() >= 0.0
    assert np.abs(tdf_model.from_channels(ch, 1) - got).max() <= 3.0 * tol
    # random column phases: nothing moves beyond rounding
    rng = np.random.default_rng(5)
    phased = U * np.exp(2j * np.pi * rng.uniform(size=(n_k, 1, n)))
    assert np.abs(tdf_model.weights(E, phased, D, delta) - got).max() <= tol
    # a random unitary mix inside the exactly degenerate pair (1, 2): the SUM over the pair stays, the split moves; with degeneracy = 0
    # only b' = b enters... and E_1 == E_2 exactly, so the pair still enters: the mask is the comparison, not a cluster label
    mix = np.linalg.qr(rng.normal(size=(n_k, 2, 2)) + 1j * rng.normal(size=(n_k, 2, 2)))[0]
    mixed = U.copy()
    mixed[:, :, 1:3] = U[:, :, 1:3] @ mix
    moved = tdf_model.weights(E, mixed, D, delta)
    assert np.abs(moved[..., 1:3].sum(axis=-1) - got[..., 1:3].sum(axis=-1)).max() <= 2.0 * tol
    others = [0, 3, 4]
    assert np.abs(moved[..., others] - got[..., others]).max() <= tol
    assert np.abs(tdf_model.weights(E, mixed, D, 0.0) - moved).max() == 0.0  # exact ties pass delta = 0
    # a pair 1e-12 apart: delta = 0 leaves it out, and then the sum over the pair does depend on the mix -- the mask matters
    near = E.copy()
    near[:, 2] = near[:, 1] + 1e-12
    with_mask = np.abs(tdf_model.weights(near, mixed, D, delta)[..., 1:3].sum(axis=-1) - tdf_model.weights(near, U, D, delta)[..., 1:3].sum(axis=-1)).max()
    without = np.abs(tdf_model.weights(near, mixed, D, 0.0)[..., 1:3].sum(axis=-1) - tdf_model.weights(near, U, D, 0.0)[..., 1:3].sum(axis=-1)).max()
    print("dim %d: pair sum under a mix: %.3e with the mask, %.3e with degeneracy = 0 (tol %.3e)" % (dim, with_mask, without, tol))
    assert with_mask <= 2.0 * tol and without > 1e3 * tol


# ---- 2, 3. the sum rule and positivity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(3, 4), (2, 3, 2)])
def test_sum_rule_and_positive_increments(mesh):
    dim, n = len(mesh), 4
    r_vec, hop, _ = syn.dense_model_arrays(n, 5, syn.MODEL_SEED + 3000 + dim, dim=dim)
    E, U, D = _model_of(np.asarray(r_vec, dtype=np.int64), hop, mesh, dim)
    grid = np.linspace(E.min() - 0.37, E.max() + 0.5, 23)
    N, sigma = tdf_model.transport_distribution(E, U, D, mesh, grid)
    w = tdf_model.weights(E, U, D)
    total = w.sum(axis=(0, 3)) / len(E)
    scale = tdf_model.scales(r_vec, hop)
    tol = tdf_model.tolerance(n, _norms(D), scale)["cumulative"]
    # (no fixed point on either side here, but the bound holds a fortiori)
    err = np.abs(N[:, :, -1] - total)
    print("mesh %s: sum rule max|N(top) - mean w| = %.3e (tol %.3e)" % (mesh, err.max(), tol.min()))
    assert np.all(err <= tol) and np.all(N[:, :, 0] == 0.0)
    assert np.array_equal(N, N.transpose(1, 0, 2)) and sigma.shape == (dim, dim, len(grid) - 1)
    lowest = min(float(np.linalg.eigvalsh(step).min()) for step in np.moveaxis(np.diff(N, axis=-1), -1, 0))
    assert lowest >= -2.0 * dim * tol.max(), lowest


# ---- 4. the square lattice ------------------------------------------------------------------------------------------------------------
def test_square_lattice_against_a_fine_sum():
    """N_xx of E = 2 (cos + cos) on 64 x 64 against the plain sum over 1024 x 1024.  The tetrahedron method's error is O(h^2) times the
    second derivatives: v_x^2 = 4 sin^2 varies by (2 pi)^2 4 per unit of k^2 and the band by as much, so C h^2 with C = 16 pi^2 / 8
    (linear interpolation's 1/8) per unit of weight: 20 h^2 = 4.8e-3 at h = 1 / 64.  The fine sum itself is a step function of 2^20
    points of weight at most 4: its own error is 4 / 1024 per energy at the van Hove steps at worst, 3.9e-3.  Found: 5.5e-4 (16 x 16: 4.6e-3, 32 x 32: 1.2e-3 -- the h^2 law down to the fine sum's own error)."""
    grid = np.linspace(-4.5, 4.5, 37)
    got, sigma = tdf_model.square_lattice_sigma((64, 64), grid)
    want = tdf_model.square_lattice_reference(grid, 1024)
    err = float(np.abs(got - want).max())
    print("square lattice 64 x 64: max|N_xx - fine sum| = %.3e" % err)
    assert err <= 20.0 / 64 ** 2 + 4.0 / 1024
    assert abs(got[-1] - 2.0) <= 1e-12  # mean of 4 sin^2 over the zone: exact on a mesh
    assert np.all(sigma >= -1e-12) and np.abs(sigma - sigma[::-1]).max() <= 1e-9  # E -> -E under k -> k + (1/2, 1/2)


# ---- 5. H (+) H ------------------------------------------------------------------------------------------------------------------------
def test_doubled_model_gives_twice_the_result():
    mesh, dim, n = (3, 4), 2, 3
    r_vec, hop, _ = syn.dense_model_arrays(n, 5, syn.MODEL_SEED + 3010, dim=dim)
    r_vec = np.asarray(r_vec, dtype=np.int64)
    double = np.zeros((len(hop), 2 * n, 2 * n), dtype=complex)
    double[:, :n, :n] = hop
    double[:, n:, n:] = hop
    E, U, D = _model_of(r_vec, hop, mesh, dim)
    E2, U2, D2 = _model_of(r_vec, double, mesh, dim)  # LAPACK picks the basis inside every doubly degenerate pair
    grid = np.linspace(E.min() - 0.2, E.max() + 0.2, 17)
    one, _ = tdf_model.transport_distribution(E, U, D, mesh, grid)
    two, _ = tdf_model.transport_distribution(E2, U2, D2, mesh, grid)
    tol = tdf_model.tolerance(2 * n, _norms(D2), tdf_model.scales(r_vec, double))["cumulative"][:, :, None]
    err = np.abs(two - 2.0 * one)
    print("H (+) H: max|N_2 - 2 N_1| = %.3e (tol %.3e)" % (err.max(), tol.min()))
    # the eigenvalues of the pairs differ by rounding between the two solves: the bound on identical inputs, plus the tetrahedron
    # sum's sensitivity to a shift of 2n u ||H|| of every corner, which the grid spacing turns into at most that over the step
    shift = 2 * n * U_ROUND * float(np.abs(E).max()) / ((grid[1] - grid[0]) / 4.0) * float(np.abs(two).max())
    assert np.all(err <= 3.0 * tol + shift)


# ---- 6. the scales ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_scales_bound_every_weight(dim):
    for seed, n in ((1, 1), (2, 4), (3, 9)):
        r_vec, hop, _ = syn.dense_model_arrays(n, 6, syn.MODEL_SEED + 3020 + seed, dim=dim)
        mesh = (3, 4) if dim == 2 else (2, 3, 2)
        E, U, D = _model_of(np.asarray(r_vec, dtype=np.int64), hop, mesh, dim)
        scale = tdf_model.scales(r_vec, hop)
        assert scale.shape == (dim * (dim + 1) // 2,) and np.all(np.frexp(scale)[0] == 0.5)  # powers of two
        for delta in (0.0, 1e-8, 10.0):  # (10: every pair enters, the whole row sum)
            ch = tdf_model.channels(E, U, D, delta) / scale[None, :, None]
            assert ch.max() <= 1.0 and ch.min() >= 0.0, (dim, n, delta, ch.max())
    assert np.array_equal(tdf_model.scales(np.zeros((1, dim), dtype=np.int64), np.ones((1, 2, 2), dtype=complex)), np.ones(dim * (dim + 1) // 2))


# ---- 7. transport coefficients ---------------------------------------------------------------------------------------------------------
class _Flat:
    def __init__(self, energies, values):
        self.energies = energies
        self.tdf = values


def test_transport_coefficients_sommerfeld_limits():
    grid = np.linspace(-3.0, 3.0, 6001)  # step 1e-3
    mid = 0.5 * (grid[:-1] + grid[1:])
    T, mu = np.array([0.02, 0.05]), np.array([-0.3, 0.0, 0.4])
    quad = (grid[1] - grid[0]) ** 2 / (24.0 * T.min() ** 2)  # the midpoint rule on a bin against the curvature of -f' x^n: relative
    const = np.zeros((2, 2, len(mid)))
    const[0, 0], const[1, 1] = 3.0, 5.0
    out = tbmodels_amd.transport_coefficients(_Flat(grid, const), T, mu)
    assert isinstance(out, tbmodels_amd.TransportCoefficients) and out.L0.shape == (2, 3, 2, 2) and out.seebeck.shape == (2, 3, 2, 2)
    assert np.array_equal(out.sigma, out.L0) and np.array_equal(out.T, T) and np.array_equal(out.mu, mu)
    assert np.abs(out.L0[..., 0, 0] - 3.0).max() <= 1e-12 and np.abs(out.L0[..., 1, 1] - 5.0).max() <= 1e-12  # exact: the window sums to 1
    assert np.abs(out.L1).max() <= 1e-12 * 5.0  # antisymmetric about mu only when mu is a grid midpoint or point: it is
    lorenz = out.kappa[..., 0, 0] / (out.sigma[..., 0, 0] * T[:, None])
    print("constant Sigma: max|kappa / (sigma T) - pi^2 / 3| = %.3e (quadrature %.3e)" % (np.abs(lorenz - np.pi ** 2 / 3).max(), 10 * quad))
    assert np.abs(lorenz - np.pi ** 2 / 3.0).max() <= 10.0 * quad * np.pi ** 2 / 3.0
    # linear Sigma: Mott's formula is exact for it (the third moment of -f' about mu vanishes)
    slope, base = 0.7, 4.0
    lin = np.zeros((2, 2, len(mid)))
    lin[0, 0] = lin[1, 1] = base + slope * mid
    out = tbmodels_amd.transport_coefficients(_Flat(grid, lin), T, mu)
    mott = -(np.pi ** 2 / 3.0) * T[:, None] * slope / (base + slope * mu[None, :])
    err = np.abs(out.seebeck[..., 0, 0] - mott).max()
    print("linear Sigma: max|S - Mott| = %.3e" % err)
    assert err <= 10.0 * quad * np.abs(mott).max() and np.abs(out.seebeck[..., 0, 1]).max() == 0.0
    # one number each
    one = tbmodels_amd.transport_coefficients(_Flat(grid, lin), 0.05, 0.4)
    assert one.L0.shape == (1, 1, 2, 2) and np.array_equal(one.seebeck[0, 0], out.seebeck[1, 2])


def test_transport_coefficients_errors():
    grid = np.linspace(-1.0, 1.0, 201)
    flat = _Flat(grid, np.ones((2, 2, 200)))
    assert tbmodels_amd.transport_coefficients(flat, 0.01, 0.5).L0.shape == (1, 1, 2, 2)
    for T, mu in ((0.02, 0.5), (0.01, -0.7), (0.01, [0.0, 0.61]), ([0.01, 0.03], 0.0)):  # mu +- 40 T leaves [-1, 1]
        with pytest.raises(ValueError, match="thermal window"):
            tbmodels_amd.transport_coefficients(flat, T, mu)
    for T, mu in ((0.0, 0.0), (-0.01, 0.0), (float("nan"), 0.0), (0.01, float("inf")), ([[0.01]], 0.0)):
        with pytest.raises(ValueError):
            tbmodels_amd.transport_coefficients(flat, T, mu)
    with pytest.raises(ValueError):
        tbmodels_amd.transport_coefficients(_Flat(grid, np.ones((2, 2, 201))), 0.01, 0.0)


# ---- 8. signatures and argument errors ---------------------------------------------------------------------------------------------------
def test_entry_points_and_python_argument_errors(monkeypatch):
    counts = {"tbk_transport_distribution": 8, "tbk_transport_distribution_multi": 9, "tbk_tdf_weights_from_eigensystem": 10, "tbk_tdf_timing": 4}
    for name, count in counts.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == count, name
    header = open(os.path.join(ROOT, "include", "tbk.h")).read()
    for name in counts:
        assert "int %s(" % name in header
    assert tbmodels_amd.TransportDistribution._fields == ("energies", "cumulative", "tdf")
    assert not hasattr(tbmodels_amd.KdotpModel, "transport_distribution")
    parameters = inspect.signature(tbmodels_amd.Model.transport_distribution).parameters
    assert list(parameters) == ["self", "mesh", "energies", "degeneracy", "cartesian"] and "convention" not in parameters
    assert parameters["degeneracy"].default == 1e-8 and parameters["degeneracy"].kind is inspect.Parameter.KEYWORD_ONLY

    r_vec, hop, pos = syn.dense_model_arrays(3, 4, syn.MODEL_SEED + 3030, dim=2)
    model = tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)

    def no_device(*_args, **_kwargs):
        raise AssertionError("an argument error must be raised before any device work")

    monkeypatch.setattr(tbmodels_amd.Model, "_handle_array", no_device)
    grid = np.linspace(-1.0, 1.0, 5)
    bad = [dict(mesh=(2,), energies=grid), dict(mesh=(2, 0), energies=grid), dict(mesh=(2, 2.5), energies=grid), dict(mesh=(2, 2), energies=[0.0]),
           dict(mesh=(2, 2), energies=[0.0, 1.0, 3.0]), dict(mesh=(2, 2), energies=grid[::-1]), dict(mesh=(2, 2), energies=grid, degeneracy=-1e-9),
           dict(mesh=(2, 2), energies=grid, degeneracy=float("nan")), dict(mesh=(2, 2), energies=grid, degeneracy=float("inf")),
           dict(mesh=(2, 2), energies=grid, degeneracy="small"), dict(mesh=(2, 2), energies=grid, cartesian=1),
           dict(mesh=(2, 2), energies=grid, cartesian=True)]  # (the model has no uc)
    for kwargs in bad:
        with pytest.raises(ValueError):
            model.transport_distribution(**kwargs)
    chain = tbmodels_amd.Model(hop={(1,): [[1.0]]}, size=1, dim=1, contains_cc=False)
    with pytest.raises(ValueError):
        chain.transport_distribution((4,), grid)
    # the scales the method passes are the model's statement
    assert np.array_equal(model._transport_scales(), tdf_model.scales(*model.packed_hop()))

    # the C entry point on the caller's arrays: every check stands in front of the one that needs a device
    lib = _lib.lib()
    E, U, D = _random_system(2, 3, 2, 1)
    E, U, D = (np.ascontiguousarray(x) for x in (E, U.astype(np.complex128), D))
    scale, out = np.ones(3), np.zeros((2, 3, 3))
    nan, inf = float("nan"), float("inf")

    def call(dim=2, n=3, nk=2, E_=E, U_=U, D_=D, delta=1e-8, scale_=scale, out_=out):
        return lib.tbk_tdf_weights_from_eigensystem(0, dim, n, nk, _lib.ptr(E_), _lib.ptr(U_), _lib.ptr(D_), delta, _lib.ptr(scale_), _lib.ptr(out_))

    statuses = [call(dim=1), call(dim=4), call(n=0), call(nk=0), call(E_=None), call(U_=None), call(D_=None), call(out_=None), call(delta=-1.0),
                call(delta=nan), call(delta=inf), call(scale_=None), call(scale_=np.array([1.0, 0.0, 1.0])), call(scale_=np.array([1.0, 1.0, -2.0])),
                call(scale_=np.array([nan, 1.0, 1.0])), call(scale_=np.array([1.0, inf, 1.0]))]
    assert statuses == [_lib.TBK_ERR_ARGUMENT] * len(statuses), statuses
    mesh = np.array([2, 2], dtype=np.int32)
    assert lib.tbk_transport_distribution(None, _lib.ptr(mesh), -1.0, 0.5, 5, 1e-8, _lib.ptr(scale), _lib.ptr(out)) == _lib.TBK_ERR_ARGUMENT
    assert lib.tbk_transport_distribution_multi(None, 1, _lib.ptr(mesh), -1.0, 0.5, 5, 1e-8, _lib.ptr(scale), _lib.ptr(out)) == _lib.TBK_ERR_ARGUMENT
