"""
The two-stage kernel and the slice reduction of the four-index susceptibility chi_0[i, l; j, m](q) (csrc/tbk_chi.hip, DESIGN.md
section 29) against tools/chi_model.py `susceptibility_tensor` -- the definition, not the kernels' factorisation -- on identical
(E, U), and `Model.susceptibility_tensor` against its properties, against the model fed with the eigensystem `Model.eigh` returns for
the same mesh, and against `Model.orbital_susceptibility` and `Model.susceptibility`.

Bound: chi_model.tensor_tolerance per component of an entry -- derived from the number formats, the sizes and an
allowance of 2 ulps for exp and expm1 per side; nothing measured on the kernels enters it.  Identities of bits (exact Hermiticity,
properties 6, 7, 9 and 10, mu against `fermi_level`, two handles against one, q batches) are asserted as such.  Every case prints its
measured maximum.
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
import chi_model  # noqa: E402  pylint: disable=wrong-import-position
import dos_model  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

MU = 0.1
TEMPERATURES = (0.05, 0.5)
_CACHE = {}


def _eigensystem(mesh, n):
    """`_eigensystem` of tests/test_gpu_chi.py: random ascending bands, band 0 flat, bands 1 and 2 an exact degenerate pair inside every
    k-point, random unitary U; shared by the cases and never written."""
    key = (mesh, n)
    if key not in _CACHE:
        n_k = int(np.prod(mesh))
        rng = np.random.default_rng(7300 + 41 * n_k + n)
        eig = np.sort(rng.uniform(-1.0, 1.0, (n_k, n)), axis=-1)
        eig[:, 0] = -1.25 if n > 1 else 0.125
        if n >= 3:
            eig[:, 2] = eig[:, 1]
        U = np.linalg.qr(rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n)))[0]
        eig, U = np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)
        for array in (eig, U):
            array.setflags(write=False)
        _CACHE[key] = (eig, U)
    return _CACHE[key]


def _vectors(mesh):
    """0, e_0, a vector with every component non-zero, its negative, the same shifted by whole mesh periods and a duplicate of it; and
    the indices of the (q, -q) pair, the (vector, shifted) pair and the (original, duplicate) pair."""
    dim = len(mesh)
    unit = np.eye(dim, dtype=np.int64)
    full = np.array([d + 1 for d in range(dim)], dtype=np.int64)
    shift = np.array([(-1) ** d * (d + 2) * mesh[d] for d in range(dim)], dtype=np.int64)
    q = np.stack([np.zeros(dim, dtype=np.int64), unit[0], full, -full, full + shift, full])
    return np.ascontiguousarray(q), (2, 3), (2, 4), (2, 5)


def _from_eigensystem(mesh, eig, U, q, T, mu=MU, orbitals=None, part_bytes=0, k_slice=0):
    n = eig.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    q = np.ascontiguousarray(q, dtype=np.int64)
    chosen = None if orbitals is None else np.ascontiguousarray(orbitals, dtype=np.int32)
    m = n if chosen is None else len(chosen)
    out = np.full((len(q), m, m, m, m), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_tensor_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), float(mu), float(T),
                                                          len(q), _lib.ptr(q), m, _lib.ptr(chosen), int(part_bytes), int(k_slice),
                                                          _lib.ptr(out)))
    return out


def _plan(n_k, n_orb, m, n_q, part_bytes=0, k_slice=0):
    out = (ctypes.c_int64 * 6)()
    _lib.check(_lib.lib().tbk_chi_tensor_plan(n_k, n_orb, m, n_q, part_bytes, k_slice, out))
    return {"row_blocks": out[0], "blocks": out[1], "k_slice": out[2], "slices": out[3], "batch": out[4], "batches": out[5]}


def _per_vector(plan, m):
    """The bytes of one vector's partial sums: the m (m + 1) / 2 rows and m^2 columns padded to 64."""
    rows, cols = -(-(m * (m + 1) // 2) // 64) * 64, -(-(m * m) // 64) * 64
    return 16 * plan["slices"] * rows * cols


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _worst(got, want):
    gap = np.asarray(got) - np.asarray(want)
    return float(max(np.abs(gap.real).max(), np.abs(gap.imag).max()))


def _matrix(chi):
    """[..., i, l, j, m] as the m^2 x m^2 matrices with rows (i, l) and columns (j, m)."""
    m = chi.shape[-1]
    return np.ascontiguousarray(chi).reshape(chi.shape[:-4] + (m * m, m * m))


def _exactly_hermitian(chi):
    matrix = _matrix(chi)
    diagonal = np.ascontiguousarray(np.diagonal(matrix, axis1=-2, axis2=-1).imag)
    no_minus_zero = not np.any(np.signbit(_bits(chi)) & (_bits(chi) == 0.0))
    return bool(np.array_equal(matrix, np.conj(np.swapaxes(matrix, -1, -2))) and np.all(diagonal == 0.0) and no_minus_zero)


def _select(full, at):
    """The entries of a tensor [q, i, l, j, m] at the positions `at` on all four axes."""
    at = np.asarray(at)
    return np.ascontiguousarray(full[:, at][:, :, at][:, :, :, at][:, :, :, :, at])


def _orbital(mesh, eig, U, q, T, orbitals=None):
    n = eig.shape[-1]
    chosen = None if orbitals is None else np.ascontiguousarray(orbitals, dtype=np.int32)
    m = n if chosen is None else len(chosen)
    out = np.full((len(q), m, m), np.nan + 1j * np.nan, dtype=np.complex128)
    _lib.check(_lib.lib().tbk_chi_orbital_from_eigensystem(0, len(mesh), _lib.ptr(np.ascontiguousarray(mesh, dtype=np.int32)), n, _lib.ptr(eig),
                                                           _lib.ptr(U), MU, float(T), len(q), _lib.ptr(q), None, m, _lib.ptr(chosen), 0, 0,
                                                           _lib.ptr(out)))
    return out


def _kernel_case(mesh, n, orbitals=None, temperatures=TEMPERATURES, identities=True):
    eig, U = _eigensystem(mesh, n)
    n_k = int(np.prod(mesh))
    q, inverse, shifted, duplicate = _vectors(mesh)
    order = np.random.default_rng(9).permutation(len(q))
    m = n if orbitals is None else len(orbitals)
    report = []
    for T in temperatures:
        bound = chi_model.tensor_tolerance(n_k, n, T)
        where = (mesh, n, None if orbitals is None else list(orbitals), T)
        got = _from_eigensystem(mesh, eig, U, q, T, orbitals=orbitals)
        want = chi_model.susceptibility_tensor(eig, U, mesh, q, MU, T, orbitals)
        err = _worst(got, want)
        report.append("T = %g: %.3e (bound %.3e, ratio %.2e)" % (T, err, bound, err / bound))
        assert np.all(np.isfinite(_bits(got))) and err <= bound, where + (err, bound)
        assert _exactly_hermitian(got), where + ("not exactly Hermitian",)  # property 1
        assert _same(got[shifted[0]], got[shifted[1]]), where + ("a whole mesh period changed bits",)  # property 7
        assert _same(got[duplicate[0]], got[duplicate[1]]), where + ("a duplicate differs",)  # property 9 ...
        lowest = np.linalg.eigvalsh(_matrix(got)).min()
        assert lowest >= -bound * m * m, where + ("not positive semidefinite", lowest)
        a, b = inverse  # property 4: chi(-q)[i, l; j, m] = chi(q)[m, j; l, i]
        assert _worst(got[b], got[a].transpose(3, 2, 1, 0)) <= bound and _worst(got[0], got[0].transpose(3, 2, 1, 0)) <= bound, where + ("-q",)
        if not identities:
            continue
        assert _same(got, _from_eigensystem(mesh, eig, U, q, T, orbitals=orbitals)), where + ("two calls differ",)
        assert _same(got[order], _from_eigensystem(mesh, eig, U, q[order], T, orbitals=orbitals)), where + ("the order changed bits",)
        for index in (0, 3):
            alone = _from_eigensystem(mesh, eig, U, q[index:index + 1], T, orbitals=orbitals)
            assert _same(alone[0], got[index]), where + ("the rest of the list changed bits",)
        # property 2: the density-density block against the orbital-resolved kernels
        block = np.einsum("qiijj->qij", got)
        both = bound + chi_model.orbital_tolerance(n_k, n, T)
        assert _worst(block, _orbital(mesh, eig, U, q, T, orbitals)) <= both, where + ("the density-density block",)
        if orbitals is None:  # property 3: the sum rule against the scalar kernels
            scalar = np.full(len(q), np.nan)
            _lib.check(_lib.lib().tbk_chi_from_eigensystem(0, len(mesh), _lib.ptr(np.ascontiguousarray(mesh, dtype=np.int32)), n, _lib.ptr(eig),
                                                           _lib.ptr(U), MU, float(T), len(q), _lib.ptr(q), None, _lib.ptr(scalar)))
            total = block.sum(axis=(1, 2))
            margin = n * n * bound + chi_model.tolerance(n_k, n, T)
            assert np.abs(total.real - scalar).max() <= margin and np.abs(total.imag).max() <= margin, where + ("the sum rule",)
    return report


# ---- 1. the kernels against the model on the same (E, U) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 9, 16])
def test_kernels_match_the_model_on_2x3x2(n):
    plan = _plan(12, n, n, 6)
    rows, cols = -(-(n * (n + 1) // 2) // 64), -(-(n * n) // 64)
    assert plan["row_blocks"] == rows and plan["blocks"] == rows * cols and plan["batches"] == 1 and plan["batch"] == 6
    assert plan["k_slice"] * plan["slices"] >= 12 > plan["k_slice"] * (plan["slices"] - 1)
    for line in _kernel_case((2, 3, 2), n):
        print("mesh (2, 3, 2) n = %d, all selected: max|chi - model|, %s" % (n, line))


@pytest.mark.parametrize("n", [17, 33, 64])
@pytest.mark.parametrize("m", [1, 3, 16])
def test_selections_match_the_model_on_2x3x2(n, m):
    rng = np.random.default_rng(100 * n + m)
    unsorted = rng.permutation(n)[:m]
    if m > 1 and np.all(np.diff(unsorted) > 0):
        unsorted = unsorted[::-1]
    ends = np.concatenate([[n - 1], rng.permutation(np.arange(1, n - 1))[:m - 2], [0]])[:m] if m > 1 else np.array([n - 1])
    for chosen in (unsorted, ends):
        for line in _kernel_case((2, 3, 2), n, orbitals=chosen, temperatures=(0.05,), identities=(m < 16)):
            print("mesh (2, 3, 2) n = %d, selected %s: max|chi - model|, %s" % (n, chosen.tolist(), line))


def test_kernels_match_the_model_at_65_orbitals():
    for line in _kernel_case((2, 3, 2), 65, orbitals=np.array([64, 3, 20]), temperatures=(0.05,)):  # one band past a round of panels
        print("mesh (2, 3, 2) n = 65, selected [64, 3, 20]: max|chi - model|, %s" % line)


def test_kernels_match_the_model_at_257_orbitals():
    for line in _kernel_case((1, 2), 257, orbitals=np.array([256, 250]), temperatures=(0.05,)):
        print("mesh (1, 2) n = 257, selected [256, 250]: max|chi - model|, %s" % line)


def test_kernels_match_the_model_on_4x4x4():
    plan = _plan(64, 9, 9, 6)
    assert plan["slices"] >= 2 and plan["blocks"] == 2  # several slices, two column blocks
    for line in _kernel_case((4, 4, 4), 9):
        print("mesh (4, 4, 4) n = 9 max|chi - model|, %s" % line)


def test_phases_and_degenerate_bases_do_not_matter():
    """Property 8: random column phases and a random rotation inside the degenerate pair (bands 1, 2) of every k-point."""
    mesh, n, T = (2, 3, 2), 9, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _ = _vectors(mesh)
    rng = np.random.default_rng(55)
    angle = rng.uniform(0.0, 2.0 * np.pi, (12, 1, n))
    turned = U * (np.cos(angle) + 1j * np.sin(angle))
    rotation = np.linalg.qr(rng.normal(size=(12, 2, 2)) + 1j * rng.normal(size=(12, 2, 2)))[0]
    turned[:, :, 1:3] = turned[:, :, 1:3] @ rotation
    turned = np.ascontiguousarray(turned)
    # the rotated eigenvectors are another input: each side is within half the bound of the exact value of ITS input, and the inputs
    # differ by the rounding of the rotation, a few u per component of U, which the amplitudes' allowance covers twice over
    bound = 2.0 * chi_model.tensor_tolerance(12, n, T)
    one, two = _from_eigensystem(mesh, eig, U, q, T), _from_eigensystem(mesh, eig, turned, q, T)
    print("column phases and cluster rotations: max difference %.3e (bound %.3e)" % (_worst(one, two), bound))
    assert _worst(one, two) <= bound


# ---- 2. selections, batches and slices -----------------------------------------------------------------------------------------------
def test_overlapping_selections_of_17_orbitals_share_their_bits():
    """Property 10 where the full tensor cannot be asked for (m > 16)."""
    mesh, n, T = (2, 3, 2), 17, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _ = _vectors(mesh)
    rng = np.random.default_rng(91)
    wide = rng.permutation(n)[:16]
    other = np.concatenate([[o for o in range(n) if o not in wide], rng.permutation(wide)[:15]])  # the orbital `wide` leaves out, 15 of its
    big, big2 = _from_eigensystem(mesh, eig, U, q, T, orbitals=wide), _from_eigensystem(mesh, eig, U, q, T, orbitals=other)
    assert _exactly_hermitian(big) and _exactly_hermitian(big2)
    common = [o for o in wide if o in other]
    at, at2 = [list(wide).index(o) for o in common], [list(other).index(o) for o in common]
    assert _same(_select(big, at), _select(big2, at2)), "two selections of 16 differ on their common entries"
    for size in (3, 1):
        for chosen in (rng.permutation(wide)[:size], wide[[15, 0, 7][:size]]):
            small = _from_eigensystem(mesh, eig, U, q, T, orbitals=chosen)
            assert small.shape == (len(q),) + (size,) * 4 and _exactly_hermitian(small)
            assert _same(small, _select(big, [list(wide).index(o) for o in chosen])), (chosen.tolist(), "the selection changed bits")


def test_every_selection_has_the_bits_of_the_full_tensor():
    mesh, n, T = (2, 3, 2), 9, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _ = _vectors(mesh)
    full = _from_eigensystem(mesh, eig, U, q, T)
    rng = np.random.default_rng(92)
    for size in range(1, n + 1):  # one block up to 8 orbitals, two column blocks at 9
        for chosen in (rng.permutation(n)[:size], np.concatenate([[n - 1], rng.permutation(n - 1)[:size - 1]])):
            got = _from_eigensystem(mesh, eig, U, q, T, orbitals=chosen)
            assert _same(got, _select(full, chosen)), (chosen.tolist(), "the selection changed bits")


def test_q_batches_change_no_bit():
    mesh, n, T = (2, 3, 2), 9, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _ = _vectors(mesh)
    plan = _plan(12, n, n, len(q))
    per_vector = _per_vector(plan, n)
    whole = _from_eigensystem(mesh, eig, U, q, T)
    for room in (1, 4):
        forced = _plan(12, n, n, len(q), part_bytes=room * per_vector + 8)
        assert forced["batch"] == room and forced["batches"] == (len(q) + room - 1) // room and forced["k_slice"] == plan["k_slice"]
        got = _from_eigensystem(mesh, eig, U, q, T, part_bytes=room * per_vector + 8)
        assert _same(got, whole), (room, "the batches changed bits")
    assert _plan(12, n, n, len(q), part_bytes=per_vector - 8)["batch"] == 0
    out = np.zeros((len(q), n, n, n, n), dtype=np.complex128)
    mesh32 = np.array(mesh, dtype=np.int32)
    assert _lib.lib().tbk_chi_tensor_from_eigensystem(0, 3, _lib.ptr(mesh32), n, _lib.ptr(eig), _lib.ptr(U), MU, T, len(q), _lib.ptr(q), n, None,
                                                      per_vector - 8, 0, _lib.ptr(out)) == _lib.TBK_ERR_MEMORY


def test_forced_slices_stay_within_the_bound():
    mesh, n, T = (5, 5, 5), 3, 0.05
    eig, U = _eigensystem(mesh, n)
    q, _, _, _ = _vectors(mesh)
    own = _plan(125, n, n, len(q))
    print("plan of 125 points, 3 orbitals:", own)
    assert 1 < own["k_slice"] < 125 and own["slices"] == -(-125 // own["k_slice"])
    assert _plan(125, n, 1, 1)["k_slice"] == own["k_slice"] == _plan(125, n, 2, 4000, part_bytes=1 << 24)["k_slice"]  # of (NK, n_orb) alone
    want = chi_model.susceptibility_tensor(eig, U, mesh, q, MU, T)
    bound = chi_model.tensor_tolerance(125, n, T)
    runs = {0: _from_eigensystem(mesh, eig, U, q, T)}
    assert _same(runs[0], _from_eigensystem(mesh, eig, U, q, T, k_slice=own["k_slice"]))  # the library's own, passed explicitly
    for k_slice in (1, 5, 125):
        assert _plan(125, n, n, len(q), k_slice=k_slice)["slices"] == -(-125 // k_slice)
        runs[k_slice] = _from_eigensystem(mesh, eig, U, q, T, k_slice=k_slice)
    for k_slice, got in runs.items():
        print("k_slice = %d: max|chi - model| = %.3e (bound %.3e)" % (k_slice, _worst(got, want), bound))
        assert _worst(got, want) <= bound and _exactly_hermitian(got)
        for other in runs.values():
            assert _worst(got, other) <= bound


def test_extreme_temperatures_and_chemical_potentials():
    mesh, n = (2, 3, 2), 17
    eig, U = _eigensystem(mesh, n)
    q, _, _, _ = _vectors(mesh)
    chosen = np.array([16, 0, 5, 9])
    for T in TEMPERATURES:
        for mu in (float(eig.min()) - 746.0 * T, float(eig.max()) + 746.0 * T):  # property 6
            flat = _bits(_from_eigensystem(mesh, eig, U, q, T, mu=mu, orbitals=chosen))
            assert np.all(flat == 0.0) and not np.any(np.signbit(flat)), (T, mu)
    hot = 1e9 * float(np.ptp(eig))
    got = _from_eigensystem(mesh, eig, U, q, hot, orbitals=chosen)  # property 5: 4 T chi -> delta_ij delta_lm
    unit = np.einsum("ij,lm->iljm", np.eye(4), np.eye(4))[None]
    err, bound = _worst(4.0 * hot * got, unit), 4.0 * hot * chi_model.tensor_tolerance(12, n, hot) + 1e-8
    print("T = 1e9 bandwidths: max|4 T chi - 1| = %.3e (bound %.3e)" % (err, bound))
    assert np.all(np.isfinite(_bits(got))) and err <= bound
    for T in (1e-3, 1e3):
        assert np.all(np.isfinite(_bits(_from_eigensystem(mesh, eig, U, q, T, orbitals=chosen))))


# ---- 3. whole calls ------------------------------------------------------------------------------------------------------------------
def _silicon(sparse=False):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    if sparse:
        model.set_sparse()
    return model


def _dense9(dim):
    r_vec, hop, pos = syn.dense_model_arrays(9, 6, syn.MODEL_SEED + 1400 + dim, dim=dim)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos)


CALLS = {"silicon CSR": (lambda: _silicon(True), (2, 3, 2), 4.5), "dense 9, 3-D": (lambda: _dense9(3), (2, 3, 2), 3.1),
         "dense 9, 2-D": (lambda: _dense9(2), (3, 4), 3.1)}


@pytest.mark.parametrize("name", list(CALLS))
def test_properties_of_a_whole_call(name):
    make, mesh, n_el = CALLS[name]
    model = make()
    n, n_k = model.size, int(np.prod(mesh))
    q, inverse, shifted, duplicate = _vectors(mesh)
    eig, vec = model.eigh(dos_model.mesh_kpoints(mesh))
    level = model.fermi_level(mesh, n_el)
    chosen = np.array([n - 1, 0, 2])
    for T in TEMPERATURES:
        tol = chi_model.tensor_tolerance(n_k, n, T)
        result = model.susceptibility_tensor(mesh, q, temperature=T, n_electrons=n_el)
        assert isinstance(result, tbmodels_amd.SusceptibilityTensor) and result.mu == level  # bit for bit
        assert result.q.dtype == np.int64 and np.array_equal(result.q, q) and result.orbitals.dtype == np.int64
        assert np.array_equal(result.orbitals, np.arange(n)) and result.chi.shape == (len(q), n, n, n, n) and result.chi.dtype == np.complex128
        chi = result.chi
        assert _exactly_hermitian(chi) and np.linalg.eigvalsh(_matrix(chi)).min() >= -tol * n * n  # property 1
        err_m = _worst(chi, chi_model.susceptibility_tensor(eig, vec, mesh, q, level.mu, T))
        block = np.einsum("qiijj->qij", chi)
        orbital = model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el).chi
        err_2 = _worst(block, orbital) / (tol + chi_model.orbital_tolerance(n_k, n, T))  # property 2
        scalar = model.susceptibility(mesh, q, temperature=T, n_electrons=n_el).chi
        err_3 = np.abs(block.sum(axis=(1, 2)) - scalar).max() / (n * n * tol + chi_model.tolerance(n_k, n, T))  # property 3
        err_4 = _worst(chi[inverse[1]], chi[inverse[0]].transpose(3, 2, 1, 0))  # property 4
        assert _same(chi[shifted[0]], chi[shifted[1]]) and _same(chi[duplicate[0]], chi[duplicate[1]])  # properties 7 and 9
        by_energy = model.susceptibility_tensor(mesh, q, temperature=T, energy=level.mu)
        assert by_energy.mu.mu == level.mu and _same(by_energy.chi, chi)
        part = model.susceptibility_tensor(mesh, q, temperature=T, n_electrons=n_el, orbitals=chosen)
        assert np.array_equal(part.orbitals, chosen) and _same(part.chi, _select(chi, chosen))  # property 10
        print("%s %s T = %g: chi - model %.3e, chi(-q) against chi(q) %.3e (bound %.3e); density block %.3e, sum rule %.3e of their margins"
              % (name, mesh, T, err_m, err_4, tol, err_2, err_3))
        assert max(err_m, err_4) <= tol and err_2 <= 1.0 and err_3 <= 1.0
    edges = model.band_edges(mesh)
    below = model.susceptibility_tensor(mesh, q, temperature=0.05, energy=float(edges.emin.min()) - 746.0 * 0.05).chi  # property 6
    assert np.all(_bits(below) == 0.0) and not np.any(np.signbit(_bits(below)))


def test_two_handles_give_the_bits_of_one():
    for make, mesh, n_el in (CALLS["silicon CSR"], CALLS["dense 9, 2-D"]):
        model = make()
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        q, _, _, _ = _vectors(mesh)
        for kwargs in ({}, {"orbitals": [3, 1]}):
            one = model.susceptibility_tensor(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs)
            two = twin.susceptibility_tensor(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs)
            assert len(twin._handles) == 2 and two.mu == one.mu
            assert _same(one.chi, two.chi), (kwargs, _worst(one.chi, two.chi))
            assert _same(one.chi[:1], twin.susceptibility_tensor(mesh, q[:1], temperature=0.05, n_electrons=n_el, **kwargs).chi)
            assert _same(one.chi, model.susceptibility_tensor(mesh, q, temperature=0.05, n_electrons=n_el, **kwargs).chi)  # the same call again


# ---- 4. timing and arguments ---------------------------------------------------------------------------------------------------------
def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    q = np.array([[1, 0, 0], [2, 1, 0]], dtype=np.int64)
    model.susceptibility_tensor((4, 4, 4), q, temperature=0.1, n_electrons=4.5)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    timed = model.susceptibility_tensor((4, 4, 4), q, temperature=0.1, n_electrons=4.5)
    _lib.check(_lib.lib().tbk_chi_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), 2 vectors: %d calls, Fermi tables %.3f ms, two-stage kernel %.3f ms, reduction %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and min(ms) > 0.0
    model.set_option(_lib.TBK_OPT_TIMING, 0)
    assert _same(timed.chi, model.susceptibility_tensor((4, 4, 4), q, temperature=0.1, n_electrons=4.5).chi)


def test_python_argument_errors_come_before_device_work(monkeypatch):
    big = tbmodels_amd.Model.from_packed(*syn.dense_model_arrays(17, 2, syn.MODEL_SEED + 1500)[:2])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    q = [[1, 0, 0]]
    with pytest.raises(ValueError):
        big.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0)  # 17 orbitals, all selected
    with pytest.raises(ValueError):
        big.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=list(range(17)))
    for bad in ([1, 1], [0, 17], [-1], [], "01", [0.5]):
        with pytest.raises(ValueError):
            big.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=bad)
    with pytest.raises(ValueError):
        one_d.susceptibility_tensor((8,), [[1]], temperature=0.1, energy=0.0)
    with pytest.raises(TypeError):
        big.susceptibility_tensor((2, 2, 2), q, temperature=0.1, energy=0.0, orbitals=[0], convention=2)  # there is no such argument


def test_c_argument_errors():
    lib = _lib.lib()
    eig, U = _eigensystem((2, 3, 2), 9)
    eig17, U17 = _eigensystem((2, 3, 2), 17)
    mesh = np.array([2, 3, 2], dtype=np.int32)
    q = np.array([[0, 0, 0], [1, 0, -1]], dtype=np.int64)
    some, twice_same, beyond = (np.array(v, dtype=np.int32) for v in ([4, 0, 8], [4, 0, 4], [4, 9, 0]))
    chi, four = np.zeros((2, 9, 9, 9, 9), dtype=np.complex128), np.zeros(4)

    def call(n_orb=9, eig_=eig, U_=U, T=0.1, n_q=2, q_=q, m=9, orbitals=None, part_bytes=0, k_slice=0, out=chi):
        return lib.tbk_chi_tensor_from_eigensystem(0, 3, _lib.ptr(mesh), n_orb, _lib.ptr(eig_), _lib.ptr(U_), 0.0, T, n_q, _lib.ptr(q_), m,
                                                   _lib.ptr(orbitals), part_bytes, k_slice, _lib.ptr(out))

    assert call() == _lib.TBK_OK and call(m=3, orbitals=some) == _lib.TBK_OK
    bad = [call(out=None), call(m=0), call(m=-1), call(m=3), call(m=10), call(U_=None), call(eig_=None), call(q_=None), call(T=0.0), call(n_q=0),
           call(m=3, orbitals=twice_same), call(m=3, orbitals=beyond), call(part_bytes=-1), call(k_slice=-1),
           call(n_orb=17, eig_=eig17, U_=U17, m=17), call(n_orb=17, eig_=eig17, U_=U17, m=17, orbitals=np.arange(17, dtype=np.int32))]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    model = _silicon()
    handle = model._staged_all()[0]
    plan = (ctypes.c_int64 * 6)()
    out8 = np.zeros((2, 8, 8, 8, 8), dtype=np.complex128)
    three = np.array([7, 0, 3], dtype=np.int32)
    m32, pq, p4, po = _lib.ptr(mesh), _lib.ptr(q), _lib.ptr(four), _lib.ptr(out8)

    def whole(handle_=handle, mesh_=m32, mode=0, value=0.0, T=0.1, n_q=2, q_=pq, m=8, orbitals=None, mu_=p4, out=po):
        return lib.tbk_susceptibility_tensor(handle_, mesh_, mode, value, T, n_q, q_, m, _lib.ptr(orbitals), mu_, out)

    assert whole() == _lib.TBK_OK and whole(m=3, orbitals=three) == _lib.TBK_OK
    bad = [whole(handle_=None), whole(mesh_=None), whole(mode=2), whole(T=0.0), whole(n_q=0), whole(q_=None), whole(mu_=None), whole(out=None),
           whole(m=0), whole(m=9), whole(m=3), whole(m=3, orbitals=np.array([7, 7, 3], dtype=np.int32)),
           lib.tbk_susceptibility_tensor_multi(None, 1, m32, 1, 4.0, 0.1, 2, pq, 8, None, p4, po),
           lib.tbk_chi_tensor_plan(0, 8, 8, 2, 0, 0, plan), lib.tbk_chi_tensor_plan(64, 0, 1, 2, 0, 0, plan),
           lib.tbk_chi_tensor_plan(64, 8, 0, 2, 0, 0, plan), lib.tbk_chi_tensor_plan(64, 8, 9, 2, 0, 0, plan),
           lib.tbk_chi_tensor_plan(64, 32, 17, 2, 0, 0, plan), lib.tbk_chi_tensor_plan(64, 8, 8, 0, 0, 0, plan),
           lib.tbk_chi_tensor_plan(64, 8, 8, 2, -1, 0, plan), lib.tbk_chi_tensor_plan(64, 8, 8, 2, 0, -1, plan),
           lib.tbk_chi_tensor_plan(64, 8, 8, 2, 0, 0, None)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
