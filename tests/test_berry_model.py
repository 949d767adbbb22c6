"""
tools/berry_model.py, the NumPy statement of the lattice Berry flux and the Chern numbers, on the Qi-Wu-Zhang
model in two and three dimensions and on smooth random unitaries; the conditions every test input of the GPU file must meet, checked
on the reference alone; and the argument checks of `Model.berry_flux` and of the C interface that need no device.

Bounds: berry_model.link_tolerance per link angle, four of them per flux.  Chern numbers are compared as integers.
"""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import berry_model as bm  # noqa: E402  pylint: disable=wrong-import-position
import chi_model  # noqa: E402  pylint: disable=wrong-import-position

SIGMA_FLOOR = 0.2    # condition 1: every link's smallest singular value
FLUX_CEILING = 0.45  # condition 2: every reference |F| in turns
AMPLITUDE = 0.25     # of the smooth unitaries: condition 1 holds at every size used
PHASE_SPREAD = 0.25  # of the phase tables that go with them, in radians: condition 1 still holds

#: the inputs (c) of the GPU file: orbitals, band sets, mesh
SMOOTH_CASES = ((5, ((0, 1), (1, 4), (0, 5)), (4, 5)), (17, ((0, 16), (3, 4), (0, 17)), (3, 4, 2)), (64, ((0, 64), (0, 33), (10, 27)), (3, 3)),
                (80, ((0, 65), (0, 80)), (2, 3)))
#: the inputs (a): u, mesh, the Chern number of the lower band
QWZ_CASES = ((1.0, (6, 6), 1), (1.0, (5, 7), 1), (-1.0, (8, 8), -1), (2.5, (6, 6), 0))
_CACHE = {}


def smooth_case(n, mesh):
    """U of input (c), shared and never written."""
    key = ("smooth", n, tuple(mesh))
    if key not in _CACHE:
        U = bm.smooth_unitaries(mesh, n, AMPLITUDE, 100 + n)
        U.setflags(write=False)
        _CACHE[key] = U
    return _CACHE[key]


def qwz_case(u, mesh):
    key = ("qwz", u, tuple(mesh))
    if key not in _CACHE:
        U = np.ascontiguousarray(bm.eigenvectors(bm.qwz_hoppings(u, len(mesh)), mesh))
        U.setflags(write=False)
        _CACHE[key] = U
    return _CACHE[key]


def check_conditions(U, mesh, sets, phases=None):
    """Conditions 1 and 2 on the reference alone; returns (reference, sigma_min per set)."""
    smallest = bm.sigma_min(U, mesh, sets, phases)
    ref = bm.berry_flux(U, mesh, sets, phases)
    turns = np.abs(ref["flux"]).max() / bm.TWO_PI
    assert smallest.min() >= SIGMA_FLOOR, (mesh, sets, smallest)
    assert turns <= FLUX_CEILING, (mesh, sets, turns)
    return ref, smallest


def flux_bounds(n, sets, smallest):
    """Four links' tolerance per set, shaped to broadcast over flux [S][P][NK]."""
    return np.array([4.0 * bm.link_tolerance(n, hi - lo, s) for (lo, hi), s in zip(sets, smallest)])[:, None, None]


def silicon_hoppings():
    g = load_golden("silicon")
    return {tuple(int(x) for x in R): np.asarray(mat) for R, mat in zip(g["R"], g["hop"])}, g


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u, mesh, want", QWZ_CASES)
def test_qwz_chern_numbers(u, mesh, want):
    U = qwz_case(u, mesh)
    ref, smallest = check_conditions(U, mesh, [(0, 1)])
    print("QWZ u = %g %r: max |F| = %.3f turn, sigma_min = %.3f" % (u, mesh, np.abs(ref["flux"]).max() / bm.TWO_PI, smallest.min()))
    assert [c.tolist() for c in ref["chern"]] == [[[want]]]
    assert all(not low.any() for low in ref["low"])
    upper = bm.berry_flux(U, mesh, [(1, 2)])
    assert [c.tolist() for c in upper["chern"]] == [[[-want]]]  # the two bands together are trivial


def test_weyl_pair_is_a_jump_of_the_slice_chern_number():
    mesh = (7, 7, 4)
    U = qwz_case(1.5, mesh)
    ref, smallest = check_conditions(U, mesh, [(0, 1)])
    print("3-D u = 1.5 %r: max |F| = %.3f turn, sigma_min = %.3f" % (mesh, np.abs(ref["flux"]).max() / bm.TWO_PI, smallest.min()))
    assert ref["planes"] == ((0, 1), (0, 2), (1, 2))
    assert ref["chern"][0].tolist() == [[0, 1, 1, 1]]
    assert ref["chern"][1].tolist() == [[0] * 7] and ref["chern"][2].tolist() == [[0] * 7]
    assert all(not low.any() for low in ref["low"])
    assert bm.chern_flat(ref["chern"]).shape == (1, 4 + 7 + 7)


@pytest.mark.parametrize("n, sets, mesh", SMOOTH_CASES)
def test_smooth_unitaries_meet_the_conditions(n, sets, mesh):
    U = smooth_case(n, mesh)
    assert np.abs(np.einsum("kij,kil->kjl", U.conj(), U) - np.eye(n)).max() <= 64 * n * 2.0 ** -53
    ref, smallest = check_conditions(U, mesh, list(sets))
    check_conditions(U, mesh, list(sets), bm.random_phases(len(mesh), n, PHASE_SPREAD, 5 + n))
    print("n = %d %r: sigma_min = %s, max |F| = %.3f turn" % (n, mesh, smallest, np.abs(ref["flux"]).max() / bm.TWO_PI))
    assert all(not low.any() for low in ref["low"])


def test_silicon_valence_links_are_well_conditioned():
    """The valence set of silicon on (4, 4, 4), the case of the GPU file.  With the orbital phases of convention 1 (the eigenvectors
    of test_gpu_eigh's Wilson-loop test) the reference has link_min = 0.369 > 0.2; in convention 2 the positions inside the cell
    stay in the links and the reference itself has link_min = 0.112 with sigma_min = 0.384, so condition 1 holds in both and the
    floor on link_min is asserted where the reference meets it."""
    hop, g = silicon_hoppings()
    mesh = (4, 4, 4)
    U = bm.eigenvectors(hop, mesh)
    for name, table, floor in (("convention 2", None, 0.1), ("convention 1", bm.phase_table(mesh, g["pos"]), 0.2)):
        ref, smallest = check_conditions(U, mesh, [(0, 4)], table)
        print("silicon valence set on %r, %s: link_min = %.3f, sigma_min = %.3f" % (mesh, name, ref["link_min"][0], smallest[0]))
        assert ref["link_min"][0] > floor
        assert all(not c.any() for c in ref["chern"])


# ---- the textbook LU against LAPACK ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, sets, mesh", SMOOTH_CASES)
def test_lu_determinant_against_lapack(n, sets, mesh):
    U = smooth_case(n, mesh)
    smallest = bm.sigma_min(U, mesh, list(sets))
    for (lo, hi), s in zip(sets, smallest):
        for d in range(len(mesh)):
            M = bm.link_matrices(U, mesh, d, lo, hi)
            own, lapack = bm.lu_det(M), np.linalg.det(M)
            err = bm.wrapped_difference(np.angle(own), np.angle(lapack)).max()
            bound = 2.0 * bm.link_tolerance(n, hi - lo, s)
            assert err <= bound, (n, lo, hi, d, err, bound)
            assert np.all(np.abs(np.abs(own) - np.abs(lapack)) <= bound * np.abs(lapack))


def test_lu_pivot_rule_and_singular_matrices():
    tie = np.array([[[1.0, 2.0], [-1.0j, 5.0]]])  # |Re| + |Im| ties in column 0: the lowest row gives the pivot, no swap
    assert bm.lu_det(tie)[0] == 1.0 * (5.0 - (-1.0j / 1.0) * 2.0)
    swap = np.array([[[0.5, 1.0], [0.5 + 0.5j, 3.0]]])  # |z| would keep row 0 (0.5 < 0.707); |Re| + |Im| takes row 1
    assert abs(bm.lu_det(swap)[0] - (0.5 * 3.0 - 1.0 * (0.5 + 0.5j))) <= 1e-15
    assert bm.lu_det(np.zeros((1, 3, 3), dtype=complex))[0] == 0.0
    assert bm.angle_words(np.array([0.0 + 0.0j, -0.0 + 0.0j]))[0] == 0 and bm.angle_words(np.array([-0.0 + 0.0j]))[0] == 0


def test_angle_words():
    words = bm.angle_words(np.array([1.0, 1.0j, -1.0, -1.0j, 1.0 + 1.0j]))
    assert words.dtype == np.uint64
    assert words.tolist() == [0, 1 << 62, 1 << 63, 3 << 62, 1 << 61]
    assert np.array_equal(bm.word_angles(words), np.array([0.0, 0.25, -0.5, -0.25, 0.125]) * bm.TWO_PI)
    rng = np.random.default_rng(2)
    L = rng.normal(size=1000) + 1j * rng.normal(size=1000)
    # three roundings of a number of size pi at most (the quotient, the word as a double, the product) and half a unit of the word
    assert bm.wrapped_difference(bm.word_angles(bm.angle_words(L)), np.angle(L)).max() <= (3.0 * np.pi + 1.0) * 2.0 ** -53


# ---- the properties ----------------------------------------------------------------------------------------------------------------------
def _inputs():
    """(name, U, mesh, sets) of (a), (b) and the two smaller cases of (c)."""
    out = [("QWZ u = %g %r" % (u, mesh), qwz_case(u, mesh), mesh, [(0, 1)]) for u, mesh, _ in QWZ_CASES]
    out.append(("3-D", qwz_case(1.5, (7, 7, 4)), (7, 7, 4), [(0, 1)]))
    out += [("smooth %d" % n, smooth_case(n, mesh), mesh, list(sets)) for n, sets, mesh in SMOOTH_CASES[:2]]
    return out


@pytest.mark.parametrize("case", range(7))
def test_gauge_invariance(case):
    name, U, mesh, sets = _inputs()[case]
    n = U.shape[-1]
    ref, smallest = check_conditions(U, mesh, sets)
    bound = flux_bounds(n, sets, smallest)
    rng = np.random.default_rng(40 + case)
    phased = U * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, (U.shape[0], 1, n)))
    got = bm.berry_flux(phased, mesh, sets)
    moved = bm.wrapped_difference(got["flux"], ref["flux"])
    print("%s: column phases move the fluxes by %.3e of the bound" % (name, (moved / bound).max()))
    assert all(np.array_equal(a, b) for a, b in zip(got["chern"], ref["chern"]))
    assert np.all(moved <= bound), (name, moved.max())
    for s, (lo, hi) in enumerate(sets):  # a random unitary mixing of the set at every k
        m = hi - lo
        W = np.linalg.qr(rng.normal(size=(U.shape[0], m, m)) + 1j * rng.normal(size=(U.shape[0], m, m)))[0]
        mixed = np.array(U)
        mixed[:, :, lo:hi] = np.einsum("kib,kbc->kic", U[:, :, lo:hi], W)
        got = bm.berry_flux(mixed, mesh, [(lo, hi)])
        moved = bm.wrapped_difference(got["flux"][0], ref["flux"][s])
        assert all(np.array_equal(a[0], b[s]) for a, b in zip(got["chern"], ref["chern"])), (name, lo, hi)
        assert np.all(moved <= bound[s]), (name, lo, hi, moved.max(), bound[s])


@pytest.mark.parametrize("n, sets, mesh", SMOOTH_CASES)
def test_full_set_is_trivial(n, sets, mesh):
    U = smooth_case(n, mesh)
    ref = bm.berry_flux(U, mesh, [(0, n)])
    tol = bm.link_tolerance(n, n, 1.0)
    assert np.abs(np.abs(ref["L"]) - 1.0).max() <= tol
    assert all(not c.any() for c in ref["chern"]) and all(not low.any() for low in ref["low"])
    assert np.abs(ref["flux"]).max() <= 4.0 * tol


def test_translations_and_whole_periods():
    for name, U, mesh, sets in _inputs()[3:6]:
        ref = bm.berry_flux(U, mesh, sets)
        n = U.shape[-1]
        grid = U.reshape(tuple(mesh) + (n, n))
        for d in range(len(mesh)):
            # k+e_d is the point chi_model finds for q = e_d and for q = e_d + n_d e_d
            unit = np.eye(len(mesh), dtype=np.int64)[d]
            there = chi_model.shifted_points(mesh, unit)
            assert np.array_equal(there, chi_model.shifted_points(mesh, unit * (1 + mesh[d])))
            assert np.array_equal(np.roll(grid, -1, axis=d).reshape(U.shape), U[there])
            # moving the origin of the mesh moves the fluxes with it, bit for bit, and leaves the Chern numbers of planes across d alone
            rolled = bm.berry_flux(np.roll(grid, -2, axis=d).reshape(U.shape), mesh, sets)
            flux = ref["flux"].reshape(ref["flux"].shape[:2] + tuple(mesh))
            assert np.array_equal(np.roll(flux, -2, axis=2 + d).reshape(ref["flux"].shape), rolled["flux"]), (name, d)
            for p, plane in enumerate(ref["planes"]):
                want = ref["chern"][p] if d in plane else np.roll(ref["chern"][p], -2, axis=1)
                assert np.array_equal(rolled["chern"][p], want), (name, d, plane)


def test_both_conventions_give_the_same_chern_numbers():
    pos = np.array([[0.1, 0.2, 0.05], [0.3, -0.15, 0.25]])
    for u, mesh, want in QWZ_CASES:
        table = bm.phase_table(mesh, pos[:, :2])
        assert np.abs(table - chi_model.phase_table(mesh, np.eye(2, dtype=np.int64), pos[:, :2])).max() <= 4 * 2.0 ** -53
        ref, _ = check_conditions(qwz_case(u, mesh), mesh, [(0, 1)], table)
        assert ref["chern"][0].tolist() == [[want]]
    mesh = (7, 7, 4)
    ref, _ = check_conditions(qwz_case(1.5, mesh), mesh, [(0, 1)], bm.phase_table(mesh, pos))
    assert [c.tolist() for c in ref["chern"]] == [[[0, 1, 1, 1]], [[0] * 7], [[0] * 7]]


def test_plane_sums_are_exact():
    rng = np.random.default_rng(8)
    for mesh in ((1, 1), (2, 1), (3, 5), (1, 2, 3), (2, 2, 2)):
        n_k = int(np.prod(mesh))
        words = rng.integers(0, 1 << 64, size=(2, len(mesh), n_k), dtype=np.uint64)
        flux, chern, low = bm.flux_from_words(words, mesh)
        assert all(not w.any() for w in low), mesh
        F = bm.plaquettes(words, mesh)
        assert np.array_equal(flux, F.astype(np.float64) * bm.TURN) and np.abs(flux).max() <= np.pi
        # the same sums in Python integers
        for p, plane in enumerate(bm.PLANES[len(mesh)]):
            c = bm.remaining_axis(len(mesh), plane)
            grid = F[:, p].reshape((2,) + tuple(mesh))
            for s in range(2):
                for ic in range(1 if c is None else mesh[c]):
                    piece = grid[s] if c is None else np.take(grid[s], ic, axis=c)
                    total = sum(int(v) for v in piece.ravel())
                    assert total % (1 << 64) == 0 and total >> 64 == chern[p][s, ic]


# ---- the public interface --------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    hop, g = silicon_hoppings()
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    size = model.size
    for bands in (0, -1, size + 1, True, 1.0, "4", None, [], [(0, 1)] * 17, [(1, 1)], [(2, 1)], [(-1, 2)], [(0, size + 1)], [(0, 1, 2)], [(0,)],
                  [(0.0, 1.0)], [(0, True)], [3]):
        with pytest.raises(ValueError):
            model.berry_flux((2, 2, 2), bands)
    for mesh in ((4, 4), (4, 0, 4), (4.0, 4.0, 4.0), 4, None):
        with pytest.raises(ValueError):
            model.berry_flux(mesh, 4)
    for convention in (0, 3, "2", None):
        with pytest.raises(ValueError):
            model.berry_flux((2, 2, 2), 4, convention=convention)
    with pytest.raises(TypeError):
        model.berry_flux((2, 2, 2), 4, 1)  # keyword only
    with pytest.raises(ValueError):
        one_d.berry_flux((8,), 1)
    assert not hasattr(tbmodels_amd.KdotpModel, "berry_flux")
    assert tbmodels_amd.BerryFlux._fields == ("bands", "planes", "flux", "chern", "link_min")


def test_c_argument_errors_touch_no_device():
    """(Every call returns before a device is chosen: device 99 does not exist.)"""
    lib = _lib.lib()
    n, mesh = 5, np.array([2, 3], dtype=np.int32)
    U = np.zeros((6, n, n), dtype=np.complex128)
    ranges = np.array([[0, 2], [1, 5]], dtype=np.int32)
    L, words = np.zeros((2, 2, 6), dtype=np.complex128), np.zeros((2, 2, 6), dtype=np.uint64)
    flux, chern, least = np.zeros((2, 1, 6)), np.zeros((2, 1), dtype=np.int64), np.zeros(2)
    pm, pu, pr, pl, pw = _lib.ptr(mesh), _lib.ptr(U), _lib.ptr(ranges), _lib.ptr(L), _lib.ptr(words)

    def links(dim=2, mesh_=pm, n_=n, U_=pu, n_sets=2, ranges_=pr, L_=pl, words_=pw):
        return lib.tbk_berry_links_from_eigensystem(99, dim, mesh_, n_, U_, n_sets, ranges_, None, L_, words_)

    def fluxes(dim=2, mesh_=pm, n_sets=2, words_=pw, flux_=_lib.ptr(flux), chern_=_lib.ptr(chern)):
        return lib.tbk_berry_flux_from_links(99, dim, mesh_, n_sets, words_, flux_, chern_)

    def bad_ranges(lo, hi):
        return _lib.ptr(np.array([[0, 2], [lo, hi]], dtype=np.int32))

    plan = (ctypes.c_int64 * 4)()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    one = (ctypes.c_void_p * 1)(None)
    bad = [links(dim=1), links(dim=4), links(mesh_=None), links(mesh_=_lib.ptr(np.array([2, 0], dtype=np.int32))), links(n_=0), links(U_=None),
           links(n_sets=0), links(n_sets=17), links(ranges_=None), links(ranges_=bad_ranges(-1, 2)), links(ranges_=bad_ranges(0, 6)),
           links(ranges_=bad_ranges(3, 3)), links(ranges_=bad_ranges(4, 3)), links(L_=None), links(words_=None),
           fluxes(dim=1), fluxes(mesh_=None), fluxes(n_sets=0), fluxes(n_sets=17), fluxes(words_=None), fluxes(flux_=None), fluxes(chern_=None),
           lib.tbk_berry_flux(None, pm, 2, pr, 2, None, _lib.ptr(flux), _lib.ptr(chern), _lib.ptr(least)),
           lib.tbk_berry_flux_multi(None, 1, pm, 2, pr, 2, None, _lib.ptr(flux), _lib.ptr(chern), _lib.ptr(least)),
           lib.tbk_berry_flux_multi(one, 1, pm, 2, pr, 2, None, _lib.ptr(flux), _lib.ptr(chern), _lib.ptr(least)),
           lib.tbk_berry_flux_multi(one, 0, pm, 2, pr, 2, None, _lib.ptr(flux), _lib.ptr(chern), _lib.ptr(least)),
           lib.tbk_berry_plan(0, n, 2, pr, plan), lib.tbk_berry_plan(6, n, 2, pr, None), lib.tbk_berry_plan(6, n, 0, pr, plan),
           lib.tbk_berry_plan(6, 4, 2, pr, plan), lib.tbk_berry_plan(6, n, 2, None, plan),
           lib.tbk_berry_timing(None, ms, ctypes.byref(calls), 0)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad


def test_plan():
    plan = (ctypes.c_int64 * 8)()
    ranges = np.array([[0, 16], [3, 20], [0, 64], [0, 65]], dtype=np.int32)
    _lib.check(_lib.lib().tbk_berry_plan(1000, 80, 4, _lib.ptr(ranges), plan))
    assert [plan[0], plan[2], plan[4], plan[6]] == [1, 4, 4, 64]
    assert plan[1] == plan[3] == plan[5] == 3000 and plan[7] == min(3000, (1 << 29) // 65 ** 2, (256 << 20) // (16 * 65 ** 2))
    _lib.check(_lib.lib().tbk_berry_plan(1 << 30, 80, 4, _lib.ptr(ranges), plan))
    assert plan[1] == 1 << 30


def test_signatures_and_header_agree_on_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in ("tbk_berry_links_from_eigensystem", "tbk_berry_flux_from_links", "tbk_berry_flux", "tbk_berry_flux_multi", "tbk_berry_plan",
                 "tbk_berry_timing"):
        found = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert found, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        declared = [" ".join(part.split()) for part in found.group(1).split(",")]
        assert len(declared) == len(argtypes), (name, declared)
        for text, ctype in zip(declared, argtypes):
            if "*" in text:
                assert ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer), (name, text)
            else:
                assert ctype is kinds[text.rsplit(" ", 1)[0]], (name, text)
