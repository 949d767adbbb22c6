"""
The link and plaquette kernels (csrc/tbk_berry.hip) against tools/berry_model.py on identical eigenvectors, and `Model.berry_flux`
against its Chern numbers, its properties and the model fed with the eigenvectors `Model.eigh` returns for the same mesh.

Bound: berry_model.link_tolerance per link angle, from the number formats, the sizes and the smallest singular value
of the reference's own M; nothing measured on the kernels enters it.  A GPU link is compared with the reference link as a wrapped
difference of angles within twice the bound (one share for each side), a flux within four links' worth.  Everything behind the angle
words is integer arithmetic and is compared bit for bit.  Every case prints its measured maximum.
"""

import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import berry_model as bm  # noqa: E402  pylint: disable=wrong-import-position
from test_berry_model import PHASE_SPREAD, QWZ_CASES, SMOOTH_CASES, check_conditions, smooth_case  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu


def _links(mesh, U, sets, phases=None):
    n = U.shape[-1]
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    ranges = np.ascontiguousarray(np.array(sets, dtype=np.int32).reshape(-1, 2))
    n_k = int(np.prod(mesh))
    L = np.full((len(sets), len(mesh), n_k), np.nan, dtype=np.complex128)
    words = np.zeros((len(sets), len(mesh), n_k), dtype=np.uint64)
    _lib.check(_lib.lib().tbk_berry_links_from_eigensystem(0, len(mesh), _lib.ptr(mesh32), n, _lib.ptr(U), len(sets), _lib.ptr(ranges),
                                                           _lib.ptr(phases), _lib.ptr(L), _lib.ptr(words)))
    return L, words


def _fluxes(mesh, words):
    mesh32 = np.ascontiguousarray(mesh, dtype=np.int32)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    n_sets, n_k = words.shape[0], int(np.prod(mesh))
    planes = bm.PLANES[len(mesh)]
    counts = [1 if bm.remaining_axis(len(mesh), p) is None else mesh[bm.remaining_axis(len(mesh), p)] for p in planes]
    flux = np.full((n_sets, len(planes), n_k), np.nan)
    chern = np.full((n_sets, sum(counts)), -99, dtype=np.int64)
    _lib.check(_lib.lib().tbk_berry_flux_from_links(0, len(mesh), _lib.ptr(mesh32), n_sets, _lib.ptr(words), _lib.ptr(flux), _lib.ptr(chern)))
    return flux, chern


def _plan(n_k, n, sets):
    out = (ctypes.c_int64 * (2 * len(sets)))()
    ranges = np.ascontiguousarray(np.array(sets, dtype=np.int32).reshape(-1, 2))
    _lib.check(_lib.lib().tbk_berry_plan(n_k, n, len(sets), _lib.ptr(ranges), out))
    return [out[2 * s] for s in range(len(sets))]


def _flux_bound(n, sets, smallest):
    """Four links' worth, a link's worth being twice the tolerance (one share for each side); broadcasts over [S][P][...]."""
    return np.array([4.0 * 2.0 * bm.link_tolerance(n, hi - lo, s) for (lo, hi), s in zip(sets, smallest)])


# ---- 1. the link kernels against the model on the same U ------------------------------------------------------------------------------
@pytest.mark.parametrize("n, sets, mesh, templates", [case + (t,) for case, t in zip(SMOOTH_CASES, ([1, 1, 1], [1, 1, 4], [4, 4, 4], [64, 64]))])
@pytest.mark.parametrize("with_phases", [False, True])
def test_links_match_the_model(n, sets, mesh, templates, with_phases):
    U, sets = smooth_case(n, mesh), list(sets)
    assert _plan(int(np.prod(mesh)), n, sets) == templates
    phases = bm.random_phases(len(mesh), n, PHASE_SPREAD, 5 + n) if with_phases else None
    ref, smallest = check_conditions(U, mesh, sets, phases)
    L, words = _links(mesh, U, sets, phases)
    for s, (lo, hi) in enumerate(sets):
        bound = 2.0 * bm.link_tolerance(n, hi - lo, smallest[s])
        err = bm.wrapped_difference(np.angle(L[s]), np.angle(ref["L"][s])).max()
        err_w = bm.wrapped_difference(bm.word_angles(words[s]), np.angle(ref["L"][s])).max()
        err_abs = (np.abs(np.abs(L[s]) - np.abs(ref["L"][s])) / np.abs(ref["L"][s])).max()
        print("n = %d set (%d, %d) template %d%s: angle %.3e, word %.3e, |L| %.3e (bound %.3e)"
              % (n, lo, hi, templates[s], " with phases" if with_phases else "", err, err_w, err_abs, bound))
        assert np.all(np.isfinite(L[s].view(np.float64)))
        assert err <= bound and err_w <= bound and err_abs <= bound, (n, lo, hi, err, err_w, err_abs, bound)


# ---- 2. the plaquette kernel is the model's integer arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(1, 1), (1, 4), (2, 5), (4, 5), (2, 1, 3), (3, 2, 2), (1, 1, 2), (3, 4, 2)])
def test_fluxes_and_chern_numbers_are_exact(mesh):
    sets = [(0, 1), (1, 4), (0, 5)]
    _, words = _links(mesh, smooth_case(5, mesh), sets)
    rng = np.random.default_rng(11)
    for given in (words, rng.integers(0, 1 << 64, size=words.shape, dtype=np.uint64)):
        flux, chern = _fluxes(mesh, given)
        want_flux, want_chern, low = bm.flux_from_words(given, mesh)
        assert all(not w.any() for w in low)
        assert np.array_equal(flux, want_flux), mesh
        assert np.array_equal(chern, bm.chern_flat(want_chern)), mesh


# ---- 3. identities of bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, mesh, first, others", [(17, (3, 4, 2), [(0, 16), (3, 4), (0, 17)], [(2, 9), (0, 17), (0, 1)]),
                                                    (80, (2, 3), [(0, 65), (0, 80), (10, 27)], [(0, 64), (5, 6)])])
def test_bits_of_a_set_do_not_depend_on_the_call(n, mesh, first, others):
    U = smooth_case(n, mesh)
    L, words = _links(mesh, U, first)
    again = _links(mesh, U, first)
    assert np.array_equal(L.view(np.float64), again[0].view(np.float64)) and np.array_equal(words, again[1]), "two calls differ"
    for s, pair in enumerate(first):
        alone = _links(mesh, U, [pair])
        assert np.array_equal(alone[0][0].view(np.float64), L[s].view(np.float64)) and np.array_equal(alone[1][0], words[s]), ("alone", pair)
        mixed = _links(mesh, U, others[:1] + [pair] + others[1:] + [pair])
        for place in (1, len(others) + 1):  # among other sets, in another place, and its duplicate
            assert np.array_equal(mixed[0][place].view(np.float64), L[s].view(np.float64)), ("among others", pair, place)
            assert np.array_equal(mixed[1][place], words[s]), ("among others", pair, place)
    order = [2, 0, 1]
    moved = _links(mesh, U, [first[i] for i in order])
    assert np.array_equal(moved[1], words[order]) and np.array_equal(moved[0].view(np.float64), L[order].view(np.float64)), "the order changed bits"


# ---- 4. the whole call on the Qi-Wu-Zhang model ---------------------------------------------------------------------------------------
def _qwz_model(u, dim):
    pos = [[0.1, 0.2, 0.05][:dim], [0.3, -0.15, 0.25][:dim]]
    return tbmodels_amd.Model(hop=bm.qwz_hoppings(u, dim), size=2, dim=dim, pos=pos, contains_cc=False)


def _against_eigh(model, mesh, bands, got, convention=2):
    """The fluxes of a whole call against the model on Model.eigh's eigenvectors for the same mesh; returns the reference."""
    U = np.ascontiguousarray(model.eigh(bm.mesh_points(mesh), convention=2)[1])
    sets = [tuple(int(x) for x in pair) for pair in got.bands]
    phases = bm.phase_table(mesh, np.asarray(model.pos)) if convention == 1 else None
    ref, smallest = check_conditions(U, mesh, sets, phases)
    bound = _flux_bound(model.size, sets, smallest)
    flux = got.flux.reshape(len(sets), len(got.planes), -1)
    err = bm.wrapped_difference(flux, ref["flux"])
    print("%r bands %r convention %d: flux error %.3e (bound %.3e), link_min %s" % (mesh, bands, convention, err.max(), bound.min(), got.link_min))
    assert np.all(err <= bound[:, None, None]), (mesh, err.max(), bound)
    assert np.all(np.abs(got.link_min - ref["link_min"]) <= bound * ref["link_min"])
    assert all(np.array_equal(a, b) for a, b in zip(got.chern, ref["chern"]))
    return ref


@pytest.mark.parametrize("u, mesh, want", QWZ_CASES)
def test_qwz_chern_numbers(u, mesh, want):
    model = _qwz_model(u, 2)
    got = model.berry_flux(mesh, [(0, 1), (1, 2), (0, 2)])
    assert got.planes == ((0, 1),) and got.flux.shape == (3, 1) + tuple(mesh) and got.link_min.shape == (3,)
    assert got.chern[0].dtype == np.int64 and got.chern[0].tolist() == [[want], [-want], [0]]
    _against_eigh(model, mesh, "lower, upper, both", got)
    assert model.berry_flux(mesh, 1).chern[0].tolist() == [[want]]
    one = model.berry_flux(mesh, 1, convention=1)
    assert one.chern[0].tolist() == [[want]]
    _against_eigh(model, mesh, 1, one, convention=1)


def test_weyl_pair_in_three_dimensions():
    mesh = (7, 7, 4)
    model = _qwz_model(1.5, 3)
    for convention in (2, 1):
        got = model.berry_flux(mesh, 1, convention=convention)
        assert got.planes == ((0, 1), (0, 2), (1, 2)) and got.flux.shape == (1, 3) + mesh
        assert [c.tolist() for c in got.chern] == [[[0, 1, 1, 1]], [[0] * 7], [[0] * 7]]
        _against_eigh(model, mesh, 1, got, convention=convention)


# ---- 5. silicon ------------------------------------------------------------------------------------------------------------------------
def _silicon():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])


def test_silicon_valence_bands_are_trivial():
    """(link_min > 0.2 holds for the eigenvectors of the Wilson-loop test, convention 1; in convention 2 the reference itself has
    0.112: tests/test_berry_model.py test_silicon_valence_links_are_well_conditioned.)"""
    model, mesh = _silicon(), (4, 4, 4)
    for convention, floor in ((2, 0.1), (1, 0.2)):
        got = model.berry_flux(mesh, 4, convention=convention)
        assert all(not c.any() for c in got.chern) and [c.shape for c in got.chern] == [(1, 4)] * 3
        assert got.link_min[0] > floor, (convention, got.link_min)
        _against_eigh(model, mesh, 4, got, convention=convention)


# ---- 6. devices, 7. timing ---------------------------------------------------------------------------------------------------------------
def test_two_handles_change_no_bit():
    for model, mesh, bands in ((_silicon(), (3, 4, 2), [(0, 4), (4, 8), (1, 3)]), (_qwz_model(1.0, 2), (5, 7), 1)):
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        for convention in (2, 1):
            one = model.berry_flux(mesh, bands, convention=convention)
            two = twin.berry_flux(mesh, bands, convention=convention)
            assert len(twin._handles) == 2
            assert np.array_equal(one.flux, two.flux) and np.array_equal(one.link_min, two.link_min)
            assert all(np.array_equal(a, b) for a, b in zip(one.chern, two.chern))
            again = model.berry_flux(mesh, bands, convention=convention)
            assert np.array_equal(one.flux, again.flux) and np.array_equal(one.link_min, again.link_min)


def test_calls_are_counted_and_timed_only_when_asked():
    model = _silicon()
    model.berry_flux((4, 4, 4), 4)  # TBK_OPT_TIMING is off
    ms, calls = (ctypes.c_double * 3)(-1.0, -1.0, -1.0), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_berry_timing(model._staged(), ms, ctypes.byref(calls), 0))
    assert calls.value == 1 and list(ms) == [0.0, 0.0, 0.0]
    model.set_option(_lib.TBK_OPT_TIMING, 1)
    model.set_option(_lib.TBK_OPT_K_CHUNK, 24)
    timed = model.berry_flux((4, 4, 4), 4)
    _lib.check(_lib.lib().tbk_berry_timing(model._staged(), ms, ctypes.byref(calls), 1))
    print("silicon (4, 4, 4), valence set: %d calls, links %.3f ms, library LU %.3f ms, fluxes %.3f ms" % (calls.value, ms[0], ms[1], ms[2]))
    assert calls.value == 2 and ms[0] > 0.0 and ms[1] == 0.0 and ms[2] > 0.0
    model.set_option(_lib.TBK_OPT_K_CHUNK, 0)
    assert np.array_equal(timed.flux, model.berry_flux((4, 4, 4), 4).flux)  # the chunk changes no bit
    _lib.check(_lib.lib().tbk_berry_timing(model._staged(), ms, ctypes.byref(calls), 1))
    assert calls.value == 1 and min(ms) >= 0.0


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------
def test_c_argument_errors():
    lib = _lib.lib()
    model = _silicon()
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    mesh, zero = np.array([2, 3, 2], dtype=np.int32), np.array([2, 0, 2], dtype=np.int32)
    ranges, wrong = np.array([[0, 4], [4, 8]], dtype=np.int32), np.array([[0, 4], [4, 9]], dtype=np.int32)
    pos = np.ascontiguousarray(model.pos, dtype=np.float64)
    flux, chern, least = np.zeros((2, 3, 12)), np.zeros((2, 7), dtype=np.int64), np.zeros(2)
    pm, pr, pp, pf, pc, pl = _lib.ptr(mesh), _lib.ptr(ranges), _lib.ptr(pos), _lib.ptr(flux), _lib.ptr(chern), _lib.ptr(least)

    def whole(handle_=handle, mesh_=pm, n_sets=2, ranges_=pr, convention=2, pos_=pp, flux_=pf, chern_=pc, least_=pl):
        return lib.tbk_berry_flux(handle_, mesh_, n_sets, ranges_, convention, pos_, flux_, chern_, least_)

    assert whole() == _lib.TBK_OK and whole(convention=1) == _lib.TBK_OK and whole(pos_=None) == _lib.TBK_OK
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    bad = [whole(handle_=None), whole(mesh_=None), whole(mesh_=_lib.ptr(zero)), whole(n_sets=0), whole(n_sets=17), whole(ranges_=None),
           whole(ranges_=_lib.ptr(wrong)), whole(convention=0), whole(convention=3), whole(convention=1, pos_=None), whole(flux_=None),
           whole(chern_=None), whole(least_=None), lib.tbk_berry_flux_multi(twice, 2, pm, 2, pr, 2, pp, pf, pc, pl),
           lib.tbk_berry_timing(handle, None, ctypes.byref(calls), 0), lib.tbk_berry_timing(handle, ms, None, 0)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
