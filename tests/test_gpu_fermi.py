"""
The probe, band-edge and Fermi-level kernels (csrc/tbk_fermi.hip) against the exact statement tools/fermi_model.py, whose N_exact is
that of tools/tetra_exact.py, and `Model.band_edges` / `Model.fermi_level` against the same model fed with `eigenval_array`.

Inputs: `tetra_exact.tie_rich_inputs` (five dyadic levels, 30 % of the eigenvalues one ulp up, rows sorted) and plain seeded random
rows sorted ascending, on the meshes 2 x 3 x 2, 4 x 4 x 4, 1 x 5 and 3 x 4 with 1, 3, 8 and 65 orbitals (65: a cell's bands cross a
wave; 2 x 3 x 2 x 65 and 3 x 4 x 65 are 780 items, four workgroups, so the row reduction runs).

Bounds.  Kernel against exact: 1e-11 n_orb, the accumulate-stage bound of DESIGN 10.5 (fixed-point worst case 4.5e-13 n_orb).  Probe
against the grid kernel: n_orb 2^-40, two fixed-point bounds.  The search contract: with p the double in front of mu,
N_exact(mu) >= n - bound and N_exact(p) <= n + bound -- the kernel's Q crosses the target between p and mu, and Q is N_exact to
within the bound; bound = 1e-11 n_orb for the kernels on given eigenvalues and 1e-9 n_orb for the whole call, where
N_exact is evaluated on `eigenval_array` of the same mesh.  Every case prints its measured maxima.
"""

import ctypes
import os
import pickle
import sys
from fractions import Fraction

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dos_model  # noqa: E402  pylint: disable=wrong-import-position
import fermi_model  # noqa: E402  pylint: disable=wrong-import-position
import tetra_exact as exact  # noqa: E402  pylint: disable=wrong-import-position

pytestmark = pytest.mark.gpu

# (kind, mesh, n_orb, probes of section 1)
CASES = [
    ("ties", (2, 3, 2), 3, 15), ("ties", (4, 4, 4), 1, 33), ("ties", (1, 5), 8, 16), ("ties", (3, 4), 3, 17),
    ("random", (2, 3, 2), 65, 17), ("random", (3, 4), 65, 33), ("random", (4, 4, 4), 8, 16), ("random", (1, 5), 1, 1),
    ("random", (3, 4), 8, 15),
]
_CACHE = {}


def _eig(kind, mesh, n_orb):
    key = ("eig", kind, mesh, n_orb)
    if key not in _CACHE:
        if kind == "ties":
            eig = exact.tie_rich_inputs(mesh, n_orb, 1)[0]
        else:
            rng = np.random.default_rng(7000 + 100 * len(mesh) + 10 * int(np.prod(mesh)) + n_orb)
            eig = np.sort(rng.uniform(-1.0, 1.0, tuple(mesh) + (n_orb,)), axis=-1)
        eig = np.ascontiguousarray(eig, dtype=np.float64)
        eig.setflags(write=False)
        _CACHE[key] = eig
    return _CACHE[key]


def _simplices(eig):
    key = ("simplices", eig.tobytes(), eig.shape)
    if key not in _CACHE:
        _CACHE[key] = fermi_model.sorted_simplices(eig)
    return _CACHE[key]


def _exact(eig, energy):
    """N_exact(energy) as a Fraction (computed once per (inputs, energy))."""
    key = ("nos", eig.tobytes(), eig.shape, float(energy))
    if key not in _CACHE:
        _CACHE[key] = fermi_model.nos_exact(eig, energy, _simplices(eig))
    return _CACHE[key]


def _mesh32(eig):
    return np.ascontiguousarray(eig.shape[:-1], dtype=np.int32)


def _nos_at(eig, energies):
    mesh, flat = _mesh32(eig), np.ascontiguousarray(eig, dtype=np.float64)
    energies = np.ascontiguousarray(energies, dtype=np.float64)
    out = np.full(len(energies), np.nan)
    _lib.check(_lib.lib().tbk_nos_at_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), _lib.ptr(energies),
                                                      len(energies), _lib.ptr(out)))
    return out


def _edges(eig):
    mesh, flat = _mesh32(eig), np.ascontiguousarray(eig, dtype=np.float64)
    emin, emax = np.full(eig.shape[-1], np.nan), np.full(eig.shape[-1], np.nan)
    _lib.check(_lib.lib().tbk_band_edges_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), _lib.ptr(emin),
                                                          _lib.ptr(emax)))
    return emin, emax


def _fermi(eig, n):
    """(mu, lower, upper, nos, passes)"""
    mesh, flat = _mesh32(eig), np.ascontiguousarray(eig, dtype=np.float64)
    out, passes = np.full(4, np.nan), ctypes.c_int32(-1)
    _lib.check(_lib.lib().tbk_fermi_from_eigenvalues(0, len(mesh), _lib.ptr(mesh), eig.shape[-1], _lib.ptr(flat), float(n), _lib.ptr(out),
                                                     ctypes.byref(passes)))
    return float(out[0]), float(out[1]), float(out[2]), float(out[3]), passes.value


def _contract(eig, mu, n, bound, label):
    """N_exact(mu) >= n - bound and N_exact(nextafter(mu, -inf)) <= n + bound; prints both margins."""
    below = np.nextafter(mu, -np.inf)
    at, under = float(_exact(eig, mu) - Fraction(n)), float(_exact(eig, below) - Fraction(n))
    print("%s n = %.17g: mu = %.17g, N_exact(mu) - n = %.3e, N_exact(mu-) - n = %.3e" % (label, n, mu, at, under))
    assert at >= -bound and under <= bound, (label, n, mu, at, under)


def _fillings(n_orb):
    third = n_orb / 3.0
    return [0.5, third if third != int(third) else third + 0.1, n_orb - 0.25]


def _probes(eig, count, seed):
    """Energies on corners, below the spectrum, above it and in between: shuffled, then ascending inside every chunk of 16."""
    rng = np.random.default_rng(seed)
    lo, hi = eig.min(), eig.max()
    special = [lo - 0.5, np.nextafter(lo, -np.inf), hi + 0.5, lo, hi]
    corners = list(rng.choice(eig.reshape(-1), size=max(1, count // 3)))
    free = list(rng.uniform(lo, hi, size=max(0, count - len(special) - len(corners))))
    pool = (corners + special + free) if count > 1 else [float(np.median(eig))]
    assert len(pool) == count
    rng.shuffle(pool)
    pool = np.array(pool)
    return np.concatenate([np.sort(pool[j:j + 16]) for j in range(0, count, 16)])


# ---- 1. the probe kernel against exact --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mesh, n_orb, count", CASES)
def test_probe_kernel_matches_exact(kind, mesh, n_orb, count):
    eig = _eig(kind, mesh, n_orb)
    energies = _probes(eig, count, 11)
    if count >= 15:  # the placement the case is there for
        assert np.isin(energies, eig).any() and (energies < eig.min()).any() and (energies > eig.max()).any()
    if count > 16:
        assert np.any(np.diff(energies) < 0)  # not sorted as a whole
    got = _nos_at(eig, energies)
    want = np.array([float(_exact(eig, e)) for e in energies])
    err = np.abs(got - want).max()
    print("%s %s x %d, %d probes: max|N - exact| = %.3e" % (kind, mesh, n_orb, count, err))
    assert err <= 1e-11 * n_orb, (kind, mesh, n_orb, count, err)
    assert np.all(got[energies < eig.min()] == 0.0) and np.all(got[energies >= eig.max()] == float(n_orb))


# ---- 2. the probe kernel against the grid kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mesh, n_orb", [("ties", (2, 3, 2), 3), ("ties", (3, 4), 3), ("random", (2, 3, 2), 65), ("random", (3, 4), 8)])
def test_probe_kernel_matches_the_grid_kernel_on_a_uniform_grid(kind, mesh, n_orb):
    eig = _eig(kind, mesh, n_orb)
    e_min, step, n_e = -1.125, 2.0 ** -4 + 2.0 ** -9, 37
    grid = e_min + np.arange(n_e) * step  # the grid kernel's points: two roundings
    mesh32, flat = _mesh32(eig), np.ascontiguousarray(eig)
    want = np.full(n_e, np.nan)
    _lib.check(_lib.lib().tbk_dos_from_eigenvalues(0, len(mesh), _lib.ptr(mesh32), n_orb, _lib.ptr(flat), e_min, step, n_e, _lib.ptr(want)))
    err = np.abs(_nos_at(eig, grid) - want).max()
    print("%s %s x %d: max|N(probe) - N(grid kernel)| = %.3e" % (kind, mesh, n_orb, err))
    assert err <= n_orb * 2.0 ** -40, (kind, mesh, n_orb, err)


# ---- 3. the chunking changes no bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mesh, n_orb", [("random", (2, 3, 2), 65), ("ties", (3, 4), 3)])
def test_seventeen_probes_at_once_and_one_by_one_give_the_same_bits(kind, mesh, n_orb):
    eig = _eig(kind, mesh, n_orb)
    energies = _probes(eig, 17, 13)
    together, again = _nos_at(eig, energies), _nos_at(eig, energies)
    single = np.array([_nos_at(eig, energies[j:j + 1])[0] for j in range(17)])
    assert np.array_equal(together, again) and np.array_equal(together, single)


# ---- 4. band edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mesh, n_orb", [case[:3] for case in CASES] + [("random", (1, 5), 300)])
def test_band_edges_are_the_doubles_of_the_array(kind, mesh, n_orb):
    eig = _eig(kind, mesh, n_orb)
    emin, emax = _edges(eig)
    flat = eig.reshape(-1, n_orb)
    assert np.array_equal(emin, flat.min(axis=0)) and np.array_equal(emax, flat.max(axis=0))


# ---- 5. the search contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mesh, n_orb", [case[:3] for case in CASES])
def test_search_contract(kind, mesh, n_orb):
    eig = _eig(kind, mesh, n_orb)
    emin, emax = fermi_model.band_edges(eig)
    for n in _fillings(n_orb):
        assert not (n == int(n) and emax[int(n) - 1] < emin[int(n)])  # metallic: the search runs
        mu, lower, upper, nos, passes = _fermi(eig, n)
        assert lower == upper == mu and 1 <= passes <= 16, (kind, mesh, n_orb, n, mu, lower, upper, passes)
        _contract(eig, mu, n, 1e-11 * n_orb, "%s %s x %d (%d passes)" % (kind, mesh, n_orb, passes))
        assert nos == _nos_at(eig, [mu])[0] and nos >= n - 1e-11 * n_orb


# ---- 6. the gap case ------------------------------------------------------------------------------------------------------------------------
def _gapped(mesh, touching):
    rng = np.random.default_rng(21 + len(mesh))
    lower = np.sort(rng.uniform(-1.0, -0.125, tuple(mesh) + (2,)), axis=-1)
    upper = np.sort(rng.uniform(0.375 if not touching else 0.0, 2.0, tuple(mesh) + (2,)), axis=-1)
    if touching:
        lower.reshape(-1, 2)[1, 1] = 0.0
        upper.reshape(-1, 2)[-1, 0] = 0.0
    return np.ascontiguousarray(np.concatenate([lower, upper], axis=-1))


@pytest.mark.parametrize("mesh", [(2, 3, 2), (3, 4)])
def test_gap_case_and_its_neighbours(mesh):
    eig = _gapped(mesh, touching=False)
    top, bottom = eig[..., 1].max(), eig[..., 2].min()
    assert top < bottom
    mu, lower, upper, nos, passes = _fermi(eig, 2)
    assert lower == top and upper == bottom and mu == top + (bottom - top) / 2 and passes == 0 and nos == 2.0
    assert nos == _nos_at(eig, [mu])[0]
    # half an electron less: the search, inside the band below
    mu, lower, upper, nos, passes = _fermi(eig, 1.5)
    assert lower == upper == mu and 1 <= passes <= 16 and mu < top
    _contract(eig, mu, 1.5, 1e-11 * 4, "gapped %s" % (mesh,))
    # touching bands (max == min): no gap, the search returns the touching energy within the contract
    eig = _gapped(mesh, touching=True)
    assert eig[..., 1].max() == eig[..., 2].min() == 0.0
    mu, lower, upper, nos, passes = _fermi(eig, 2)
    assert lower == upper == mu and 1 <= passes <= 16
    _contract(eig, mu, 2, 1e-11 * 4, "touching %s" % (mesh,))


# ---- 7. a flat band --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(2, 3, 2), (3, 4)])
def test_flat_band_returns_its_energy_inside_the_jump(mesh):
    rng = np.random.default_rng(31)
    flat = 0.37
    eig = np.ascontiguousarray(np.stack([rng.uniform(-1.0, 0.0, mesh), np.full(mesh, flat), rng.uniform(1.0, 2.0, mesh)], axis=-1))
    for n in (1.0625, 1.5, 1.9375, 1.0 + 2.0 ** -40, 2.0 - 2.0 ** -40):
        mu, lower, upper, nos, passes = _fermi(eig, n)
        assert mu == lower == upper == flat and nos == 2.0 and 1 <= passes <= 16, (mesh, n, mu, nos, passes)


# ---- 8. scaling and a shift ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exponent", [-100, 100])
@pytest.mark.parametrize("kind, mesh, n_orb", [("ties", (2, 3, 2), 3), ("random", (3, 4), 8)])
def test_scaling_by_a_power_of_two_scales_mu_bit_for_bit(kind, mesh, n_orb, exponent):
    eig = _eig(kind, mesh, n_orb)
    factor = 2.0 ** exponent
    for n in _fillings(n_orb):
        plain, scaled = _fermi(eig, n), _fermi(eig * factor, n)
        assert scaled[0] == plain[0] * factor and scaled[3] == plain[3] and scaled[4] == plain[4], (kind, mesh, n, plain, scaled)


@pytest.mark.parametrize("kind, mesh, n_orb", [("ties", (2, 3, 2), 3), ("random", (3, 4), 8)])
def test_shift_by_two_to_the_twenty(kind, mesh, n_orb):
    shift = 2.0 ** 20
    shifted = np.ascontiguousarray(_eig(kind, mesh, n_orb) + shift)  # one-ulp ties round onto their level: the contract is on these rows
    for n in _fillings(n_orb):
        mu, lower, upper, _, passes = _fermi(shifted, n)
        assert lower == upper == mu and 1 <= passes <= 16
        _contract(shifted, mu, n, 1e-11 * n_orb, "%s %s x %d shifted" % (kind, mesh, n_orb))
        print("    mu - 2^20 = %.17g, unshifted mu = %.17g" % (mu - shift, _fermi(_eig(kind, mesh, n_orb), n)[0]))


# ---- 9. Model.fermi_level / Model.band_edges -------------------------------------------------------------------------------------------------------
def _models():
    g = load_golden("silicon")
    yield "silicon", tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"]), (2, 3, 2), [4, 0.5, 8.0 / 3.0, 7.75]
    for dim, mesh in ((3, (2, 3, 2)), (2, (3, 4))):
        r_vec, hop, pos = syn.dense_model_arrays(9, 6, syn.MODEL_SEED + 1400 + dim, dim=dim)
        yield "dense 9 orbitals", tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos), mesh, [0.5, 3.1, 8.75, 4]


def _check_model(label, model, mesh, eig, fillings):
    n_orb, scale = model.size, np.abs(eig).max()
    edges = model.band_edges(mesh)
    want_min, want_max = fermi_model.band_edges(eig)
    err = max(np.abs(edges.emin - want_min).max(), np.abs(edges.emax - want_max).max())
    print("%s %s: max|edge - model| = %.3e (|E|max = %.3f)" % (label, mesh, err, scale))
    assert isinstance(edges, tbmodels_amd._model.BandEdges) and edges.emin.shape == edges.emax.shape == (n_orb,)
    assert err <= 1e-12 * scale, (label, mesh, err)
    for n in fillings:
        got = model.fermi_level(mesh, n)
        want_mu, want_lower, want_upper = fermi_model.fermi_level(eig, n) if n == int(n) else (None, 0.0, 0.0)
        assert isinstance(got, tbmodels_amd._model.FermiLevel) and all(isinstance(x, float) for x in got)
        if want_lower < want_upper:  # the model takes the gap: so does the call, at the same edges
            print("%s %s n = %s: gap [%.12f, %.12f], mu = %.12f" % (label, mesh, n, got.lower, got.upper, got.mu))
            assert got.lower < got.upper and got.mu == got.lower + (got.upper - got.lower) / 2 and got.nos == float(n)
            assert max(abs(got.lower - want_lower), abs(got.upper - want_upper), abs(got.mu - want_mu)) <= 1e-12 * scale
        else:
            assert got.lower == got.upper == got.mu
            _contract(eig, got.mu, n, 1e-9 * n_orb, "%s %s" % (label, mesh))
    return edges


def test_model_methods_against_the_model_of_the_same_mesh():
    gaps = 0
    for label, model, mesh, fillings in _models():
        eig = np.ascontiguousarray(np.array(model.eigenval_array(dos_model.mesh_kpoints(mesh))).reshape(tuple(mesh) + (model.size,)))
        model.set_option(_lib.TBK_OPT_TIMING, 1)
        single = _check_model(label, model, mesh, eig, fillings)
        ms, calls, passes = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().tbk_fermi_timing(model._staged_all()[0], ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(passes), 1))
        print("%s %s: %d calls, %d passes, %.3f ms of kernels" % (label, mesh, calls.value, passes.value, ms.value))
        assert calls.value == 1 + len(fillings) and 1 <= passes.value <= 16 * len(fillings) and ms.value > 0.0
        gaps += sum(1 for n in fillings if n == int(n) and fermi_model.fermi_level(eig, n)[1] < fermi_model.fermi_level(eig, n)[2])
        # two handles on one device against one: the edges to rounding, mu within the contract
        twin = pickle.loads(pickle.dumps(model))
        twin.devices = [0, 0]
        both = _check_model(label + ", two handles", twin, mesh, eig, fillings)
        assert len(twin._handles) == 2
        assert max(np.abs(both.emin - single.emin).max(), np.abs(both.emax - single.emax).max()) <= 1e-12 * np.abs(eig).max()
    print("gap cases met: %d" % gaps)


def test_untimed_calls_are_counted_without_time():
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    model.fermi_level((4, 4, 4), 4.5)  # TBK_OPT_TIMING is off
    ms, calls, passes = ctypes.c_double(-1.0), ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_fermi_timing(model._staged(), ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(passes), 0))
    assert calls.value == 1 and passes.value >= 1 and ms.value == 0.0


# ---- 10. arguments --------------------------------------------------------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    for mesh in ((4, 4), (4, 4, 4, 4), (4, 0, 4), (4, -2, 4), (4, 2.5, 4), (4.0, 4.0, 4.0), 4, (2 ** 11, 2 ** 10, 2 ** 10)):
        with pytest.raises(ValueError):
            model.fermi_level(mesh, 4)
        with pytest.raises(ValueError):
            model.band_edges(mesh)
    for n in (True, np.bool_(False), "4", None, 4 + 0j, [4], np.nan, np.inf, -np.inf, 0, 0.0, -1, 8, 8.0, 9.5):
        with pytest.raises(ValueError):
            model.fermi_level((2, 2, 2), n)
    with pytest.raises(ValueError):
        one_d.fermi_level((8,), 1)
    with pytest.raises(ValueError):
        one_d.band_edges((8,))
    assert not hasattr(tbmodels_amd.KdotpModel, "fermi_level") and not hasattr(tbmodels_amd.KdotpModel, "band_edges")


def test_c_argument_errors():
    lib = _lib.lib()
    eig = np.ascontiguousarray(_eig("random", (2, 3, 2), 65)[..., :8])
    mesh = np.array([2, 3, 2], dtype=np.int32)
    probes, out, emin, emax, four = np.array([-0.5, 0.0, 0.5]), np.zeros(3), np.zeros(8), np.zeros(8), np.zeros(4)

    def nos_at(dim=3, mesh_=mesh, n_orb=8, eig_=eig, probes_=probes, n_p=3, out_=out):
        return lib.tbk_nos_at_from_eigenvalues(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(probes_), n_p, _lib.ptr(out_))

    def edges(dim=3, mesh_=mesh, n_orb=8, eig_=eig, lo=emin, hi=emax):
        return lib.tbk_band_edges_from_eigenvalues(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), _lib.ptr(lo), _lib.ptr(hi))

    def fermi(dim=3, mesh_=mesh, n_orb=8, eig_=eig, n=3.5, out_=four):
        return lib.tbk_fermi_from_eigenvalues(0, dim, _lib.ptr(mesh_), n_orb, _lib.ptr(eig_), n, _lib.ptr(out_), None)

    assert nos_at() == edges() == fermi() == _lib.TBK_OK
    zero = np.array([2, 0, 2], dtype=np.int32)
    bad = [nos_at(dim=1), nos_at(dim=4), nos_at(mesh_=zero), nos_at(mesh_=None), nos_at(eig_=None), nos_at(probes_=None), nos_at(out_=None),
           nos_at(n_orb=0), nos_at(n_p=0), nos_at(probes_=np.array([0.0, np.nan, 0.5])), nos_at(probes_=np.array([0.0, 0.25, np.inf])),
           edges(dim=1), edges(mesh_=zero), edges(mesh_=None), edges(eig_=None), edges(lo=None), edges(hi=None), edges(n_orb=0),
           fermi(dim=4), fermi(mesh_=zero), fermi(mesh_=None), fermi(eig_=None), fermi(out_=None), fermi(n_orb=0), fermi(n=0.0), fermi(n=8.0),
           fermi(n=-1.0), fermi(n=float("nan")), fermi(n=float("inf"))]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
    # the handle entry points: NULL pointers, a handle given twice, n_electrons (a k.p model has no such method: test above)
    g = load_golden("silicon")
    model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    handle = model._staged_all()[0]
    twice = (ctypes.c_void_p * 2)(handle.value, handle.value)
    ms, calls, passes = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_int64(0)
    bad = [lib.tbk_fermi(None, _lib.ptr(mesh), 4.0, _lib.ptr(four)), lib.tbk_fermi(handle, None, 4.0, _lib.ptr(four)),
           lib.tbk_fermi(handle, _lib.ptr(mesh), 4.0, None), lib.tbk_fermi(handle, _lib.ptr(mesh), 8.0, _lib.ptr(four)),
           lib.tbk_fermi(handle, _lib.ptr(zero), 4.0, _lib.ptr(four)), lib.tbk_fermi_multi(twice, 2, _lib.ptr(mesh), 4.0, _lib.ptr(four)),
           lib.tbk_fermi_multi(None, 1, _lib.ptr(mesh), 4.0, _lib.ptr(four)),
           lib.tbk_band_edges(None, _lib.ptr(mesh), _lib.ptr(emin), _lib.ptr(emax)), lib.tbk_band_edges(handle, None, _lib.ptr(emin), _lib.ptr(emax)),
           lib.tbk_band_edges(handle, _lib.ptr(mesh), None, _lib.ptr(emax)), lib.tbk_band_edges_multi(twice, 2, _lib.ptr(mesh), _lib.ptr(emin), _lib.ptr(emax)),
           lib.tbk_fermi_timing(None, ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(passes), 0),
           lib.tbk_fermi_timing(handle, None, ctypes.byref(calls), ctypes.byref(passes), 0)]
    assert bad == [_lib.TBK_ERR_ARGUMENT] * len(bad), bad
