"""The argument checks of the tetrahedron calls (density of states, projected density of states, number of states at probe energies,
band edges, Fermi level, point weights, occupations): for every invalid input the exact status and the exact text of
``tbk_last_error()``.  Inputs with two faults pin the order of the checks: the message names the first.

Two tables of (entry point, overrides of a valid input, message), the status being ``TBK_ERR_ARGUMENT`` throughout:

* ``CASES``: the seven entry points on the caller's arrays (``tbk_*_from_eigenvalues`` / ``_from_eigensystem``).  Every one of their
  checks stands in front of the one that needs a device, so the table holds no valid input and no case needs a GPU.
* ``HANDLE_CASES`` (marked ``gpu``): the entry points on staged handles and their ``_multi`` forms.  Their checks cannot be pinned
  without a GPU: they take a ``tbk_model*``, and a handle exists only on a device.  The handles are a 2-orbital model in three
  dimensions (twice), a 3-orbital one, a 2-orbital chain, a 2-orbital k.p model and a 65-orbital model with ``TBK_EIG_WAVE`` (twice);
  the meshes of the inputs that pass are ``(2, 3, 2)``.

``tbk_dos_multi`` and ``tbk_pdos_multi`` run one host thread per handle, each on a slab of its own: with two handles their front looks
at the size of the grid (under a text of its own) and at the groups before the slabs look at anything, with one handle they are
``tbk_dos`` / ``tbk_pdos``.  ``SEVERAL`` pins that difference.
"""

import ctypes

import numpy as np
import pytest

from tbmodels_amd import _lib

nan, inf = float("nan"), float("inf")

_GRID = ["e_min", "e_step", "n_e", "out"]
_HEAD = ["device", "dim", "mesh", "n_orb"]
ENTRIES = {
    "dos": ("tbk_dos_from_eigenvalues", _HEAD + ["E"] + _GRID),
    "pdos": ("tbk_pdos_from_eigensystem", _HEAD + ["n_groups", "E", "W"] + _GRID),
    "nos_at": ("tbk_nos_at_from_eigenvalues", _HEAD + ["E", "energies", "n_p", "out"]),
    "edges": ("tbk_band_edges_from_eigenvalues", _HEAD + ["E", "emin", "emax"]),
    "fermi": ("tbk_fermi_from_eigenvalues", _HEAD + ["E", "n_electrons", "out", "passes"]),
    "weights": ("tbk_tetra_weights_from_eigenvalues", _HEAD + ["E", "energy", "out"]),
    "occ": ("tbk_occupations_from_eigensystem", _HEAD + ["E", "U", "energy", "k_chunk", "q", "f", "eb"]),
}
ARRAYS = tuple(ENTRIES)
_GROUPS = ["offsets", "orbitals", "n_groups"]
HANDLE_ENTRIES = {
    "dos": ("tbk_dos", ["handle", "mesh"] + _GRID),
    "pdos": ("tbk_pdos", ["handle", "mesh"] + _GROUPS + _GRID),
    "edges": ("tbk_band_edges", ["handle", "mesh", "emin", "emax"]),
    "fermi": ("tbk_fermi", ["handle", "mesh", "n_electrons", "out"]),
    "weights": ("tbk_tetra_weights", ["handle", "mesh", "energy", "out"]),
    "occ": ("tbk_occupations", ["handle", "mesh", "mode", "value", "mu", "q", "f", "eb"]),
}
for _key, (_name, _order) in list(HANDLE_ENTRIES.items()):
    HANDLE_ENTRIES[_key + "_multi"] = (_name + "_multi", ["handles", "n_handles"] + _order[1:])
SINGLE = ("dos", "pdos", "edges", "fermi", "weights", "occ")
MULTI = tuple(entry + "_multi" for entry in SINGLE)
BOTH = SINGLE + MULTI

# An input that passes every check (on the caller's arrays: every check but the device's); a case overrides some of it.  "buf": some
# memory that no check reads and, on handles, that is large enough for the results of a call that passes.
BASE = {"device": 0, "dim": 3, "mesh": [2, 3, 2], "n_orb": 2, "n_groups": 1, "e_min": -1.0, "e_step": 0.25, "n_e": 9, "energies": [0.1, 0.2],
        "n_p": 2, "n_electrons": 1.0, "energy": 0.25, "k_chunk": 0, "passes": None, "offsets": [0, 1], "orbitals": [0], "mode": 0, "value": 0.25,
        "handle": "two", "handles": ["two"]}
_BUF = np.zeros(256)
_INT32 = ("mesh", "offsets", "orbitals")


def _arguments(order, overrides, handles):
    values = dict({key: "buf" for key in order}, **BASE)
    values.update(overrides)
    if "n_handles" in order and "n_handles" not in overrides:
        values["n_handles"] = 0 if values["handles"] is None else len(values["handles"])
    keep = []  # the arrays stay alive until the call has returned
    args = []
    for key in order:
        value = values[key]
        if key in _INT32 + ("energies",) and value is not None:
            keep.append(np.array(value, dtype=np.int32 if key in _INT32 else np.float64))
            value = _lib.ptr(keep[-1])
        elif key == "handle":
            value = None if value is None else handles[value]
        elif key == "handles" and value is not None:
            keep.append((ctypes.c_void_p * len(value))(*[None if name is None else handles[name].value for name in value]))
            value = keep[-1]
        elif isinstance(value, str) and value == "buf":
            value = _lib.ptr(_BUF)
        args.append(value)
    return args, keep


def call(entry, overrides, table=ENTRIES, handles=None):
    """(status, tbk_last_error()) of the entry point on BASE with the overrides."""
    name, order = table[entry]
    args, keep = _arguments(order, overrides, handles)
    status = getattr(_lib.lib(), name)(*args)
    del keep
    return status, _lib.last_error()


def _each(entries, overrides, message):
    return [(entry, overrides, message) for entry in entries]


_DOS_MESH = 'invalid argument: the density of states needs a 2- or 3-dimensional mesh'
_OCC_MESH = 'invalid argument: the tetrahedron weights need a 2- or 3-dimensional mesh'
_ENTRY = 'invalid argument: a mesh entry is < 1'
_POINTS = 'invalid argument: the mesh has 2^31 points or more'
_MESH_NOS = 'invalid argument: mesh / nos is NULL'
_MESH_NULL = 'invalid argument: mesh is NULL'
_FEW = 'invalid argument: the energy grid needs at least two points'
_MANY = 'invalid argument: the energy grid has more than 2^20 points'
_STEP = 'invalid argument: the energy step must be positive and finite'
_E_MIN = 'invalid argument: e_min is not finite'
_N_ORB = 'invalid argument: n_orb < 1'
_ELECTRONS = 'invalid argument: n_electrons must lie inside (0, n_orb)'
_ENERGY = 'invalid argument: the energy is not finite'
_FERMI = ("nos_at", "edges", "fermi")
_OCC = ("weights", "occ")

# (entry, overrides of BASE, tbk_last_error())
CASES = (
    # the mesh
    _each(("dos", "pdos") + _FERMI, {'dim': 1}, _DOS_MESH)
    + _each(("dos", "pdos") + _FERMI, {'dim': 4}, _DOS_MESH)
    + _each(_OCC, {'dim': 1}, _OCC_MESH)
    + _each(_OCC, {'dim': 4}, _OCC_MESH)
    + _each(("dos", "pdos"), {'mesh': None}, _MESH_NOS)
    + _each(("dos", "pdos"), {'out': None}, _MESH_NOS)
    + _each(_FERMI + _OCC, {'mesh': None}, _MESH_NULL)
    + _each(ARRAYS, {'mesh': [2, 0, 2]}, _ENTRY)
    + _each(ARRAYS, {'mesh': [2, 3, -1]}, _ENTRY)
    + _each(ARRAYS, {'mesh': [65536, 32768, 1]}, _POINTS)
    + _each(ARRAYS, {'dim': 2, 'mesh': [65536, 65536]}, _POINTS)
    # the energy grid
    + _each(("dos", "pdos"), {'n_e': 1}, _FEW)
    + _each(("dos", "pdos"), {'n_e': (1 << 20) + 1}, _MANY)
    + _each(("dos", "pdos"), {'e_step': 0.0}, _STEP)
    + _each(("dos", "pdos"), {'e_step': -0.25}, _STEP)
    + _each(("dos", "pdos"), {'e_step': nan}, _STEP)
    + _each(("dos", "pdos"), {'e_step': inf}, _STEP)
    + _each(("dos", "pdos"), {'e_min': nan}, _E_MIN)
    + _each(("dos", "pdos"), {'e_min': -inf}, _E_MIN)
    # the caller's arrays and the sizes
    + [('dos', {'E': None}, 'invalid argument: E is NULL'),
       ('pdos', {'E': None}, 'invalid argument: E / W is NULL'),
       ('pdos', {'W': None}, 'invalid argument: E / W is NULL'),
       ('pdos', {'n_groups': 0}, 'invalid argument: n_groups outside [1, TBK_PDOS_MAX_GROUPS]'),
       ('pdos', {'n_groups': 17}, 'invalid argument: n_groups outside [1, TBK_PDOS_MAX_GROUPS]'),
       ('nos_at', {'E': None}, 'invalid argument: E / energies / nos is NULL'),
       ('nos_at', {'energies': None}, 'invalid argument: E / energies / nos is NULL'),
       ('nos_at', {'out': None}, 'invalid argument: E / energies / nos is NULL'),
       ('nos_at', {'n_p': 0}, 'invalid argument: no probe energies'),
       ('nos_at', {'energies': [0.1, nan]}, 'invalid argument: a probe energy is not finite'),
       ('nos_at', {'energies': [-inf, 0.2]}, 'invalid argument: a probe energy is not finite'),
       ('edges', {'E': None}, 'invalid argument: E / emin / emax is NULL'),
       ('edges', {'emin': None}, 'invalid argument: E / emin / emax is NULL'),
       ('edges', {'emax': None}, 'invalid argument: E / emin / emax is NULL'),
       ('fermi', {'E': None}, 'invalid argument: E / out is NULL'),
       ('fermi', {'out': None}, 'invalid argument: E / out is NULL'),
       ('fermi', {'n_electrons': 0.0}, _ELECTRONS),
       ('fermi', {'n_electrons': 2.0}, _ELECTRONS),
       ('fermi', {'n_electrons': -1.0}, _ELECTRONS),
       ('fermi', {'n_electrons': nan}, _ELECTRONS),
       ('weights', {'E': None}, 'invalid argument: E / w is NULL'),
       ('weights', {'out': None}, 'invalid argument: E / w is NULL'),
       ('weights', {'energy': nan}, _ENERGY),
       ('weights', {'energy': inf}, _ENERGY),
       ('occ', {'E': None}, 'invalid argument: E / U is NULL'),
       ('occ', {'U': None}, 'invalid argument: E / U is NULL'),
       ('occ', {'q': None}, 'invalid argument: q / f / eb is NULL'),
       ('occ', {'f': None}, 'invalid argument: q / f / eb is NULL'),
       ('occ', {'eb': None}, 'invalid argument: q / f / eb is NULL'),
       ('occ', {'energy': -inf}, _ENERGY),
       ('occ', {'k_chunk': -1}, 'invalid argument: k_chunk < 0')]
    + _each(ARRAYS, {'n_orb': 0}, _N_ORB)
    # two faults: the order of the checks
    + _each(("dos", "pdos"), {'dim': 1, 'mesh': None}, _DOS_MESH)
    + _each(("dos", "pdos"), {'dim': 1, 'out': None}, _DOS_MESH)
    + _each(_FERMI, {'dim': 4, 'mesh': None}, _DOS_MESH)
    + _each(_OCC, {'dim': 1, 'mesh': None}, _OCC_MESH)
    + _each(("dos", "pdos"), {'out': None, 'mesh': [2, 0, 2]}, _MESH_NOS)
    + _each(("dos", "pdos"), {'mesh': [2, 0, 2], 'n_e': 1}, _ENTRY)
    + _each(("dos", "pdos"), {'n_e': 1, 'e_step': 0.0}, _FEW)
    + _each(("dos", "pdos"), {'n_e': (1 << 20) + 1, 'e_step': nan}, _MANY)
    + _each(("dos", "pdos"), {'e_step': 0.0, 'E': None}, _STEP)
    + _each(_FERMI + _OCC, {'mesh': None, 'E': None}, _MESH_NULL)
    + _each(_FERMI + _OCC, {'mesh': [0, 3, 2], 'n_orb': 0}, _ENTRY)
    + [('dos', {'E': None, 'n_orb': 0}, 'invalid argument: E is NULL'),
       ('dos', {'n_orb': 0, 'e_min': nan}, _N_ORB),
       ('pdos', {'W': None, 'n_orb': 0}, 'invalid argument: E / W is NULL'),
       ('pdos', {'n_orb': 0, 'n_groups': 0}, _N_ORB),
       ('pdos', {'n_groups': 17, 'e_min': inf}, 'invalid argument: n_groups outside [1, TBK_PDOS_MAX_GROUPS]'),
       ('nos_at', {'out': None, 'n_orb': 0}, 'invalid argument: E / energies / nos is NULL'),
       ('nos_at', {'n_orb': 0, 'n_p': 0}, _N_ORB),
       ('nos_at', {'n_p': 0, 'energies': [nan, nan]}, 'invalid argument: no probe energies'),
       ('edges', {'emax': None, 'n_orb': 0}, 'invalid argument: E / emin / emax is NULL'),
       ('fermi', {'E': None, 'n_orb': 0}, 'invalid argument: E / out is NULL'),
       ('fermi', {'n_orb': 0, 'n_electrons': nan}, _N_ORB),
       ('weights', {'out': None, 'n_orb': 0}, 'invalid argument: E / w is NULL'),
       ('weights', {'n_orb': 0, 'energy': nan}, _N_ORB),
       ('occ', {'U': None, 'q': None}, 'invalid argument: E / U is NULL'),
       ('occ', {'eb': None, 'n_orb': 0}, 'invalid argument: q / f / eb is NULL'),
       ('occ', {'n_orb': 0, 'energy': nan}, _N_ORB),
       ('occ', {'energy': nan, 'k_chunk': -1}, _ENERGY)]
)


@pytest.mark.parametrize("entry,overrides,message", CASES, ids=["%s-%d" % (case[0], i) for i, case in enumerate(CASES)])
def test_entry_rejects_with_the_exact_message(entry, overrides, message):
    status, text = call(entry, overrides)
    assert status == _lib.TBK_ERR_ARGUMENT
    assert text == message


def test_the_table_covers_every_entry_with_pairs_of_faults():
    for entry in ARRAYS:
        pairs = [case for case in CASES if case[0] == entry and len(case[1]) >= 2 and not set(case[1]) <= {'dim', 'mesh'}]
        assert len(pairs) >= 2, entry


# ---- the entry points on staged handles ----------------------------------------------------------------------------------------------
def _dense(dim, n_orb, seed, hops=True):
    """A handle of a seeded model: an on-site block and, with `hops`, one pair of hoppings along the first axis."""
    rng = np.random.default_rng(seed)
    onsite = rng.normal(size=(n_orb, n_orb)) + 1j * rng.normal(size=(n_orb, n_orb))
    blocks, vectors = [onsite + onsite.conj().T], [[0] * dim]
    if hops:
        step = 0.3 * (rng.normal(size=(n_orb, n_orb)) + 1j * rng.normal(size=(n_orb, n_orb)))
        blocks += [step, step.conj().T]
        vectors += [[1] + [0] * (dim - 1), [-1] + [0] * (dim - 1)]
    R = np.ascontiguousarray(vectors, dtype=np.int32)
    hop = np.ascontiguousarray(blocks, dtype=np.complex128)
    handle = ctypes.c_void_p()
    _lib.check(_lib.lib().tbk_model_create_dense(0, dim, n_orb, len(R), _lib.ptr(R), _lib.ptr(hop), ctypes.byref(handle)))
    return handle


@pytest.fixture(scope="module")
def handles():
    lib = _lib.lib()
    made = {"two": _dense(3, 2, 1), "two_b": _dense(3, 2, 1), "three": _dense(3, 3, 2), "chain": _dense(1, 2, 3), "chain_b": _dense(1, 2, 3),
            "wave65": _dense(3, 65, 4, hops=False), "wave65_b": _dense(3, 65, 4, hops=False)}
    for name in ("wave65", "wave65_b"):
        _lib.check(lib.tbk_model_set_option(made[name], _lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_WAVE))
    powers = np.zeros((1, 3), dtype=np.int32)
    coeffs = np.ascontiguousarray([[[0.5, 0.1j], [-0.1j, -0.5]]], dtype=np.complex128)
    kdotp = ctypes.c_void_p()
    _lib.check(lib.tbk_kdotp_create(0, 3, 2, 1, _lib.ptr(powers), _lib.ptr(coeffs), ctypes.byref(kdotp)))
    # the tbk_model* of a k.p handle is its first member (csrc/tbk_internal.h): no entry point hands it out
    made["kp"] = ctypes.c_void_p(ctypes.c_void_p.from_address(kdotp.value).value)
    yield made
    lib.tbk_kdotp_destroy(kdotp)
    for name, handle in made.items():
        if name != "kp":
            lib.tbk_model_destroy(handle)


def _pair(single, several):
    """The overrides that give a one-handle entry `single` and a _multi entry the list `several`."""
    return {'handle': single, 'handles': several}


_NO_HANDLES = 'invalid argument: no handles'
_NULL_HANDLE = 'invalid argument: a handle is NULL'
_DIFFERENT = 'invalid argument: handles of different models (dim / n_orb differ)'
_TWICE = 'invalid argument: a handle appears twice'
_KP = 'invalid argument: a k.p model has no Brillouin zone'
_WAVE = 'TBK_EIG_WAVE handles n_orb <= 64 only (n_orb = 65)'
_DOS = ("dos", "pdos")
_DOS_M = ("dos_multi", "pdos_multi")
_DOS_ALL = _DOS + _DOS_M
_FERMI_H = ("edges", "fermi", "edges_multi", "fermi_multi")
_OCC_H = ("weights", "occ", "weights_multi", "occ_multi")
_TWO = {'handles': ["two", "two_b"]}


def _with(extra, overrides):
    return dict(overrides, **extra)


def _one_and_two(entries, overrides, message):
    """On one handle, and for the _multi entries among them on two handles as well."""
    return _each(entries, overrides, message) + _each([e for e in entries if e.endswith("_multi")], _with(_TWO, overrides), message)


HANDLE_CASES = (
    # the handles
    _each(_DOS, {'handle': None}, 'invalid argument: model is NULL')
    + _each(("edges", "weights"), {'handle': None}, _NULL_HANDLE)
    + _each(("fermi", "occ"), {'handle': None}, _NO_HANDLES)
    + _each(MULTI, {'handles': None}, _NO_HANDLES)
    + _each(MULTI, {'n_handles': 0}, _NO_HANDLES)
    + _each(_DOS_M + ("edges_multi", "weights_multi"), {'handles': [None]}, _NULL_HANDLE)
    + _each(("fermi_multi", "occ_multi"), {'handles': [None, "two"]}, _NO_HANDLES)
    + _each(MULTI, {'handles': ["two", None]}, _NULL_HANDLE)
    + _each(MULTI, {'handles': ["two", "three"]}, _DIFFERENT)
    + _each(MULTI, {'handles': ["two", "chain"]}, _DIFFERENT)
    + _each(("edges_multi", "fermi_multi", "weights_multi", "occ_multi"), {'handles': ["two", "two"]}, _TWICE)
    + _each(BOTH, _pair("kp", ["kp"]), _KP)
    + _each(MULTI, {'handles': ["two", "kp"]}, _KP)
    + _each(MULTI, {'handles': ["kp", "two"]}, _KP)
    # a 1-dimensional model
    + _each(_DOS_ALL + _FERMI_H, _with(_pair("chain", ["chain"]), {'mesh': [4]}), _DOS_MESH)
    + _each(_OCC_H, _with(_pair("chain", ["chain"]), {'mesh': [4]}), _OCC_MESH)
    + _each(_DOS_M + ("edges_multi", "fermi_multi"), {'handles': ["chain", "chain_b"], 'mesh': [4]}, _DOS_MESH)
    + _each(("weights_multi", "occ_multi"), {'handles': ["chain", "chain_b"], 'mesh': [4]}, _OCC_MESH)
    # the mesh
    + _one_and_two(_DOS_ALL, {'mesh': None}, _MESH_NOS)
    + _one_and_two(_FERMI_H + _OCC_H, {'mesh': None}, _MESH_NULL)
    + _one_and_two(BOTH, {'mesh': [0, 3, 2]}, _ENTRY)
    + _one_and_two(BOTH, {'mesh': [2, 0, 2]}, _ENTRY)
    + _one_and_two(BOTH, {'mesh': [2, 3, -1]}, _ENTRY)
    + _one_and_two(BOTH, {'mesh': [65536, 32768, 1]}, _POINTS)
    # the results
    + _one_and_two(_DOS_ALL, {'out': None}, _MESH_NOS)
    + _one_and_two(("edges", "edges_multi"), {'emin': None}, 'invalid argument: emin / emax is NULL')
    + _one_and_two(("edges", "edges_multi"), {'emax': None}, 'invalid argument: emin / emax is NULL')
    + _one_and_two(("fermi", "fermi_multi"), {'out': None}, 'invalid argument: out is NULL')
    + _one_and_two(("weights", "weights_multi"), {'out': None}, 'invalid argument: w is NULL')
    + [(entry, _with(extra, {key: None}), 'invalid argument: mu / q / f / eb is NULL')
       for entry, extra in (("occ", {}), ("occ_multi", {}), ("occ_multi", _TWO)) for key in ("mu", "q", "f", "eb")]
    # the energy grid: a fault that the slabs of several handles find (the front of the _multi entries does not look at it)
    + _one_and_two(_DOS_ALL, {'e_step': 0.0}, _STEP)
    + _one_and_two(_DOS_ALL, {'e_step': -0.25}, _STEP)
    + _one_and_two(_DOS_ALL, {'e_step': nan}, _STEP)
    + _one_and_two(_DOS_ALL, {'e_min': nan}, _E_MIN)
    + _one_and_two(_DOS_ALL, {'e_min': inf}, _E_MIN)
    # ... and one that the front of the _multi entries finds first with several handles, under another text: one handle here
    + _each(_DOS_ALL, {'n_e': 1}, _FEW)
    + _each(_DOS_ALL, {'n_e': 0}, _FEW)
    + _each(_DOS_ALL, {'n_e': (1 << 20) + 1}, _MANY)
    # the groups
    + _one_and_two(("pdos", "pdos_multi"), {'offsets': None}, 'invalid argument: group_offsets / group_orbitals is NULL')
    + _one_and_two(("pdos", "pdos_multi"), {'orbitals': None}, 'invalid argument: group_offsets / group_orbitals is NULL')
    + _one_and_two(("pdos", "pdos_multi"), {'n_groups': 0}, 'invalid argument: no projection groups')
    + _one_and_two(("pdos", "pdos_multi"), {'n_groups': 17}, 'invalid argument: more than TBK_PDOS_MAX_GROUPS projection groups')
    + _one_and_two(("pdos", "pdos_multi"), {'offsets': [1, 2]}, 'invalid argument: group_offsets[0] must be 0')
    + _one_and_two(("pdos", "pdos_multi"), {'offsets': [0, 0]}, 'invalid argument: a projection group is empty')
    + _one_and_two(("pdos", "pdos_multi"), {'n_groups': 2, 'offsets': [0, 1, 1], 'orbitals': [0]}, 'invalid argument: a projection group is empty')
    + _one_and_two(("pdos", "pdos_multi"), {'offsets': [0, 3], 'orbitals': [0, 1, 0]}, 'invalid argument: an orbital repeats inside a projection group')
    + _one_and_two(("pdos", "pdos_multi"), {'offsets': [0, 2], 'orbitals': [1, 1]}, 'invalid argument: an orbital repeats inside a projection group')
    + _one_and_two(("pdos", "pdos_multi"), {'orbitals': [2]}, 'invalid argument: an orbital index of a projection group is out of range')
    + _one_and_two(("pdos", "pdos_multi"), {'orbitals': [-1]}, 'invalid argument: an orbital index of a projection group is out of range')
    # n_electrons, the mode and the energy
    + [(entry, _with(extra, {'n_electrons': value}), _ELECTRONS)
       for entry, extra in (("fermi", {}), ("fermi_multi", {}), ("fermi_multi", _TWO)) for value in (0.0, 2.0, -1.0, nan, inf)]
    + [(entry, _with(extra, {'mode': 1, 'value': value}), _ELECTRONS)
       for entry, extra in (("occ", {}), ("occ_multi", {}), ("occ_multi", _TWO)) for value in (0.0, 2.0, nan)]
    + _one_and_two(("occ", "occ_multi"), {'mode': 2}, 'invalid argument: mode must be 0 (value = energy) or 1 (value = n_electrons)')
    + _one_and_two(("occ", "occ_multi"), {'mode': -1}, 'invalid argument: mode must be 0 (value = energy) or 1 (value = n_electrons)')
    + _one_and_two(("occ", "occ_multi"), {'value': nan}, _ENERGY)
    + _one_and_two(("occ", "occ_multi"), {'value': -inf}, _ENERGY)
    + _one_and_two(("weights", "weights_multi"), {'energy': nan}, _ENERGY)
    + _one_and_two(("weights", "weights_multi"), {'energy': inf}, _ENERGY)
    # TBK_EIG_WAVE above 64 orbitals: the eigenvalue path's text, whoever asks first
    + _each(BOTH, _pair("wave65", ["wave65"]), _WAVE)
    + _each(MULTI, {'handles': ["wave65", "wave65_b"]}, _WAVE)
    # two faults: the order of the checks
    + _each(_DOS, {'handle': None, 'mesh': None}, 'invalid argument: model is NULL')
    + _each(_DOS, {'handle': "chain", 'mesh': None}, _MESH_NOS)
    + _each(_DOS, {'handle': "chain", 'mesh': [4], 'out': None}, _DOS_MESH)  # (a wrong dim in front of a NULL nos ...)
    + _each(_DOS_M, {'handles': ["chain"], 'mesh': [4], 'out': None}, _MESH_NOS)  # (... but not in the _multi entries)
    + _each(_DOS_M, {'handles': ["chain", "chain_b"], 'mesh': [4], 'out': None}, _MESH_NOS)
    + _each(_DOS_M, {'handles': ["two", None], 'mesh': None}, _NULL_HANDLE)
    + _each(_DOS_M, {'handles': ["two", "three"], 'out': None}, _DIFFERENT)
    + _each(_DOS_ALL, _with(_pair("chain", ["chain"]), {'mesh': [0]}), _DOS_MESH)
    + _each(_DOS_ALL, _with(_pair("kp", ["kp"]), {'mesh': [0, 3, 2]}), _ENTRY)
    + _each(_DOS_ALL, _with(_pair("kp", ["kp"]), {'mesh': [2, 0, 2]}), _KP)
    + _each(_DOS_ALL, _with(_pair("kp", ["kp"]), {'n_e': 1}), _KP)
    + _each(_DOS, {'handle': "kp", 'out': None}, _KP)
    + _each(_DOS_M, {'handles': ["two", "kp"], 'mesh': [2, 0, 2]}, _ENTRY)  # (the first slab's fault)
    + _each(_DOS_ALL, {'mesh': [2, 0, 2], 'n_e': 1}, _ENTRY)
    + _each(_DOS_ALL, {'mesh': [65536, 32768, 1], 'n_e': 1}, _POINTS)
    + _each(_DOS_ALL, {'n_e': 1, 'e_step': 0.0}, _FEW)
    + _one_and_two(_DOS_ALL, {'e_step': 0.0, 'e_min': nan}, _STEP)
    + _each(("pdos", "pdos_multi"), {'e_min': nan, 'n_groups': 0}, _E_MIN)
    + _each(("pdos", "pdos_multi"), _with(_pair("wave65", ["wave65"]), {'n_groups': 0}), 'invalid argument: no projection groups')
    + _each(_DOS_ALL, _with(_pair("wave65", ["wave65"]), {'e_min': nan}), _E_MIN)
    + _each(_FERMI_H + _OCC_H, _with(_pair("kp", ["kp"]), {'mesh': None}), _KP)
    + _each(("edges_multi", "fermi_multi", "weights_multi", "occ_multi"), {'handles': ["two", "two"], 'mesh': None}, _TWICE)
    + _each(("edges_multi", "fermi_multi", "weights_multi", "occ_multi"), {'handles': ["kp", "kp"]}, _KP)
    + _each(("edges_multi", "fermi_multi", "weights_multi", "occ_multi"), {'handles': ["kp", None]}, _KP)
    + _each(("edges_multi", "weights_multi"), {'handles': ["two", "three", None]}, _DIFFERENT)
    + _each(("edges", "edges_multi"), _with(_pair(None, [None]), {'emin': None}), 'invalid argument: emin / emax is NULL')
    + _each(("fermi", "fermi_multi"), _with(_pair(None, [None]), {'out': None}), 'invalid argument: out is NULL')
    + _each(("fermi", "fermi_multi"), _with(_pair(None, [None]), {'n_electrons': 0.0}), _NO_HANDLES)
    + _each(("fermi", "fermi_multi"), {'n_electrons': 0.0, 'mesh': None}, _ELECTRONS)
    + _each(("fermi", "fermi_multi"), _with(_pair("kp", ["kp"]), {'n_electrons': 2.0}), _ELECTRONS)
    + _each(("fermi", "fermi_multi"), _with(_pair("three", ["three"]), {'n_electrons': 2.5, 'mesh': [2, 0, 2]}), _ENTRY)
    + _each(("fermi_multi",), {'handles': ["three", "two"], 'n_electrons': 2.5}, _DIFFERENT)
    + _each(("fermi_multi",), {'handles': ["two", "three"], 'n_electrons': 2.5}, _ELECTRONS)
    + _each(("weights", "weights_multi"), _with(_pair(None, [None]), {'energy': nan}), _ENERGY)
    + _each(("weights", "weights_multi"), {'out': None, 'energy': nan}, 'invalid argument: w is NULL')
    + _each(("weights", "weights_multi"), _with(_pair("wave65", ["wave65"]), {'mesh': [2, 0, 2]}), _ENTRY)
    + _each(("occ", "occ_multi"), {'mu': None, 'mode': 2}, 'invalid argument: mu / q / f / eb is NULL')
    + _each(("occ", "occ_multi"), _with(_pair(None, [None]), {'mode': 2}), 'invalid argument: mode must be 0 (value = energy) or 1 (value = n_electrons)')
    + _each(("occ", "occ_multi"), _with(_pair(None, [None]), {'value': nan}), _NO_HANDLES)
    + _each(("occ", "occ_multi"), _with(_pair("kp", ["kp"]), {'value': nan}), _ENERGY)
    + _each(("occ", "occ_multi"), {'mode': 1, 'value': 2.0, 'mesh': None}, _ELECTRONS)
)

# With two handles the front of tbk_dos_multi and tbk_pdos_multi looks at the size of the grid and at the groups before a slab looks at
# the mesh, at a k.p handle or at e_min
_GRID_SEVERAL = 'invalid argument: the energy grid needs 2 to 2^20 points'
SEVERAL = (
    _each(_DOS_M, _with(_TWO, {'n_e': 1}), _GRID_SEVERAL)
    + _each(_DOS_M, _with(_TWO, {'n_e': (1 << 20) + 1}), _GRID_SEVERAL)
    + _each(_DOS_M, _with(_TWO, {'mesh': [2, 0, 2], 'n_e': 1}), _GRID_SEVERAL)
    + _each(_DOS_M, {'handles': ["kp", "two"], 'n_e': 1}, _GRID_SEVERAL)
    + _each(_DOS_M, {'handles': ["two", "kp"], 'n_e': 1}, _GRID_SEVERAL)
    + _each(("pdos_multi",), _with(_TWO, {'e_min': nan, 'n_groups': 0}), 'invalid argument: no projection groups')
    + _each(("pdos_multi",), _with(_TWO, {'mesh': [2, 0, 2], 'offsets': [1, 2]}), 'invalid argument: group_offsets[0] must be 0')
    + _each(("pdos_multi",), {'handles': ["kp", "two"], 'n_groups': 17}, 'invalid argument: more than TBK_PDOS_MAX_GROUPS projection groups')
)
HANDLE_CASES = HANDLE_CASES + SEVERAL


def _ids(cases):
    return ["%s-%d" % (case[0], i) for i, case in enumerate(cases)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,overrides,message", HANDLE_CASES, ids=_ids(HANDLE_CASES))
def test_handle_entry_rejects_with_the_exact_message(handles, entry, overrides, message):
    status, text = call(entry, overrides, HANDLE_ENTRIES, handles)
    assert status == _lib.TBK_ERR_ARGUMENT
    assert text == message


@pytest.mark.gpu
@pytest.mark.parametrize("entry", BOTH)
def test_the_input_the_cases_override_passes(handles, entry):
    for overrides in ({}, _TWO) if entry.endswith("_multi") else ({},):
        status, text = call(entry, overrides, HANDLE_ENTRIES, handles)
        assert status == 0, text


def test_the_handle_table_covers_every_entry_with_pairs_of_faults():
    for entry in BOTH:
        pairs = [case for case in HANDLE_CASES if case[0] == entry and len({'handles' if key == 'handle' else key for key in case[1]}) >= 2]
        assert len(pairs) >= 2, entry
