"""The argument checks of the three entry points that Fourier-sum a per-k matrix of the caller's arrays over a uniform mesh into
lattice vectors -- ``tbk_density_matrix_from_eigensystem``, ``tbk_green_from_eigensystem``, ``tbk_green_dressed_from_matrices`` -- and
of ``tbk_dm_plan`` / ``tbk_green_plan``: for every invalid input the exact status and the exact text of ``tbk_last_error()``.  Every
one of these checks stands in front of the one that needs a device, so the table holds no valid input and no case needs a GPU.
Inputs with two faults pin the order of the checks: the message names the first.

Not in the table: "more than 16320 orbitals" of the dressed function.  Its check of the self-energy stands in front and reads all
``n_z * n_orb^2`` complex values of Sigma: 4 GiB at 16321 orbitals.  The density matrix and the Green's function, which share the check,
have the case.
"""

import ctypes

import numpy as np
import pytest

from tbmodels_amd import _lib

nan, inf = float("nan"), float("inf")

_GREEN_HEAD = ["k_chunk", "z_tile", "n_z", "z"]
ENTRIES = {
    "dm": ("tbk_density_matrix_from_eigensystem", ["device", "dim", "mesh", "n_orb", "E", "U", "energy", "k_chunk", "n_r", "R", "out"]),
    "green": ("tbk_green_from_eigensystem", ["device", "dim", "mesh", "n_orb", "E", "U"] + _GREEN_HEAD + ["n_r", "R", "out"]),
    "dressed": ("tbk_green_dressed_from_matrices", ["device", "dim", "mesh", "n_orb", "H"] + _GREEN_HEAD + ["Sigma", "n_r", "R", "out"]),
    "dm_plan": ("tbk_dm_plan", ["rows", "n_orb", "n_r", "plan"]),
    "green_plan": ("tbk_green_plan", ["rows", "n_orb", "n_r", "n_z", "z_tile", "k_chunk", "plan"]),
}
ARRAYS = ("dm", "green", "dressed")

# An input that passes every check but the device's; a case overrides some of it.  "buf": some memory that no check reads.
BASE = {"device": 0, "dim": 3, "mesh": [2, 3, 2], "n_orb": 2, "energy": 0.25, "k_chunk": 0, "z_tile": 0, "n_z": 1, "z": [0.3, 0.1],
        "Sigma": [0.0] * 8, "n_r": 1, "rows": 12}
_BUF = np.zeros(64)
_PLAN = (ctypes.c_int64 * 8)()


def call(entry, overrides):
    """(status, tbk_last_error()) of the entry point on BASE with the overrides."""
    name, order = ENTRIES[entry]
    values = dict({key: "buf" for key in order}, **BASE)
    values.update(overrides)
    keep = []  # the arrays stay alive until the call has returned
    args = []
    for key in order:
        value = values[key]
        if key in ("mesh", "z", "Sigma") and value is not None:
            keep.append(np.array(value, dtype=np.int32 if key == "mesh" else np.float64))
            value = _lib.ptr(keep[-1])
        elif key == "plan" and value == "buf":
            value = _PLAN
        elif isinstance(value, str) and value == "buf":
            value = _lib.ptr(_BUF)
        args.append(value)
    status = getattr(_lib.lib(), name)(*args)
    return status, _lib.last_error()


_MESH = 'invalid argument: the tetrahedron weights need a 2- or 3-dimensional mesh'
_NZ = 'invalid argument: n_z must be 1 to 4096'
_PLAN_SIZES = 'invalid argument: rows / n_orb / n_r < 1 or out is NULL'


def _each(entries, overrides, message):
    return [(entry, overrides, message) for entry in entries]


# (entry, overrides of BASE, tbk_last_error())
CASES = (
    # the mesh
    _each(ARRAYS, {'dim': 1}, _MESH)
    + _each(ARRAYS, {'dim': 4}, _MESH)
    + _each(ARRAYS, {'mesh': None}, 'invalid argument: mesh is NULL')
    + _each(ARRAYS, {'mesh': [2, 0, 2]}, 'invalid argument: a mesh entry is < 1')
    + _each(ARRAYS, {'mesh': [2, 3, -1]}, 'invalid argument: a mesh entry is < 1')
    + _each(ARRAYS, {'mesh': [65536, 32768, 1]}, 'invalid argument: the mesh has 2^31 points or more')
    + _each(ARRAYS, {'dim': 2, 'mesh': [65536, 65536]}, 'invalid argument: the mesh has 2^31 points or more')
    # the caller's arrays and the sizes
    + [('dm', {'E': None}, 'invalid argument: E / U is NULL'),
       ('dm', {'U': None}, 'invalid argument: E / U is NULL'),
       ('green', {'E': None}, 'invalid argument: E / U is NULL'),
       ('green', {'U': None}, 'invalid argument: E / U is NULL'),
       ('dressed', {'H': None}, 'invalid argument: H is NULL')]
    + _each(ARRAYS, {'n_orb': 0}, 'invalid argument: n_orb < 1')
    + [('dm', {'energy': nan}, 'invalid argument: the energy is not finite'),
       ('dm', {'energy': -inf}, 'invalid argument: the energy is not finite'),
       ('dm', {'k_chunk': -1}, 'invalid argument: k_chunk < 0'),
       ('green', {'k_chunk': -1}, 'invalid argument: k_chunk / z_tile < 0'),
       ('green', {'z_tile': -1}, 'invalid argument: k_chunk / z_tile < 0'),
       ('dressed', {'k_chunk': -1}, 'invalid argument: k_chunk / z_tile < 0'),
       ('dressed', {'z_tile': -1}, 'invalid argument: k_chunk / z_tile < 0')]
    # the energies and the self-energy
    + _each(('green', 'dressed'), {'n_z': 0}, _NZ)
    + _each(('green', 'dressed'), {'n_z': 4097}, _NZ)
    + [('green', {'z': None}, 'invalid argument: z is NULL'),
       ('dressed', {'z': None}, 'invalid argument: z / Sigma is NULL'),
       ('dressed', {'Sigma': None}, 'invalid argument: z / Sigma is NULL')]
    + _each(('green', 'dressed'), {'z': [nan, 0.1]}, 'invalid argument: an energy z is not finite')
    + _each(('green', 'dressed'), {'z': [0.3, inf]}, 'invalid argument: an energy z is not finite')
    + [('green', {'z': [0.3, 0.0]}, 'invalid argument: an energy z has Im z = 0: the resolvent is evaluated off the real axis only'),
       ('green', {'n_z': 2, 'z': [0.3, 0.1, 0.4, 0.0]},
        'invalid argument: an energy z has Im z = 0: the resolvent is evaluated off the real axis only'),
       ('dressed', {'n_z': 2, 'z': [0.3, 0.1, nan, 0.0], 'Sigma': [0.0] * 16}, 'invalid argument: an energy z is not finite'),
       ('dressed', {'Sigma': [0.0] * 7 + [nan]}, 'invalid argument: an element of the self-energy is not finite'),
       ('dressed', {'Sigma': [inf] + [0.0] * 7}, 'invalid argument: an element of the self-energy is not finite'),
       ('dressed', {'n_z': 2, 'z': [0.3, 0.1, 0.4, 0.0], 'Sigma': [0.0] * 15 + [-inf]},
        'invalid argument: an element of the self-energy is not finite')]
    # the lattice vectors and the result
    + _each(ARRAYS, {'n_r': 0}, 'invalid argument: n_r < 1')
    + _each(ARRAYS, {'R': None}, 'invalid argument: R / rho is NULL')
    + _each(ARRAYS, {'out': None}, 'invalid argument: R / rho is NULL')
    + _each(ARRAYS, {'n_r': 1048561}, 'invalid argument: more than 1048560 lattice vectors in one call')
    + _each(('dm', 'green'), {'n_orb': 16321}, 'invalid argument: more than 16320 orbitals')
    # the plans
    + _each(('dm_plan', 'green_plan'), {'rows': 0}, _PLAN_SIZES)
    + _each(('dm_plan', 'green_plan'), {'n_orb': 0}, _PLAN_SIZES)
    + _each(('dm_plan', 'green_plan'), {'n_r': 0}, _PLAN_SIZES)
    + _each(('dm_plan', 'green_plan'), {'plan': None}, _PLAN_SIZES)
    + [('green_plan', {'n_z': 0}, _NZ),
       ('green_plan', {'n_z': 4097}, _NZ),
       ('green_plan', {'z_tile': -1}, 'invalid argument: z_tile / k_chunk < 0'),
       ('green_plan', {'k_chunk': -1}, 'invalid argument: z_tile / k_chunk < 0')]
    # two faults: the order of the checks
    + _each(ARRAYS, {'dim': 1, 'mesh': None}, _MESH)
    + _each(ARRAYS, {'mesh': None, 'n_orb': 0}, 'invalid argument: mesh is NULL')
    + _each(ARRAYS, {'mesh': [2, 0, 2], 'n_r': 0}, 'invalid argument: a mesh entry is < 1')
    + [('dm', {'E': None, 'n_orb': 0}, 'invalid argument: E / U is NULL'),
       ('green', {'U': None, 'n_orb': 0}, 'invalid argument: E / U is NULL'),
       ('dressed', {'H': None, 'n_orb': 0}, 'invalid argument: H is NULL'),
       ('dm', {'n_orb': 0, 'energy': nan}, 'invalid argument: n_orb < 1'),
       ('dm', {'energy': nan, 'k_chunk': -1}, 'invalid argument: the energy is not finite'),
       ('dm', {'k_chunk': -1, 'n_r': 0}, 'invalid argument: k_chunk < 0'),
       ('dm', {'n_r': 0, 'R': None}, 'invalid argument: n_r < 1'),
       ('dm', {'R': None, 'n_r': 1048561}, 'invalid argument: R / rho is NULL'),
       ('dm', {'n_r': 1048561, 'n_orb': 16321}, 'invalid argument: more than 1048560 lattice vectors in one call'),
       ('green', {'n_orb': 0, 'z_tile': -1}, 'invalid argument: n_orb < 1'),
       ('green', {'k_chunk': -1, 'n_z': 0}, 'invalid argument: k_chunk / z_tile < 0'),
       ('green', {'n_z': 0, 'z': None}, _NZ),
       ('green', {'z': None, 'n_r': 0}, 'invalid argument: z is NULL'),
       ('green', {'z': [nan, 0.0]}, 'invalid argument: an energy z is not finite'),
       ('green', {'n_z': 2, 'z': [0.3, 0.0, nan, 0.1]},
        'invalid argument: an energy z has Im z = 0: the resolvent is evaluated off the real axis only'),
       ('green', {'z': [0.3, 0.0], 'out': None},
        'invalid argument: an energy z has Im z = 0: the resolvent is evaluated off the real axis only'),
       ('green', {'n_r': 0, 'n_orb': 16321}, 'invalid argument: n_r < 1'),
       ('dressed', {'n_orb': 0, 'k_chunk': -1}, 'invalid argument: n_orb < 1'),
       ('dressed', {'z_tile': -1, 'n_z': 4097}, 'invalid argument: k_chunk / z_tile < 0'),
       ('dressed', {'n_z': 0, 'Sigma': None}, _NZ),
       ('dressed', {'Sigma': None, 'z': [nan, 0.1]}, 'invalid argument: z / Sigma is NULL'),
       ('dressed', {'z': [0.3, inf], 'Sigma': [nan] * 8}, 'invalid argument: an energy z is not finite'),
       ('dressed', {'Sigma': [nan] * 8, 'n_r': 0}, 'invalid argument: an element of the self-energy is not finite'),
       ('dressed', {'n_r': 0, 'out': None}, 'invalid argument: n_r < 1'),
       ('dressed', {'out': None, 'n_r': 1048561}, 'invalid argument: R / rho is NULL'),
       ('green_plan', {'rows': 0, 'n_z': 0}, _PLAN_SIZES),
       ('green_plan', {'n_z': 0, 'k_chunk': -1}, _NZ),
       ('green_plan', {'plan': None, 'z_tile': -1}, _PLAN_SIZES),
       ('dm_plan', {'rows': 0, 'plan': None}, _PLAN_SIZES)]
)


@pytest.mark.parametrize("entry,overrides,message", CASES, ids=["%s-%d" % (case[0], i) for i, case in enumerate(CASES)])
def test_entry_rejects_with_the_exact_message(entry, overrides, message):
    status, text = call(entry, overrides)
    assert status == _lib.TBK_ERR_ARGUMENT
    assert text == message


def test_the_table_covers_every_entry_with_pairs_of_faults():
    for entry in ARRAYS:
        pairs = [case for case in CASES if case[0] == entry and len(case[1]) >= 2 and not set(case[1]) <= {'dim', 'mesh', 'n_z', 'z', 'Sigma'}]
        assert len(pairs) >= 3, entry
    for entry in ("dm_plan", "green_plan"):
        assert any(case[0] == entry and len(case[1]) >= 2 for case in CASES), entry
