"""
The argument checks of `Model.green_function(self_energy=...)`, which need no device, and the C ABI of the dressed entry points
(header = ctypes).  No GPU.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _silicon():
    g = load_golden("silicon")
    return tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])


class _Reached(Exception):
    """the argument checks are behind us: the call asked for the library"""


def test_python_argument_errors_need_no_device(monkeypatch):
    model = _silicon()
    n = model.size
    one_d = tbmodels_amd.Model(hop={(0,): np.eye(2, dtype=complex) / 2, (1,): 0.1 * np.ones((2, 2), dtype=complex)}, size=2, dim=1,
                               contains_cc=False)

    def no_device_call():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "lib", no_device_call)
    mesh, z2 = (2, 2, 2), [0.1 + 0.2j, -0.3]
    good = np.zeros((2, n, n), dtype=complex)
    nan_entry, inf_entry = good.copy(), good.copy()
    nan_entry[1, 2, 3] = complex(0.0, np.nan)
    inf_entry[0, 0, 0] = np.inf
    wrong = [
        np.zeros((n, n)),                  # one matrix for two energies
        np.zeros((2, n)),                  # wrong rank
        np.zeros((2, n, n, 1)),
        np.zeros((2, n, n + 1)),           # not square / not the model's size
        np.zeros((2, n - 1, n - 1)),
        np.zeros((3, n, n)),               # NZ mismatch
        np.zeros((1, n, n)),
        nan_entry, inf_entry,              # not finite
        "sigma", b"sigma", [["a"] * n] * n,  # strings
        np.zeros((2, n, n), dtype=object),
        0.5, [],
    ]
    for sigma in wrong:
        with pytest.raises(ValueError):
            model.green_function(mesh, z2, self_energy=sigma)
    with pytest.raises(ValueError):
        model.green_function(mesh, 0.5, self_energy=np.zeros((2, n, n)))  # one energy, two matrices
    # the other arguments keep their checks with a self-energy
    for z in (np.nan, [1j, complex(np.inf, 1.0)], [], "1j", None, [[1j, 2j]]):
        with pytest.raises(ValueError):
            model.green_function(mesh, z, self_energy=good)
    with pytest.raises(ValueError):
        model.green_function((2, 0, 2), z2, self_energy=good)
    with pytest.raises(ValueError):
        model.green_function(mesh, z2, self_energy=good, R=[[0.5, 0, 0]])
    with pytest.raises(ValueError):
        one_d.green_function((4,), 1j, self_energy=np.zeros((2, 2)))
    # a real z is refused without a self-energy, as before ...
    for z in (0.5, [1j, 2.0], -0.3 + 0j):
        with pytest.raises(ValueError):
            model.green_function(mesh, z)
        with pytest.raises(ValueError):
            model.green_function(mesh, z, self_energy=None)

    # ... and accepted with one: the call gets as far as the library
    def reached():
        raise _Reached

    monkeypatch.setattr(_lib, "lib", reached)
    with pytest.raises(_Reached):
        model.green_function(mesh, z2, self_energy=good)
    with pytest.raises(_Reached):
        model.green_function(mesh, 0.5, self_energy=np.zeros((n, n)))  # one number, one matrix
    with pytest.raises(_Reached):
        model.green_function(mesh, [0.5], self_energy=[np.eye(n).tolist()])  # array-like, real dtype
    assert not hasattr(tbmodels_amd.KdotpModel, "green_function")


def test_self_energy_argument_is_normalised():
    model = _silicon()
    n = model.size
    sigma = model._self_energy_argument(np.eye(n, dtype=np.float32), 0.5, 1)
    assert sigma.shape == (1, n, n) and sigma.dtype == np.complex128 and sigma.flags.c_contiguous
    strided = np.zeros((n, n, 3), dtype=complex).transpose(2, 0, 1)
    assert model._self_energy_argument(strided, [1, 2, 3], 3).flags.c_contiguous
    assert np.array_equal(model._complex_energies_argument([0.5, 1j], off_axis=False), np.array([0.5 + 0j, 1j]))


def test_status_and_signatures_agree_with_the_header():
    with open(os.path.join(ROOT, "include", "tbk.h")) as handle:
        header = handle.read()
    assert re.search(r"TBK_ERR_SINGULAR\s*=\s*6\b", header) and _lib.TBK_ERR_SINGULAR == 6
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    counts = {"tbk_green_dressed_from_matrices": 13, "tbk_green_dressed": 8, "tbk_green_dressed_multi": 9, "tbk_green_dressed_timing": 4}
    for name, count in counts.items():
        found = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert found, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        declared = [" ".join(part.split()) for part in found.group(1).split(",")]
        assert len(declared) == len(argtypes) == count, (name, declared)
        for text, ctype in zip(declared, argtypes):
            if "*" in text:
                assert ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer), (name, text)
            else:
                assert ctype is kinds[text.rsplit(" ", 1)[0]], (name, text)


def test_singular_status_maps_to_linalgerror(monkeypatch):
    monkeypatch.setattr(_lib, "last_error", lambda: "Singular matrix: somewhere")
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        _lib.check(_lib.TBK_ERR_SINGULAR)
