"""
Model.eigh / the tbk_eigh* entry points on the host side (no GPU): argument errors surface before any device work.
"""

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib


def _two_band_model():
    return tbmodels_amd.Model(hop={(0, 0, 0): np.diag([0.5, -0.5]).astype(complex)}, size=2, dim=3, contains_cc=False)


@pytest.mark.parametrize("convention", ["a", "1", None, 3])
def test_eigh_invalid_convention_raises_before_any_library_call(convention, monkeypatch):
    """The ValueError of Model.hamilton for the same convention, raised before the library is even loaded."""
    model = _two_band_model()

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match="Invalid value .* for 'convention'"):
        model.eigh((0, 0, 0), convention=convention)
    with pytest.raises(ValueError, match="Invalid value .* for 'convention'"):
        model.eigh([(0, 0, 0), (0.1, 0.2, 0.3)], convention=convention)


def _calls(lib, k, pos, out_e, out_u):
    """Every eigh entry point as call(model_or_handles, nk, convention, pos) -> status (k.p entries: convention 2)."""
    kp, pp, ep, up = _lib.ptr(k), _lib.ptr(pos), _lib.ptr(out_e), _lib.ptr(out_u)
    return {
        "tbk_eigh": lambda nk, conv, p: lib.tbk_eigh(None, kp, nk, conv, p, ep, up),
        "tbk_eigh_device": lambda nk, conv, p: lib.tbk_eigh_device(None, kp, nk, conv, p, ep, up),
        "tbk_eigh_multi": lambda nk, conv, p: lib.tbk_eigh_multi(None, 1, kp, nk, conv, p, ep, up),
        "tbk_kdotp_eigh": lambda nk, conv, p: lib.tbk_kdotp_eigh(None, kp, nk, ep, up),
        "tbk_kdotp_eigh_multi": lambda nk, conv, p: lib.tbk_kdotp_eigh_multi(None, 1, kp, nk, ep, up),
    }, pp


def test_eigh_entries_reject_bad_arguments_before_touching_a_device():
    lib = _lib.lib()
    k = np.zeros((4, 3))
    pos = np.zeros((2, 3))
    out_e = np.zeros((4, 2))
    out_u = np.zeros((4, 2, 2), dtype=complex)
    calls, pos_ptr = _calls(lib, k, pos, out_e, out_u)
    for name, call in calls.items():
        kdotp = name.startswith("tbk_kdotp")
        assert call(4, 2, pos_ptr) == _lib.TBK_ERR_ARGUMENT, name  # NULL model / no handles
        assert call(-1, 2, pos_ptr) == _lib.TBK_ERR_ARGUMENT, name
        assert "nk < 0" in _lib.last_error(), (name, _lib.last_error())
        if kdotp:
            continue
        assert call(4, 3, pos_ptr) == _lib.TBK_ERR_ARGUMENT, name
        assert "convention must be 1 or 2" in _lib.last_error(), (name, _lib.last_error())
        assert call(4, 1, None) == _lib.TBK_ERR_ARGUMENT, name
        assert "convention 1 needs pos" in _lib.last_error(), (name, _lib.last_error())
    assert not out_e.any() and not out_u.any()
    with pytest.raises(ValueError):
        _lib.check(lib.tbk_eigh(None, _lib.ptr(k), 4, 2, None, _lib.ptr(out_e), _lib.ptr(out_u)))
