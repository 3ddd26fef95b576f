"""KZG opening on resident base sets (sv_bn254_fr_poly_div_linear_device, sv_bn254_kzg_open,
sv_bn254_kzg_open_device; include/svgpu.h): every argument rule returns its code and message before
anything touches a device, in the documented order -- form / null, empty, length, z, handle, range --
so all of it is checked here without a GPU.  No call below is valid through rule 4 for the division
or through rule 5 for the openings, so none reaches a device where there is one."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

_BUF = np.zeros(64, np.uint64)
_P = _BUF.ctypes.data
_EVAL = _lib.sv_fe()
_OUT = _lib.sv_g1_affine()
_PART = _lib.sv_g1_jacobian()
_Z = enc.fe_struct(5)
_Z_BAD = [enc.fe_struct(v) for v in (b.R, b.R + 5, (1 << 256) - 1)]
_UNKNOWN = 424242
_TOO_LONG = (1 << 26) + 1


def _div(coeffs, n, z, form, ev=ctypes.byref(_EVAL)):
    return _lib.lib.sv_bn254_fr_poly_div_linear_device(coeffs, n, z, form, 0, None, None, ev)


def _open(coeffs, n, z, form, ev=ctypes.byref(_EVAL), handle=_UNKNOWN, offset=0, out=ctypes.byref(_OUT)):
    return _lib.lib.sv_bn254_kzg_open(handle, offset, coeffs, n, z, form, ev, out)


def _open_dev(coeffs, n, z, form, ev=ctypes.byref(_EVAL), handle=_UNKNOWN, offset=0, out=ctypes.byref(_PART)):
    return _lib.lib.sv_bn254_kzg_open_device(handle, offset, coeffs, n, z, form, None, ev, out)


CALLS = [_div, _open, _open_dev]


@pytest.mark.parametrize("call", CALLS)
def test_form_and_null_pointers_come_first(call):
    z = ctypes.byref(_Z)
    assert call(_P, 1, z, 7) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    assert call(None, 1, z, 0) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert call(_P, 1, None, 0) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert call(_P, 1, z, 1, ev=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    # before emptiness, the length and z
    assert call(_P, 0, z, 7) == _lib.SV_ERR_ARG
    assert call(None, 0, z, 0) == _lib.SV_ERR_ARG
    assert call(_P, _TOO_LONG, ctypes.byref(_Z_BAD[0]), 9) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()


@pytest.mark.parametrize("call", [_open, _open_dev])
def test_null_witness_pointer(call):
    assert call(_P, 1, ctypes.byref(_Z), 0, out=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()


@pytest.mark.parametrize("call", CALLS)
def test_empty_then_length_then_z(call):
    z, zbad = ctypes.byref(_Z), ctypes.byref(_Z_BAD[0])
    for form in (0, 1):
        assert call(_P, 0, z, form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert call(_P, 0, zbad, form) == _lib.SV_ERR_EMPTY          # emptiness before z
        assert call(_P, _TOO_LONG, z, form) == _lib.SV_ERR_LEN
        assert "2^26" in _lib.last_error()
        assert call(_P, _TOO_LONG, zbad, form) == _lib.SV_ERR_LEN    # the length before z
        for bad in _Z_BAD:                                           # z before the handle
            assert call(_P, 1, ctypes.byref(bad), form) == _lib.SV_ERR_ARG
            assert "not reduced" in _lib.last_error()
            assert call(_P, 1 << 26, ctypes.byref(bad), form) == _lib.SV_ERR_ARG
            assert "not reduced" in _lib.last_error()


@pytest.mark.parametrize("call", [_open, _open_dev])
def test_handle_then_range(call):
    z = ctypes.byref(_Z)
    assert call(_P, 1, z, 0) == _lib.SV_ERR_ARG
    assert "unknown base set handle 424242" in _lib.last_error()     # sv_bn254_g1_msm_bases' message
    assert call(_P, 1 << 26, z, 1, handle=987654321) == _lib.SV_ERR_ARG
    assert "unknown base set handle 987654321" in _lib.last_error()
    # offsets near 2^64: the range check must not wrap into the handle's range
    assert call(_P, 2, z, 1, offset=(1 << 64) - 1) == _lib.SV_ERR_ARG
    assert call(_P, 1, z, 0, offset=(1 << 64) - 1) == _lib.SV_ERR_ARG


def test_python_wrappers_map_the_errors():
    import svgpu
    assert svgpu.poly_div_linear_device is not None
    s = svgpu.ResidentBases.__new__(svgpu.ResidentBases)  # no device here: a number no set carries
    s.handle = _UNKNOWN
    try:
        one = np.zeros((1, 4), np.uint64)
        with pytest.raises(svgpu.EmptyError, match="empty"):
            s.open_arrays(np.zeros((0, 4), np.uint64), 5)
        with pytest.raises(svgpu.ArgumentError, match="bad form"):
            s.open_arrays(one, 5, form=5)
        for form in (svgpu.SV_CANONICAL, svgpu.SV_MONTGOMERY):
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                s.open_arrays(one, b.R, form=form)
            with pytest.raises(svgpu.ArgumentError, match="unknown base set handle 424242"):
                s.open_arrays(one, b.R - 1, form=form)
        with pytest.raises(svgpu.ArgumentError, match="unknown base set handle"):
            s.open_arrays(one, 5, offset=(1 << 64) - 1)
        with pytest.raises(svgpu.ArgumentError):
            s.open_arrays(one, 1 << 256)
        with pytest.raises(svgpu.ArgumentError):
            s.open_arrays(one, -1)
    finally:
        s.handle = None
    with pytest.raises(svgpu.ArgumentError, match="closed"):
        s.open_arrays(np.zeros((1, 4), np.uint64), 5)
