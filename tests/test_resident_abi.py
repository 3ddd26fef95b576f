"""Resident base sets (sv_bn254_g1_bases_* / sv_bn254_g1_msm_bases*, include/svgpu.h): every
argument, emptiness, length and handle rule returns its code and message before anything touches a
device, so all of it is checked here without a GPU."""
import ctypes

import numpy as np

from svgpu import _lib

_BUF = np.zeros(64, np.uint64)
_OUT = _lib.sv_g1_affine()
_PART = _lib.sv_g1_jacobian()


def _h():
    return ctypes.c_uint64(0)


def test_create_arguments_rejected_without_compute():
    p = _BUF.ctypes.data
    for create, extra in ((_lib.lib.sv_bn254_g1_bases_create, ()), (_lib.lib.sv_bn254_g1_bases_create_device, (None,))):
        h = _h()
        assert create(p, 1, 9, 0, *extra, ctypes.byref(h)) == _lib.SV_ERR_ARG
        assert "bad form" in _lib.last_error()
        assert create(None, 1, 0, 0, *extra, ctypes.byref(h)) == _lib.SV_ERR_ARG
        assert "null" in _lib.last_error()
        assert create(p, 1, 0, 0, *extra, None) == _lib.SV_ERR_ARG
        # a bad form wins over emptiness, emptiness over the length (sv_bn254_g1_table_create's order)
        assert create(p, 0, 9, 0, *extra, ctypes.byref(h)) == _lib.SV_ERR_ARG
        assert create(p, 0, 0, 0, *extra, ctypes.byref(h)) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert create(p, (1 << 26) + 1, 1, 0, *extra, ctypes.byref(h)) == _lib.SV_ERR_LEN
        assert "2^26" in _lib.last_error()
        assert h.value == 0


def test_msm_call_arguments_rejected_without_compute():
    p = _BUF.ctypes.data
    host = lambda hd, off, sc, n, form, out=ctypes.byref(_OUT): _lib.lib.sv_bn254_g1_msm_bases(hd, off, sc, n, form, out)
    dev = lambda hd, off, sc, n, form, out=ctypes.byref(_PART): _lib.lib.sv_bn254_g1_msm_bases_device(
        hd, off, sc, n, form, None, out)
    for call in (host, dev):
        assert call(1, 0, p, 1, 7) == _lib.SV_ERR_ARG
        assert "bad form" in _lib.last_error()
        assert call(1, 0, None, 1, 0) == _lib.SV_ERR_ARG
        assert call(1, 0, p, 1, 0, None) == _lib.SV_ERR_ARG
        assert call(1, 0, p, 0, 7) == _lib.SV_ERR_ARG           # form before emptiness
        assert call(1, 0, p, 0, 0) == _lib.SV_ERR_EMPTY
        assert "pairs should not be empty" in _lib.last_error()
        assert call(1, 0, p, (1 << 26) + 1, 0) == _lib.SV_ERR_LEN
        # an unknown handle, named in the message; checked before any device is looked for
        assert call(424242, 0, p, 1, 0) == _lib.SV_ERR_ARG
        assert "unknown base set handle 424242" in _lib.last_error()
        # offsets near 2^64: the range check must not wrap into the handle's range
        assert call(424242, (1 << 64) - 1, p, 2, 1) == _lib.SV_ERR_ARG


def test_unknown_handles_and_double_destroy():
    assert _lib.lib.sv_bn254_g1_bases_destroy(123456789) == _lib.SV_ERR_ARG
    assert "unknown base set handle 123456789" in _lib.last_error()
    assert _lib.lib.sv_bn254_g1_bases_destroy(123456789) == _lib.SV_ERR_ARG
    n, d, by = ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_uint64(7)
    assert _lib.lib.sv_bn254_g1_bases_info(55, ctypes.byref(n), ctypes.byref(d), ctypes.byref(by)) == _lib.SV_ERR_ARG
    assert "unknown base set handle 55" in _lib.last_error()
    assert (n.value, d.value, by.value) == (7, 7, 7)
    # a base-set number is no base-table handle either
    assert _lib.lib.sv_bn254_g1_table_destroy(55) == _lib.SV_ERR_ARG
    assert "unknown base table" in _lib.last_error()


def test_python_wrapper_is_exported_and_maps_errors():
    import pytest
    import svgpu
    assert svgpu.ResidentBases is svgpu.loader.ResidentBases
    with pytest.raises(svgpu.EmptyError):
        svgpu.ResidentBases(np.zeros((0, 8), np.uint64))
    with pytest.raises(svgpu.ArgumentError):
        svgpu.ResidentBases(np.zeros((1, 8), np.uint64), form=5)
