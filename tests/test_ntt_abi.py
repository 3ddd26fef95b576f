"""Fr NTT (sv_bn254_fr_root_of_unity, sv_bn254_fr_ntt_device; include/svgpu.h) without a GPU: the
domain's roots against Python-int arithmetic, and every argument rule of the transform in the
documented order -- form / direction / null / alignment, empty, length, shift not reduced, shift
zero, partial overlap -- each with its code and message before anything touches a device.  No call
below except the last test's is valid through rule 6, so none reaches a device where there is one."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c
_BUF = np.zeros(64, np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15          # 16-byte aligned, room for 8 elements behind it
_ONE = enc.fe_struct(1)
_G = enc.fe_struct(5)
_G_BAD = [enc.fe_struct(v) for v in (b.R, b.R + 5, (1 << 256) - 1)]
_ZERO = enc.fe_struct(0)
FWD, INV = _lib.SV_NTT_FORWARD, _lib.SV_NTT_INVERSE


def _ntt(d_in=_P, d_out=_P, log_n=1, count=1, direction=FWD, shift=None, form=0):
    return _lib.lib.sv_bn254_fr_ntt_device(d_in, d_out, log_n, count, direction,
                                           ctypes.byref(shift) if shift is not None else None, form, 0, None)


def _root(k, form):
    out = _lib.sv_fe()
    rc = _lib.lib.sv_bn254_fr_root_of_unity(k, form, ctypes.byref(out))
    return rc, enc.limbs_to_int(list(out.l))


def test_roots_of_unity_are_the_reference_domain():
    import svgpu
    assert pow(ROOT_OF_UNITY, 1 << 27, b.R) == b.R - 1         # the constant itself: order exactly 2^28
    assert ROOT_OF_UNITY == pow(7, (b.R - 1) >> 28, b.R)
    assert svgpu.root_of_unity(28) == ROOT_OF_UNITY
    assert svgpu.root_of_unity(0) == 1
    assert svgpu.root_of_unity(1) == b.R - 1
    w = [svgpu.root_of_unity(k) for k in range(29)]
    for k in range(1, 29):
        assert pow(w[k], 1 << (k - 1), b.R) == b.R - 1, k
        assert w[k - 1] == w[k] * w[k] % b.R, k
        assert w[k] == pow(ROOT_OF_UNITY, 1 << (28 - k), b.R), k


def test_root_of_unity_forms_and_rejections():
    import svgpu
    for k in (0, 1, 5, 26, 28):
        rc, canonical = _root(k, _lib.SV_CANONICAL)
        assert rc == _lib.SV_OK
        rc, mont = _root(k, _lib.SV_MONTGOMERY)
        assert rc == _lib.SV_OK
        assert mont == (canonical << 256) % b.R, k
        assert svgpu.root_of_unity(k, form=_lib.SV_MONTGOMERY) == canonical
    rc, _ = _root(29, 0)
    assert rc == _lib.SV_ERR_ARG and "28" in _lib.last_error()
    rc, _ = _root((1 << 32) - 1, 1)
    assert rc == _lib.SV_ERR_ARG
    rc, _ = _root(3, 7)
    assert rc == _lib.SV_ERR_ARG and "bad form" in _lib.last_error()
    assert _lib.lib.sv_bn254_fr_root_of_unity(3, 0, None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    with pytest.raises(svgpu.ArgumentError):
        svgpu.root_of_unity(29)


def test_form_direction_null_and_alignment_come_first():
    assert _ntt(form=7) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    for d in (2, -1, 77):
        assert _ntt(direction=d) == _lib.SV_ERR_ARG
        assert "direction" in _lib.last_error()
    assert _ntt(d_in=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert _ntt(d_out=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    for off in (8, 4, 1):
        assert _ntt(d_in=_P + off) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
        assert _ntt(d_out=_P + off) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
    # ... before emptiness, the length and the shift; the form before the direction
    assert _ntt(form=7, direction=9, count=0) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    assert _ntt(direction=9, count=0, log_n=40, shift=_G_BAD[0]) == _lib.SV_ERR_ARG
    assert "direction" in _lib.last_error()
    assert _ntt(d_in=None, count=0) == _lib.SV_ERR_ARG
    assert _ntt(d_out=_P + 8, log_n=27, shift=_ZERO) == _lib.SV_ERR_ARG
    assert "aligned" in _lib.last_error()


def test_empty_then_length_then_shift():
    for form in (0, 1):
        for d in (FWD, INV):
            assert _ntt(count=0, direction=d, form=form) == _lib.SV_ERR_EMPTY
            assert "empty" in _lib.last_error()
            assert _ntt(count=0, log_n=27, shift=_G_BAD[0], direction=d, form=form) == _lib.SV_ERR_EMPTY
            assert _ntt(log_n=27, direction=d, form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()
            assert _ntt(log_n=(1 << 32) - 1, direction=d, form=form) == _lib.SV_ERR_LEN
            assert _ntt(log_n=27, shift=_G_BAD[0], direction=d, form=form) == _lib.SV_ERR_LEN   # the length before the shift
            # count * 2^log_n may reach 2^28 and not pass it
            for log_n, count in ((26, 5), (20, 257), (0, (1 << 28) + 1), (3, 1 << 62), (1, (1 << 64) - 1)):
                assert _ntt(log_n=log_n, count=count, shift=_ZERO, direction=d, form=form) == _lib.SV_ERR_LEN, (log_n, count)
                assert "2^28" in _lib.last_error()
            for bad in _G_BAD:
                assert _ntt(shift=bad, direction=d, form=form) == _lib.SV_ERR_ARG
                assert "not reduced" in _lib.last_error()
                assert _ntt(log_n=26, count=4, shift=bad, d_out=_P + 32, direction=d, form=form) == _lib.SV_ERR_ARG
                assert "not reduced" in _lib.last_error()                                       # before the overlap
            assert _ntt(shift=_ZERO, direction=d, form=form) == _lib.SV_ERR_ARG
            assert "zero" in _lib.last_error()
            assert _ntt(shift=_ZERO, d_out=_P + 32, direction=d, form=form) == _lib.SV_ERR_ARG  # before the overlap
            assert "zero" in _lib.last_error()


def test_partial_overlap_is_refused():
    """Two elements at _P (log_n = 1): a d_out one element behind or in front of d_in shares one of
    them; two elements away it is disjoint, and d_out == d_in is in place.  The calls that pass the
    rule would reach the device, so they are only made under the no-GPU test below."""
    for form in (0, 1):
        assert _ntt(d_in=_P + 64, d_out=_P + 96, form=form) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()
        assert _ntt(d_in=_P + 64, d_out=_P + 32, form=form, shift=_G) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()
        assert _ntt(d_in=_P + 64, d_out=_P + 80, form=form, direction=INV) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()
        # a batch: 3 transforms of 2 elements, shifted by one whole transform
        assert _ntt(d_in=_P, d_out=_P + 64, count=3, form=form) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    """Past every rule -- in place, disjoint ranges on either side, a shift of 1, a coset -- a machine
    without a GPU answers SV_ERR_DEVICE, like every other compute entry point."""
    for form in (0, 1):
        assert _ntt(form=form) == _lib.SV_ERR_DEVICE                                   # in place
        assert _ntt(d_in=_P + 64, d_out=_P, form=form) == _lib.SV_ERR_DEVICE           # ends right before d_in
        assert _ntt(d_in=_P, d_out=_P + 64, form=form, direction=INV) == _lib.SV_ERR_DEVICE
        assert _ntt(log_n=0, count=1, shift=_ONE, form=form) == _lib.SV_ERR_DEVICE
        assert _ntt(log_n=26, count=4, shift=_G, form=form) == _lib.SV_ERR_DEVICE      # exactly 2^28 elements
        assert _ntt(log_n=0, count=1 << 28, form=form) == _lib.SV_ERR_DEVICE


def test_python_wrapper_is_exported():
    import svgpu
    assert callable(svgpu.ntt_device) and callable(svgpu.root_of_unity)
    assert (_lib.SV_NTT_MAX_LOG, _lib.SV_NTT_FORWARD, _lib.SV_NTT_INVERSE) == (26, 0, 1)
