"""The extended-domain calls (sv_bn254_fr_coset_lde_device, sv_bn254_fr_quotient_coeffs_device;
include/svgpu.h) without a GPU: every argument rule of both in the documented order, each with its
code and message before anything touches a device, and svgpu.extended_k against halo2's table.
LDE: form / null / alignment, empty, length (log_ext, K, count 2^K), shift not reduced, shift zero,
overlap.  Quotient: form / null (a NULL shift included) / alignment, empty, length (log_ext, K, then
pieces), shift not reduced, shift zero, coset meets the domain, overlap.  No call below except the
last test's is valid through its last rule, so none reaches a device where there is one."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

R = b.R
ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c
ZETA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
_BUF = np.zeros(160, np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15          # 16-byte aligned, room for 38 elements behind it
_G_BAD = [enc.fe_struct(v) for v in (R, R + 5, (1 << 256) - 1)]
_ZERO = enc.fe_struct(0)
E = 32                                      # bytes per element


def _fe(v, form):
    return enc.fr_struct(v, form)


def _lde(d_coeffs=_P, d_evals=_P + 2 * E, log_n=1, log_ext=1, count=1, shift=None, form=0):
    return _lib.lib.sv_bn254_fr_coset_lde_device(d_coeffs, d_evals, log_n, log_ext, count,
                                                 ctypes.byref(shift) if shift is not None else None, form, 0, None)


_UNSET = object()


def _quot(d_numer=_P, d_out=_P, log_n=1, log_ext=1, pieces=1, shift=_UNSET, form=0):
    if shift is _UNSET:
        shift = _fe(ZETA, form)
    return _lib.lib.sv_bn254_fr_quotient_coeffs_device(d_numer, d_out, log_n, log_ext, pieces,
                                                       ctypes.byref(shift) if shift is not None else None, form, 0,
                                                       None)


def _root(k):
    return pow(ROOT_OF_UNITY, 1 << (28 - k), R)


def test_zeta_is_the_cube_root_the_header_names():
    assert ZETA == pow(7, (R - 1) // 3, R)
    assert ZETA != 1 and pow(ZETA, 3, R) == 1 and (ZETA * ZETA + ZETA + 1) % R == 0
    assert _lib.SV_EXT_LOG_MAX == 8


@pytest.mark.parametrize("degree,ext", [(2, 0), (3, 1), (4, 2), (5, 2), (6, 3), (9, 3), (10, 4)])
def test_extended_k_is_halo2s_rule(degree, ext):
    import svgpu
    for k in (0, 1, 4, 17, 22):
        K = svgpu.extended_k(k, degree)
        assert K - k == ext
        assert (1 << K) >= (1 << k) * (degree - 1) and (K == k or (1 << (K - 1)) < (1 << k) * (degree - 1))
    with pytest.raises(svgpu.LengthError):
        svgpu.extended_k(3, 1)


# ---- coset_lde ----
def test_lde_form_null_and_alignment_come_first():
    assert _lde(form=7) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    assert _lde(d_coeffs=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert _lde(d_evals=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    for off in (8, 4, 1):
        assert _lde(d_coeffs=_P + off) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
        assert _lde(d_evals=_P + 2 * E + off) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
    # ... before emptiness, the length and the shift
    assert _lde(form=7, d_coeffs=None, count=0) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    assert _lde(d_coeffs=None, count=0, log_ext=9) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert _lde(d_evals=_P + 8, count=0, log_n=27, shift=_ZERO) == _lib.SV_ERR_ARG
    assert "aligned" in _lib.last_error()


def test_lde_empty_then_length_then_shift_then_overlap():
    for form in (0, 1):
        assert _lde(count=0, form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _lde(count=0, log_ext=9, shift=_G_BAD[0], form=form) == _lib.SV_ERR_EMPTY      # before the length
        # the length: log_ext, K, count 2^K
        for log_n, log_ext, count in ((1, 9, 1), (1, (1 << 32) - 1, 1), (26, 1, 1), (19, 8, 1), (27, 0, 1),
                                      ((1 << 32) - 1, 0, 1), ((1 << 32) - 1, 1, 1), (20, 2, 65), (24, 2, 5),
                                      (0, 0, (1 << 28) + 1), (1, 2, 1 << 62), (0, 1, (1 << 64) - 1)):
            assert _lde(log_n=log_n, log_ext=log_ext, count=count, form=form) == _lib.SV_ERR_LEN, (log_n, log_ext, count)
            assert "2^28" in _lib.last_error()
            assert _lde(log_n=log_n, log_ext=log_ext, count=count, shift=_G_BAD[0], d_evals=_P + E,
                        form=form) == _lib.SV_ERR_LEN                                           # before the shift
        for bad in _G_BAD:
            assert _lde(shift=bad, form=form) == _lib.SV_ERR_ARG
            assert "not reduced" in _lib.last_error()
            assert _lde(shift=bad, d_evals=_P + E, form=form) == _lib.SV_ERR_ARG                # before the overlap
            assert "not reduced" in _lib.last_error()
        assert _lde(shift=_ZERO, form=form) == _lib.SV_ERR_ARG
        assert "zero" in _lib.last_error()
        assert _lde(shift=_ZERO, d_evals=_P + E, form=form) == _lib.SV_ERR_ARG                  # before the overlap
        assert "zero" in _lib.last_error()


def test_lde_any_overlap_is_refused():
    """log_n = 1, log_ext = 1: two coefficients at d_coeffs, four evaluations at d_evals.  There is no
    in place: equal pointers are an overlap too."""
    g = _fe(5, 0)
    for form in (0, 1):
        for c_off, e_off in ((0, 0), (0, 1), (4, 1), (4, 3), (4, 5), (3, 0), (1, 0)):
            assert _lde(d_coeffs=_P + c_off * E, d_evals=_P + e_off * E, form=form, shift=g if form == 0 else None) \
                == _lib.SV_ERR_ARG, (c_off, e_off)
            assert "overlaps" in _lib.last_error()
        # a batch of 3: 6 coefficients, 12 evaluations
        assert _lde(d_coeffs=_P + 11 * E, d_evals=_P, count=3, form=form) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()
        assert _lde(d_coeffs=_P, d_evals=_P + 5 * E, count=3, form=form) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()
        # log_ext = 0 is no exception
        assert _lde(log_ext=0, d_evals=_P, form=form) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()


# ---- quotient_coeffs ----
def test_quotient_form_null_and_alignment_come_first():
    assert _quot(form=7, shift=_ZERO) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    assert _quot(d_numer=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert _quot(d_out=None) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert _quot(shift=None) == _lib.SV_ERR_ARG                    # a coset is required
    assert "null" in _lib.last_error()
    for off in (8, 4, 1):
        assert _quot(d_numer=_P + off) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
        assert _quot(d_out=_P + off) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
    assert _quot(shift=None, pieces=0, log_ext=9) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()
    assert _quot(d_out=_P + 8, pieces=0, log_n=27, shift=_ZERO) == _lib.SV_ERR_ARG
    assert "aligned" in _lib.last_error()


def test_quotient_empty_then_length_then_shift_then_domain_then_overlap():
    for form in (0, 1):
        assert _quot(pieces=0, form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _quot(pieces=0, log_ext=9, shift=_G_BAD[0], form=form) == _lib.SV_ERR_EMPTY      # before the length
        for log_n, log_ext in ((1, 9), (1, (1 << 32) - 1), (26, 1), (19, 8), (27, 0), ((1 << 32) - 1, 0),
                               ((1 << 32) - 1, 1)):
            assert _quot(log_n=log_n, log_ext=log_ext, form=form) == _lib.SV_ERR_LEN, (log_n, log_ext)
            assert "2^26" in _lib.last_error()
            assert _quot(log_n=log_n, log_ext=log_ext, pieces=1 << 40, shift=_G_BAD[0], form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()                                                  # K before the pieces
        for log_ext, pieces in ((0, 2), (1, 3), (2, 5), (8, 257), (3, 1 << 63), (0, (1 << 64) - 1)):
            assert _quot(log_ext=log_ext, pieces=pieces, form=form) == _lib.SV_ERR_LEN, (log_ext, pieces)
            assert "pieces" in _lib.last_error()
            assert _quot(log_ext=log_ext, pieces=pieces, shift=_G_BAD[0], form=form) == _lib.SV_ERR_LEN   # before the shift
        for bad in _G_BAD:
            assert _quot(shift=bad, form=form) == _lib.SV_ERR_ARG
            assert "not reduced" in _lib.last_error()
            assert _quot(shift=bad, d_out=_P + E, form=form) == _lib.SV_ERR_ARG
            assert "not reduced" in _lib.last_error()
        assert _quot(shift=_ZERO, form=form) == _lib.SV_ERR_ARG
        assert "zero" in _lib.last_error()
        assert _quot(shift=_ZERO, d_out=_P + E, form=form) == _lib.SV_ERR_ARG
        assert "zero" in _lib.last_error()
        # g^(2^K) == 1: 1, r - 1, omega_K^3 at K = 2 and K = 12; before the overlap
        for log_n, log_ext in ((1, 1), (9, 3)):
            K = log_n + log_ext
            for g in (1, R - 1, pow(_root(K), 3, R), _root(K)):
                assert _quot(log_n=log_n, log_ext=log_ext, shift=_fe(g, form), form=form) == _lib.SV_ERR_ARG, (K, g)
                assert "coset meets the domain" in _lib.last_error()
                assert _quot(log_n=log_n, log_ext=log_ext, shift=_fe(g, form), d_out=_P + E, form=form) == _lib.SV_ERR_ARG
                assert "coset meets the domain" in _lib.last_error()
        # log_n = 1, log_ext = 1: four evaluations in, pieces * 2 coefficients out
        for n_off, o_off, pieces in ((4, 3, 1), (4, 5, 1), (4, 7, 2), (4, 1, 2), (0, 3, 2), (4, 2, 2)):
            assert _quot(d_numer=_P + n_off * E, d_out=_P + o_off * E, pieces=pieces, form=form) == _lib.SV_ERR_ARG, \
                (n_off, o_off, pieces)
            assert "overlaps" in _lib.last_error()


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    """Past every rule a machine without a GPU answers SV_ERR_DEVICE, like every other compute entry
    point: disjoint ranges on either side, the limits themselves, in place for the quotient, and a
    shift one squaring outside the domain (omega_(K+1))."""
    for form in (0, 1):
        assert _lde(form=form) == _lib.SV_ERR_DEVICE                                         # evals right behind coeffs
        assert _lde(d_coeffs=_P + 4 * E, d_evals=_P, form=form) == _lib.SV_ERR_DEVICE         # ... right before
        assert _lde(log_n=0, log_ext=0, d_evals=_P + E, form=form) == _lib.SV_ERR_DEVICE
        assert _lde(log_n=18, log_ext=8, d_evals=_P + (1 << 18) * E, shift=_fe(ZETA, form), form=form) == _lib.SV_ERR_DEVICE
        assert _lde(log_n=24, log_ext=2, count=4, d_evals=_P + (1 << 26) * E, form=form) == _lib.SV_ERR_DEVICE
        assert _quot(form=form) == _lib.SV_ERR_DEVICE                                        # in place
        assert _quot(d_numer=_P + 4 * E, d_out=_P, pieces=2, form=form) == _lib.SV_ERR_DEVICE
        assert _quot(d_numer=_P, d_out=_P + 4 * E, pieces=2, form=form) == _lib.SV_ERR_DEVICE
        assert _quot(d_numer=_P + 4 * E, d_out=_P + 2 * E, pieces=1, form=form) == _lib.SV_ERR_DEVICE
        assert _quot(log_n=18, log_ext=8, pieces=256, form=form) == _lib.SV_ERR_DEVICE
        assert _quot(shift=_fe(_root(3), form), form=form) == _lib.SV_ERR_DEVICE             # omega_(K+1), K = 2
        assert _quot(shift=_fe(ZETA * ZETA % R, form), form=form) == _lib.SV_ERR_DEVICE


def test_python_wrappers_are_exported():
    import svgpu
    for name in ("coset_lde_device", "quotient_coeffs_device", "extended_k", "commit_pieces"):
        assert callable(getattr(svgpu, name)), name
