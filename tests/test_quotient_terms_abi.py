"""The terms calls (sv_bn254_fr_permutation_terms_device, sv_bn254_fr_lookup_terms_device;
include/svgpu.h) without a GPU: every argument rule of both in the documented order, each with its
code and message before anything touches a device.
  1 bad form; 2 a null d_out, pointer array, entry, l column, s, beta, gamma or y; 3 chunk == 0;
  4 alignment; 5 empty; 6 log_ext; 7 K; 8 a count above its cap; 9 a scalar not reduced; 10 a zero
  shift; 11 last_rotation; 12 the overlaps.
No call below except the last tests' is valid through its last rule, so none reaches a device where
there is one."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

R = b.R
E = 32                                       # bytes per element
_BUF = np.zeros(4 * 164, np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15           # 16-byte aligned, room for 163 elements (40 columns) behind it
_BAD = [enc.fe_struct(v) for v in (R, R + 5, (1 << 256) - 1)]
_ZERO = enc.fe_struct(0)
_UNSET = object()
N = 4                                        # log_n = 1, log_ext = 1: four rows per column


def _fe(v, form=0):
    return enc.fr_struct(v, form)


def _col(i):
    """The i-th disjoint column of N rows in the buffer."""
    return _P + i * N * E


def _ptrs(values):
    arr = (ctypes.c_void_p * max(len(values), 1))()
    for j, v in enumerate(values):
        arr[j] = v
    return arr


def _ref(x):
    return ctypes.byref(x) if x is not None else None


# columns of the default call: 0 out, 1 acc, 2..4 l, 5.. the rest
def _perm(m=2, chunk=1, cols=_UNSET, sigmas=_UNSET, s=_UNSET, z=_UNSET, l0=_col(2), l_last=_col(3), l_active=_col(4),
          beta=_UNSET, gamma=_UNSET, y=_UNSET, shift=None, last_rotation=-1, acc=_col(1), out=_col(0), log_n=1,
          log_ext=1, form=0):
    # the buffer holds three columns of each kind: entries beyond them repeat
    cols = _ptrs([_col(5 + j % 3) for j in range(m)]) if cols is _UNSET else cols
    sigmas = _ptrs([_col(8 + j % 3) for j in range(m)]) if sigmas is _UNSET else sigmas
    z = _ptrs([_col(11 + j % 3) for j in range(m)]) if z is _UNSET else z
    s = (_lib.sv_fe * max(m, 1))(*[_fe(3 + j, form) for j in range(m)]) if s is _UNSET else s
    beta, gamma, y = (_fe(v, form) if x is _UNSET else x for v, x in ((5, beta), (6, gamma), (7, y)))
    return _lib.lib.sv_bn254_fr_permutation_terms_device(cols, sigmas, s, m, chunk, z, l0, l_last, l_active,
                                                         _ref(beta), _ref(gamma), _ref(y), _ref(shift), last_rotation,
                                                         acc, out, log_n, log_ext, form, 0, None)


def _lookup_array(n, first=5):
    arr = (_lib.sv_fr_lookup * max(n, 1))()
    for j in range(n):                       # the buffer holds two lookups: descriptors beyond them repeat
        (arr[j].d_z, arr[j].d_permuted_input, arr[j].d_permuted_table, arr[j].d_input,
         arr[j].d_table) = (_col(first + 5 * (j % 2) + i) for i in range(5))
    return arr


def _look(n=1, lookups=_UNSET, l0=_col(2), l_last=_col(3), l_active=_col(4), beta=_UNSET, gamma=_UNSET, y=_UNSET,
          acc=_col(1), out=_col(0), log_n=1, log_ext=1, form=0):
    lookups = _lookup_array(n) if lookups is _UNSET else lookups
    beta, gamma, y = (_fe(v, form) if x is _UNSET else x for v, x in ((5, beta), (6, gamma), (7, y)))
    return _lib.lib.sv_bn254_fr_lookup_terms_device(lookups, n, l0, l_last, l_active, _ref(beta), _ref(gamma), _ref(y),
                                                    acc, out, log_n, log_ext, form, 0, None)


def _is(rc, code, word):
    assert rc == code, (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def test_caps_are_pinned():
    assert _lib.SV_TERMS_COLUMNS_MAX == 64 and _lib.SV_TERMS_LOOKUPS_MAX == 16
    h = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "svgpu.h")).read()
    assert "#define SV_TERMS_COLUMNS_MAX 64" in h and "#define SV_TERMS_LOOKUPS_MAX 16" in h
    assert ctypes.sizeof(_lib.sv_fr_lookup) == 40


# ---- permutation terms ----
def test_permutation_rule_1_form_and_rule_2_nulls():
    _is(_perm(form=7, out=None, chunk=0), _lib.SV_ERR_ARG, "bad form")           # before every other rule
    for kw in ("out", "l0", "l_last", "l_active", "beta", "gamma", "y", "cols", "sigmas", "z", "s"):
        _is(_perm(**{kw: None}), _lib.SV_ERR_ARG, "null")
        _is(_perm(**{kw: None}, chunk=0, m=0, log_ext=9), _lib.SV_ERR_ARG, "null")    # before rules 3, 5, 6
    for kw, base in (("cols", 5), ("sigmas", 8), ("z", 11)):
        for hole in (0, 1):
            arr = _ptrs([None if j == hole else _col(base + j) for j in range(2)])
            _is(_perm(**{kw: arr}), _lib.SV_ERR_ARG, "null")
            _is(_perm(**{kw: arr}, out=_col(0) + 8), _lib.SV_ERR_ARG, "null")    # before the alignment
    # d_acc_in may be null, and a z entry beyond ceil(m / chunk) is not looked at: a later rule answers
    two = _ptrs([_col(11), None])
    _is(_perm(acc=None, z=two, chunk=2, last_rotation=0), _lib.SV_ERR_ARG, "last_rotation")


def test_permutation_rule_3_chunk_and_rule_4_alignment():
    _is(_perm(chunk=0), _lib.SV_ERR_ARG, "chunk")
    _is(_perm(chunk=0, out=_col(0) + 8, m=0, log_ext=9), _lib.SV_ERR_ARG, "chunk")     # before rules 4, 5, 6
    for off in (8, 4, 1):
        for kw in ("out", "acc", "l0", "l_last", "l_active"):
            _is(_perm(**{kw: _col(20) + off}), _lib.SV_ERR_ARG, "aligned")
        for kw, base in (("cols", 5), ("sigmas", 8), ("z", 11)):
            arr = _ptrs([_col(base), _col(base + 1) + off])
            _is(_perm(**{kw: arr}), _lib.SV_ERR_ARG, "aligned")
    _is(_perm(out=_col(0) + 8, m=0, log_ext=9), _lib.SV_ERR_ARG, "aligned")            # before rules 5, 6


def test_permutation_rules_5_to_8_empty_then_lengths():
    for form in (0, 1):
        _is(_perm(m=0, form=form), _lib.SV_ERR_EMPTY, "empty")
        _is(_perm(m=0, log_ext=9, beta=_BAD[0], form=form), _lib.SV_ERR_EMPTY, "empty")     # before the length
        for log_ext in (9, (1 << 32) - 1):
            _is(_perm(log_ext=log_ext, form=form), _lib.SV_ERR_LEN, "log_ext")
            _is(_perm(log_ext=log_ext, log_n=27, m=65, form=form), _lib.SV_ERR_LEN, "log_ext")  # before K and the cap
        for log_n, log_ext in ((26, 1), (19, 8), (27, 0), ((1 << 32) - 1, 0), ((1 << 32) - 1, 1)):
            _is(_perm(log_n=log_n, log_ext=log_ext, form=form), _lib.SV_ERR_LEN, "2^26")
            _is(_perm(log_n=log_n, log_ext=log_ext, m=65, beta=_BAD[0], form=form), _lib.SV_ERR_LEN, "2^26")
        for m in (65, 1000):
            _is(_perm(m=m, form=form), _lib.SV_ERR_LEN, "at most 64")
            _is(_perm(m=m, gamma=_BAD[1], last_rotation=0, form=form), _lib.SV_ERR_LEN, "at most 64")  # before 9, 11


def test_permutation_rules_9_to_11_scalars_shift_rotation():
    for form in (0, 1):
        for bad in _BAD:
            for kw in ("beta", "gamma", "y", "shift"):
                _is(_perm(**{kw: bad}, form=form), _lib.SV_ERR_ARG, "not reduced")
                _is(_perm(**{kw: bad}, last_rotation=0, out=_col(5), form=form), _lib.SV_ERR_ARG, "not reduced")
            for j in (0, 1):
                s = (_lib.sv_fe * 2)(*[bad if i == j else _fe(3, form) for i in range(2)])
                _is(_perm(s=s, form=form), _lib.SV_ERR_ARG, "not reduced")
                _is(_perm(s=s, shift=_ZERO, form=form), _lib.SV_ERR_ARG, "not reduced")    # before the zero shift
        _is(_perm(shift=_ZERO, form=form), _lib.SV_ERR_ARG, "zero")
        _is(_perm(shift=_ZERO, last_rotation=0, out=_col(5), form=form), _lib.SV_ERR_ARG, "zero")   # before 11, 12
        # -n < last_rotation < 0 with n = 2^log_n
        for log_n, r in ((1, 0), (1, 1), (1, -2), (1, -3), (3, -8), (3, 5), (1, -(1 << 31)), (1, (1 << 31) - 1)):
            _is(_perm(log_n=log_n, log_ext=0, last_rotation=r, form=form), _lib.SV_ERR_ARG, "last_rotation")
            _is(_perm(log_n=log_n, log_ext=0, last_rotation=r, out=_col(5), form=form), _lib.SV_ERR_ARG,
                "last_rotation")                                                            # before the overlap


def test_permutation_rule_12_overlaps():
    for form in (0, 1):
        for i in (1, 2, 3, 4, 5, 6, 8, 9, 11, 12):      # acc, the l columns, both columns, sigmas and z
            for off in (-3, -1, 1, 3):                  # rows: partial overlap on either side
                _is(_perm(out=_col(i) + off * E, form=form), _lib.SV_ERR_ARG, "overlaps")
        for i in (2, 3, 4, 5, 6, 8, 9, 11, 12):         # equal pointers: in place is d_acc_in only
            _is(_perm(out=_col(i), form=form), _lib.SV_ERR_ARG, "overlaps")
        _is(_perm(out=_col(12), acc=_col(12), form=form), _lib.SV_ERR_ARG, "overlaps")     # in place, but onto a z


# ---- lookup terms ----
def test_lookup_rule_1_form_and_rule_2_nulls():
    _is(_look(form=7, out=None), _lib.SV_ERR_ARG, "bad form")
    for kw in ("out", "l0", "l_last", "l_active", "beta", "gamma", "y", "lookups"):
        _is(_look(**{kw: None}), _lib.SV_ERR_ARG, "null")
        _is(_look(**{kw: None}, n=0, log_ext=9), _lib.SV_ERR_ARG, "null")
    for field in ("d_z", "d_permuted_input", "d_permuted_table", "d_input", "d_table"):
        for hole in (0, 1):
            arr = _lookup_array(2)
            setattr(arr[hole], field, None)
            _is(_look(n=2, lookups=arr), _lib.SV_ERR_ARG, "null")
            _is(_look(n=2, lookups=arr, out=_col(0) + 8), _lib.SV_ERR_ARG, "null")
    _is(_look(acc=None, n=0), _lib.SV_ERR_EMPTY, "empty")                                   # d_acc_in may be null


def test_lookup_rule_4_alignment():
    for off in (8, 4, 1):
        for kw in ("out", "acc", "l0", "l_last", "l_active"):
            _is(_look(**{kw: _col(20) + off}), _lib.SV_ERR_ARG, "aligned")
        for field in ("d_z", "d_permuted_input", "d_permuted_table", "d_input", "d_table"):
            arr = _lookup_array(2)
            setattr(arr[1], field, getattr(arr[1], field) + off)
            _is(_look(n=2, lookups=arr), _lib.SV_ERR_ARG, "aligned")
    _is(_look(out=_col(0) + 8, n=0, log_ext=9), _lib.SV_ERR_ARG, "aligned")


def test_lookup_rules_5_to_9_empty_lengths_scalars():
    for form in (0, 1):
        _is(_look(n=0, form=form), _lib.SV_ERR_EMPTY, "empty")
        _is(_look(n=0, log_ext=9, beta=_BAD[0], form=form), _lib.SV_ERR_EMPTY, "empty")
        for log_ext in (9, (1 << 32) - 1):
            _is(_look(log_ext=log_ext, form=form), _lib.SV_ERR_LEN, "log_ext")
            _is(_look(log_ext=log_ext, log_n=27, n=17, form=form), _lib.SV_ERR_LEN, "log_ext")
        for log_n, log_ext in ((26, 1), (19, 8), (27, 0), ((1 << 32) - 1, 0), ((1 << 32) - 1, 1)):
            _is(_look(log_n=log_n, log_ext=log_ext, form=form), _lib.SV_ERR_LEN, "2^26")
            _is(_look(log_n=log_n, log_ext=log_ext, n=17, beta=_BAD[0], form=form), _lib.SV_ERR_LEN, "2^26")
        for n in (17, 1000):
            _is(_look(n=n, form=form), _lib.SV_ERR_LEN, "at most 16")
            _is(_look(n=n, y=_BAD[2], form=form), _lib.SV_ERR_LEN, "at most 16")
        for bad in _BAD:
            for kw in ("beta", "gamma", "y"):
                _is(_look(**{kw: bad}, form=form), _lib.SV_ERR_ARG, "not reduced")
                _is(_look(**{kw: bad}, out=_col(5), form=form), _lib.SV_ERR_ARG, "not reduced")   # before the overlap


def test_lookup_rule_12_overlaps():
    for form in (0, 1):
        for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14):
            for off in (-3, -1, 1, 3):
                _is(_look(n=2, out=_col(i) + off * E, form=form), _lib.SV_ERR_ARG, "overlaps")
        for i in (2, 3, 4, 5, 6, 7, 8, 9, 10, 14):
            _is(_look(n=2, out=_col(i), form=form), _lib.SV_ERR_ARG, "overlaps")
        _is(_look(out=_col(7), acc=_col(7), form=form), _lib.SV_ERR_ARG, "overlaps")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    """Past every rule a machine without a GPU answers SV_ERR_DEVICE, like every other compute entry
    point: out of place, in place, no accumulator, the plain domain, the limits themselves."""
    for form in (0, 1):
        assert _perm(form=form) == _lib.SV_ERR_DEVICE
        assert _perm(out=_col(1), form=form) == _lib.SV_ERR_DEVICE                           # in place
        assert _perm(acc=None, m=3, chunk=2, shift=_fe(7, form), form=form) == _lib.SV_ERR_DEVICE
        assert _perm(log_n=2, log_ext=0, last_rotation=-3, out=_col(19), form=form) == _lib.SV_ERR_DEVICE
        assert _perm(m=64, chunk=64, form=form) == _lib.SV_ERR_DEVICE
        assert _perm(m=64, chunk=1, form=form) == _lib.SV_ERR_DEVICE
        assert _look(form=form) == _lib.SV_ERR_DEVICE
        assert _look(n=2, out=_col(1), form=form) == _lib.SV_ERR_DEVICE
        assert _look(acc=None, log_n=0, log_ext=0, form=form) == _lib.SV_ERR_DEVICE
        assert _look(n=16, form=form) == _lib.SV_ERR_DEVICE


def test_python_wrappers_are_exported():
    import svgpu
    for name in ("permutation_terms_device", "lookup_terms_device", "permutation_terms",
                 "lagrange_selectors_device"):
        assert callable(getattr(svgpu, name)), name
