"""Batched KZG opening (sv_bn254_fr_poly_combine_eval_device, sv_bn254_kzg_open_batch_device;
include/svgpu.h): every argument rule returns its code and message before anything touches a device,
in the documented order -- form / null / alignment, empty, length, z, v, then the overlap
(combine_eval) or the handle and the range (opening) -- so all of it is checked here without a GPU.
No call below is valid through its last rule, so none reaches a device where there is one: the
"device pointers" are addresses inside a host buffer that nothing dereferences."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

_BUF = np.zeros(4096, np.uint64)
_P = _BUF.ctypes.data          # numpy's buffers are 16-byte aligned (checked below)
_EVALS = (_lib.sv_fe * 8)()
_PART = _lib.sv_g1_jacobian()
_Z = enc.fe_struct(5)
_V = enc.fe_struct(7)
_BAD = [enc.fe_struct(x) for x in (b.R, b.R + 5, (1 << 256) - 1)]
_UNKNOWN = 424242
_TOO_LONG = (1 << 26) + 1
_MAX = 4096


def _arrays(ptrs, lens):
    m = len(ptrs)
    return (ctypes.c_void_p * max(m, 1))(*ptrs), (ctypes.c_uint64 * max(m, 1))(*lens), m


def _combine(ptrs, lens, z=_Z, v=_V, form=0, m=None, ev=_EVALS, combined=None, null=()):
    P, L, mm = _arrays(ptrs, lens)
    return _lib.lib.sv_bn254_fr_poly_combine_eval_device(
        None if "polys" in null else P, None if "lens" in null else L, mm if m is None else m,
        None if "z" in null else ctypes.byref(z), None if "v" in null else ctypes.byref(v), form, 0, None, combined,
        None if "evals" in null else ev)


def _open(ptrs, lens, z=_Z, v=_V, form=0, m=None, ev=_EVALS, handle=_UNKNOWN, offset=0, out=_PART, null=()):
    P, L, mm = _arrays(ptrs, lens)
    return _lib.lib.sv_bn254_kzg_open_batch_device(
        handle, offset, None if "polys" in null else P, None if "lens" in null else L, mm if m is None else m,
        None if "z" in null else ctypes.byref(z), None if "v" in null else ctypes.byref(v), form, None,
        None if "evals" in null else ev, None if "out" in null else ctypes.byref(out))


CALLS = [_combine, _open]


def test_header_constant_matches_the_binding():
    import os
    import re
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    assert int(re.search(r"#define SV_OPEN_BATCH_MAX (\d+)", h).group(1)) == _lib.SV_OPEN_BATCH_MAX == _MAX
    assert _P % 16 == 0


@pytest.mark.parametrize("call", CALLS)
def test_form_null_and_alignment_come_first(call):
    assert call([_P], [1], form=7) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    for which in ("polys", "lens", "z", "v", "evals"):
        assert call([_P], [1], null=(which,)) == _lib.SV_ERR_ARG, which
        assert "null" in _lib.last_error(), which
    # a null d_polys[j], first, middle or last -- before emptiness, the length, z and v
    for ptrs in ([None, _P, _P], [_P, None, _P], [_P, _P, None]):
        assert call(ptrs, [1, 1, 1]) == _lib.SV_ERR_ARG
        assert "null" in _lib.last_error()
        assert call(ptrs, [0, 1, 1]) == _lib.SV_ERR_ARG
        assert call(ptrs, [1, _TOO_LONG, 1], z=_BAD[0], v=_BAD[0]) == _lib.SV_ERR_ARG
        assert "null" in _lib.last_error()
    # a misaligned d_polys[j]
    for ptrs in ([_P + 8, _P], [_P, _P + 24]):
        assert call(ptrs, [1, 1]) == _lib.SV_ERR_ARG
        assert "aligned" in _lib.last_error()
        assert call(ptrs, [0, 0]) == _lib.SV_ERR_ARG
    assert call([_P, _P + 16, _P + 32], [1, 1, 1], v=_BAD[0]) == _lib.SV_ERR_ARG  # 16-byte steps are fine: on to v
    assert "v not reduced" in _lib.last_error()
    # the form before everything else
    assert call([None], [0], form=9, z=_BAD[0]) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()
    assert call([], [], form=-1) == _lib.SV_ERR_ARG
    assert "bad form" in _lib.last_error()


def test_null_witness_pointer():
    assert _open([_P], [1], null=("out",)) == _lib.SV_ERR_ARG
    assert "null" in _lib.last_error()


@pytest.mark.parametrize("call", CALLS)
def test_empty_then_length_then_z_then_v(call):
    for form in (0, 1):
        assert call([], [], form=form) == _lib.SV_ERR_EMPTY                      # m == 0
        assert "empty" in _lib.last_error()
        for lens in ([0, 1, 1], [1, 0, 1], [1, 1, 0]):
            assert call([_P] * 3, lens, form=form) == _lib.SV_ERR_EMPTY
            assert "empty" in _lib.last_error()
        # emptiness before the length, z and v
        assert call([_P] * 2, [_TOO_LONG, 0], form=form) == _lib.SV_ERR_EMPTY
        assert call([], [], z=_BAD[0], v=_BAD[0], form=form) == _lib.SV_ERR_EMPTY
        assert call([_P] * 2, [1, 0], z=_BAD[0], form=form) == _lib.SV_ERR_EMPTY
        # the length: of the batch, of a polynomial
        assert call([_P] * (_MAX + 1), [1] * (_MAX + 1), form=form) == _lib.SV_ERR_LEN
        assert str(_MAX) in _lib.last_error()
        for lens in ([_TOO_LONG, 1], [1, _TOO_LONG]):
            assert call([_P] * 2, lens, form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()
            assert call([_P] * 2, lens, z=_BAD[0], form=form) == _lib.SV_ERR_LEN  # the length before z
            assert call([_P] * 2, lens, v=_BAD[0], form=form) == _lib.SV_ERR_LEN  # ... and before v
        assert call([_P] * (_MAX + 1), [1] * (_MAX + 1), z=_BAD[1], form=form) == _lib.SV_ERR_LEN
        for bad in _BAD:
            assert call([_P], [1], z=bad, form=form) == _lib.SV_ERR_ARG
            assert "z not reduced" in _lib.last_error()
            assert call([_P], [1], z=bad, v=bad, form=form) == _lib.SV_ERR_ARG    # z before v
            assert "z not reduced" in _lib.last_error()
            assert call([_P] * 2, [1 << 26, 1], v=bad, form=form) == _lib.SV_ERR_ARG
            assert "v not reduced" in _lib.last_error()


def test_v_comes_before_the_overlap():
    comb = ctypes.c_void_p(_P)
    assert _combine([_P], [4], v=_BAD[0], combined=comb) == _lib.SV_ERR_ARG
    assert "v not reduced" in _lib.last_error()


def test_combined_over_an_input_is_rejected():
    """Inputs of 4, 2 and 3 rows at rows 8, 20 and 30 of the buffer; N = 4, so d_combined covers four
    rows from its start."""
    row = 32
    ptrs, lens = [_P + 8 * row, _P + 20 * row, _P + 30 * row], [4, 2, 3]
    for start in (5, 8, 11, 17, 21, 27, 32):
        assert _combine(ptrs, lens, combined=ctypes.c_void_p(_P + start * row)) == _lib.SV_ERR_ARG, start
        assert "overlaps" in _lib.last_error()
    assert _combine(ptrs, lens, combined=ctypes.c_void_p(_P + 8)) == _lib.SV_ERR_ARG
    assert "aligned" in _lib.last_error()


def test_v_then_handle_then_range():
    assert _open([_P], [1], v=_BAD[0]) == _lib.SV_ERR_ARG                         # v before the handle
    assert "v not reduced" in _lib.last_error()
    assert _open([_P], [1]) == _lib.SV_ERR_ARG
    assert "unknown base set handle 424242" in _lib.last_error()                  # sv_bn254_g1_msm_bases' message
    assert _open([_P] * 2, [1, 1 << 26], form=1, handle=987654321) == _lib.SV_ERR_ARG
    assert "unknown base set handle 987654321" in _lib.last_error()
    # offsets near 2^64: the range check must not wrap into the handle's range
    assert _open([_P] * 2, [2, 1], offset=(1 << 64) - 1) == _lib.SV_ERR_ARG
    assert _open([_P], [1], offset=(1 << 64) - 1) == _lib.SV_ERR_ARG


def test_python_wrappers_map_the_errors():
    import svgpu
    from svgpu import device as dv
    assert svgpu.poly_combine_eval_device is not None and svgpu.gwc19_open is not None
    s = svgpu.ResidentBases.__new__(svgpu.ResidentBases)  # no device here: a number no set carries
    s.handle = _UNKNOWN
    try:
        one = _arrays([_P], [1])
        with pytest.raises(svgpu.EmptyError, match="empty"):
            s.open_batch_device([], 5, 7)
        with pytest.raises(svgpu.EmptyError, match="empty"):
            s.open_batch_arrays([], 5, 7)
        with pytest.raises(svgpu.EmptyError, match="empty"):
            s.open_batch_pointers(*_arrays([_P, _P], [1, 0]), 5, 7, 0, svgpu.SV_CANONICAL, None)
        with pytest.raises(svgpu.LengthError, match="2\\^26"):
            s.open_batch_pointers(*_arrays([_P], [_TOO_LONG]), 5, 7, 0, svgpu.SV_CANONICAL, None)
        with pytest.raises(svgpu.LengthError, match=str(_MAX)):
            s.open_batch_pointers(*_arrays([_P] * (_MAX + 1), [1] * (_MAX + 1)), 5, 7, 0, svgpu.SV_CANONICAL, None)
        with pytest.raises(svgpu.ArgumentError, match="bad form"):
            s.open_batch_pointers(*one, 5, 7, 0, 5, None)
        for form in (svgpu.SV_CANONICAL, svgpu.SV_MONTGOMERY):
            with pytest.raises(svgpu.ArgumentError, match="z not reduced"):
                s.open_batch_pointers(*one, b.R, 7, 0, form, None)
            with pytest.raises(svgpu.ArgumentError, match="v not reduced"):
                s.open_batch_pointers(*one, 5, b.R, 0, form, None)
            with pytest.raises(svgpu.ArgumentError, match="unknown base set handle 424242"):
                s.open_batch_pointers(*one, b.R - 1, b.R - 1, 0, form, None)
        with pytest.raises(svgpu.ArgumentError, match="unknown base set handle"):
            s.open_batch_pointers(*one, 5, 7, (1 << 64) - 1, svgpu.SV_CANONICAL, None)
        with pytest.raises(svgpu.ArgumentError):
            s.open_batch_pointers(*one, 1 << 256, 7, 0, svgpu.SV_CANONICAL, None)
        with pytest.raises(svgpu.ArgumentError):
            s.open_batch_pointers(*one, 5, -1, 0, svgpu.SV_CANONICAL, None)
        # the division-free entry point through its pointer-level wrapper
        with pytest.raises(svgpu.EmptyError, match="empty"):
            dv.poly_combine_eval_device([], 5, 7)
        with pytest.raises(svgpu.LengthError, match="2\\^26"):
            dv.combine_eval_pointers(*_arrays([_P], [_TOO_LONG]), 5, 7, svgpu.SV_CANONICAL, 0, None, None)
        with pytest.raises(svgpu.ArgumentError, match="v not reduced"):
            dv.combine_eval_pointers(*one, 5, b.R, svgpu.SV_CANONICAL, 0, None, None)
        with pytest.raises(svgpu.ArgumentError, match="overlaps"):
            dv.combine_eval_pointers(*one, 5, 7, svgpu.SV_CANONICAL, 0, None, ctypes.c_void_p(_P))
    finally:
        s.handle = None
    for call in (lambda: s.open_batch_device([], 5, 7), lambda: s.open_batch_arrays([], 5, 7),
                 lambda: s.open_batch_pointers(*_arrays([_P], [1]), 5, 7, 0, svgpu.SV_CANONICAL, None),
                 lambda: svgpu.gwc19_open(s, [None], [(0, 1)], 5, 7)):
        with pytest.raises(svgpu.ArgumentError, match="closed"):
            call()


def test_gwc19_query_sets_group_like_the_reference():
    """gwc19.rs:140-158: sets in order of the first appearance of a shift, polynomials in query order."""
    import svgpu
    w = 0xABCDEF
    queries = [(0, 1), (1, 1), (2, w), (0, w), (3, 1), (4, 5), (2, 1)]
    assert svgpu.gwc19_query_sets(queries) == [(1, [0, 1, 3, 2], [0, 1, 4, 6]), (w, [2, 0], [2, 3]), (5, [4], [5])]
    assert svgpu.gwc19_query_sets([]) == []
