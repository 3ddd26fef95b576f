"""Several points (sv_bn254_fr_poly_eval_points_device, sv_bn254_fr_poly_div_roots_device) and the
SHPLONK opening (sv_bn254_shplonk_work_elems, sv_bn254_shplonk_quotient_device,
sv_bn254_shplonk_witness_device; include/svgpu.h): every argument rule returns its code and message
before anything touches a device, in the documented order -- form / null / alignment, empty, length,
"not reduced", then the call's own rules (n <= K and the overlap; the partition, a repeated point, z'
on a point, the work buffer, the handle and the range) -- so all of it is checked here without a GPU.
No call below is valid through its last rule, so none reaches a device where there is one: the
"device pointers" are addresses inside a host buffer that nothing dereferences.

The grouping of svgpu.bdfg21_query_sets is compared with sets written out by hand from
bdfg21.rs:117-167, on lists that GWC19's grouping (by single shift) would split differently."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

_BUF = np.zeros(4096, np.uint64)
_P = _BUF.ctypes.data
_ROW = 32
_EVALS = (_lib.sv_fe * 64)()
_PART = _lib.sv_g1_jacobian()
_BAD = enc.fe_struct(b.R)
_UNKNOWN = 424242
_TOO_LONG = (1 << 26) + 1
_MAX = 4096
_KMAX = 16


def _fes(values):
    arr = (_lib.sv_fe * max(len(values), 1))()
    for k, x in enumerate(values):
        arr[k] = enc.fe_struct(x)
    return arr


def _arrays(ptrs, lens):
    m = len(ptrs)
    return (ctypes.c_void_p * max(m, 1))(*ptrs), (ctypes.c_uint64 * max(m, 1))(*lens), m


def _sets(descr):
    return (_lib.sv_shplonk_set * max(len(descr), 1))(*[_lib.sv_shplonk_set(*d) for d in descr])


def _eval(ptrs, lens, points=(5,), form=0, null=()):
    P, L, m = _arrays(ptrs, lens)
    return _lib.lib.sv_bn254_fr_poly_eval_points_device(
        None if "polys" in null else P, None if "lens" in null else L, m,
        None if "points" in null else _fes(points), len(points), form, 0, None, None if "evals" in null else _EVALS)


def _div(n, roots=(5,), form=0, coeffs=_P, quot=_P + 2048 * 8, null=()):
    return _lib.lib.sv_bn254_fr_poly_div_roots_device(
        None if "coeffs" in null else coeffs, n, None if "roots" in null else _fes(roots), len(roots), form, 0, None,
        None if "quot" in null else quot)


# one valid shape: three polynomials in two sets, (p0, p1) at two points and p2 at one
_S2 = [(0, 2, 0, 2), (2, 1, 2, 1)]
_WORK = _P + 1024 * 8


def _quot(ptrs=(_P, _P, _P), lens=(8, 5, 3), sets=_S2, points=(5, 6, 7), mu=7, gamma=9, form=0, handle=_UNKNOWN,
          offset=0, work=_WORK, work_elems=24, n_sets=None, null=()):
    P, L, m = _arrays(list(ptrs), list(lens))
    return _lib.lib.sv_bn254_shplonk_quotient_device(
        handle, offset, None if "polys" in null else P, None if "lens" in null else L, m,
        None if "sets" in null else _sets(sets), len(sets) if n_sets is None else n_sets,
        None if "points" in null else _fes(points), len(points),
        None if "mu" in null else ctypes.byref(enc.fe_struct(mu)),
        None if "gamma" in null else ctypes.byref(enc.fe_struct(gamma)), form, None,
        None if "work" in null else work, work_elems, None if "out" in null else ctypes.byref(_PART))


def _wit(set_lens=(8, 3), sets=_S2, points=(5, 6, 7), gamma=9, z_prime=11, form=0, handle=_UNKNOWN, offset=0,
         work=_WORK, work_elems=24, null=()):
    return _lib.lib.sv_bn254_shplonk_witness_device(
        handle, offset, None if "sets" in null else _sets(sets), len(sets),
        None if "points" in null else _fes(points), len(points),
        None if "set_lens" in null else (ctypes.c_uint64 * max(len(set_lens), 1))(*set_lens),
        None if "gamma" in null else ctypes.byref(enc.fe_struct(gamma)),
        None if "z_prime" in null else ctypes.byref(enc.fe_struct(z_prime)), form, None,
        None if "work" in null else work, work_elems, None if "out" in null else ctypes.byref(_PART))


def test_header_constants_match_the_binding():
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    assert int(re.search(r"#define SV_EVAL_POINTS_MAX (\d+)", h).group(1)) == _lib.SV_EVAL_POINTS_MAX == _KMAX
    assert ctypes.sizeof(_lib.sv_shplonk_set) == 16
    assert "typedef struct { uint32_t first_poly, num_polys, first_point, num_points; } sv_shplonk_set;" in h
    assert _P % 16 == 0


def test_eval_points_rules_in_order():
    assert _eval([_P], [1], form=7) == _lib.SV_ERR_ARG and "bad form" in _lib.last_error()
    assert _eval([None], [0], points=(), form=9) == _lib.SV_ERR_ARG and "bad form" in _lib.last_error()
    for which in ("polys", "lens", "points", "evals"):
        assert _eval([_P], [1], null=(which,)) == _lib.SV_ERR_ARG and "null" in _lib.last_error(), which
    assert _eval([_P, None], [0, 1]) == _lib.SV_ERR_ARG and "null" in _lib.last_error()       # before emptiness
    assert _eval([_P, _P + 8], [0, 1]) == _lib.SV_ERR_ARG and "aligned" in _lib.last_error()
    assert _eval([], [], points=(b.R,) * 17) == _lib.SV_ERR_EMPTY                               # m == 0 first
    assert _eval([_P, _P], [1, 0], points=(b.R,) * 17) == _lib.SV_ERR_EMPTY
    assert _eval([_P], [_TOO_LONG], points=()) == _lib.SV_ERR_EMPTY and "points" in _lib.last_error()   # K == 0
    assert _eval([_P], [1], points=(b.R,) * (_KMAX + 1)) == _lib.SV_ERR_LEN and str(_KMAX) in _lib.last_error()
    assert _eval([_P] * (_MAX + 1), [1] * (_MAX + 1), points=(b.R,)) == _lib.SV_ERR_LEN
    assert _eval([_P, _P], [1, _TOO_LONG], points=(b.R,)) == _lib.SV_ERR_LEN and "2^26" in _lib.last_error()
    for form in (0, 1):
        assert _eval([_P], [1 << 26], points=(5, b.R), form=form) == _lib.SV_ERR_ARG
        assert "point 1 not reduced" in _lib.last_error()
        assert _eval([_P], [1], points=((1 << 256) - 1,) * _KMAX, form=form) == _lib.SV_ERR_ARG
        assert "point 0 not reduced" in _lib.last_error()


def test_div_roots_rules_in_order():
    assert _div(8, form=5) == _lib.SV_ERR_ARG and "bad form" in _lib.last_error()
    for which in ("coeffs", "roots", "quot"):
        assert _div(8, null=(which,)) == _lib.SV_ERR_ARG and "null" in _lib.last_error(), which
    assert _div(0, coeffs=_P + 8) == _lib.SV_ERR_ARG and "aligned" in _lib.last_error()
    assert _div(0, roots=(b.R,)) == _lib.SV_ERR_EMPTY
    assert _div(8, roots=()) == _lib.SV_ERR_EMPTY and "roots" in _lib.last_error()
    assert _div(8, roots=(b.R,) * (_KMAX + 1)) == _lib.SV_ERR_LEN and str(_KMAX) in _lib.last_error()
    assert _div(_TOO_LONG, roots=(b.R,)) == _lib.SV_ERR_LEN and "2^26" in _lib.last_error()
    assert _div(1, roots=(5, b.R)) == _lib.SV_ERR_ARG and "root 1 not reduced" in _lib.last_error()
    for n, roots in ((1, (5,)), (3, (5, 6, 7)), (2, (5, 5, 5))):                 # n <= K, before the overlap
        assert _div(n, roots=roots, quot=_P) == _lib.SV_ERR_ARG and "no quotient" in _lib.last_error()
    # coefficients in rows [8, 16): the n - K = 6 quotient rows from row s overlap them for 3 <= s <= 15
    for s in (3, 8, 15):
        assert _div(8, roots=(5, 6), coeffs=_P + 8 * _ROW, quot=_P + s * _ROW) == _lib.SV_ERR_ARG
        assert "overlaps" in _lib.last_error()


def test_work_elems():
    e = ctypes.c_uint64(0)
    assert _lib.lib.sv_bn254_shplonk_work_elems(3, 100, None) == _lib.SV_ERR_ARG
    assert _lib.lib.sv_bn254_shplonk_work_elems(0, 100, ctypes.byref(e)) == _lib.SV_ERR_EMPTY
    assert _lib.lib.sv_bn254_shplonk_work_elems(3, 0, ctypes.byref(e)) == _lib.SV_ERR_EMPTY
    assert _lib.lib.sv_bn254_shplonk_work_elems(_MAX + 1, 1, ctypes.byref(e)) == _lib.SV_ERR_LEN
    assert _lib.lib.sv_bn254_shplonk_work_elems(1, _TOO_LONG, ctypes.byref(e)) == _lib.SV_ERR_LEN
    assert _lib.lib.sv_bn254_shplonk_work_elems(3, 100, ctypes.byref(e)) == _lib.SV_OK and e.value == 400
    assert _lib.lib.sv_bn254_shplonk_work_elems(_MAX, 1 << 26, ctypes.byref(e)) == _lib.SV_OK
    assert e.value == (_MAX + 1) << 26


def test_shplonk_form_null_alignment_come_first():
    for call in (_quot, _wit):
        assert call(form=3, points=(b.R, b.R, b.R)) == _lib.SV_ERR_ARG and "bad form" in _lib.last_error()
        assert call(work=_WORK + 8, sets=[]) == _lib.SV_ERR_ARG and "aligned" in _lib.last_error()
    for which in ("polys", "lens", "sets", "points", "mu", "gamma", "work", "out"):
        assert _quot(null=(which,), sets=[]) == _lib.SV_ERR_ARG and "null" in _lib.last_error(), which
    for which in ("sets", "points", "set_lens", "gamma", "z_prime", "work", "out"):
        assert _wit(null=(which,), sets=[]) == _lib.SV_ERR_ARG and "null" in _lib.last_error(), which
    assert _quot(ptrs=(_P, None, _P), lens=(0, 0, 0)) == _lib.SV_ERR_ARG and "null" in _lib.last_error()
    assert _quot(ptrs=(_P, _P, _P + 8), lens=(0, 0, 0)) == _lib.SV_ERR_ARG and "aligned" in _lib.last_error()


def test_shplonk_empty_then_length_then_reduced():
    big = [(0, 2, 0, _KMAX + 1), (2, 1, _KMAX + 1, 1)]
    assert _quot(ptrs=(), lens=(), sets=[], points=()) == _lib.SV_ERR_EMPTY
    assert _quot(lens=(8, 0, 3), sets=big, mu=b.R) == _lib.SV_ERR_EMPTY                  # a length of 0
    assert _quot(sets=[], mu=b.R) == _lib.SV_ERR_EMPTY and "sets" in _lib.last_error()  # n_sets == 0
    assert _quot(points=(), mu=b.R) == _lib.SV_ERR_EMPTY and "points" in _lib.last_error()
    assert _quot(sets=[(0, 3, 0, 3), (3, 0, 3, 0)], lens=(8, _TOO_LONG, 3)) == _lib.SV_ERR_EMPTY
    assert "set 1" in _lib.last_error()
    assert _wit(set_lens=(8, 0), sets=big, gamma=b.R) == _lib.SV_ERR_EMPTY
    assert _wit(sets=[], gamma=b.R) == _lib.SV_ERR_EMPTY
    # the lengths: a polynomial, the points of a set, the number of sets -- before any "not reduced"
    assert _quot(lens=(8, _TOO_LONG, 3), mu=b.R) == _lib.SV_ERR_LEN and "2^26" in _lib.last_error()
    assert _quot(sets=big, points=(b.R,) * (_KMAX + 2)) == _lib.SV_ERR_LEN and str(_KMAX) in _lib.last_error()
    assert _wit(set_lens=(_TOO_LONG, 3), gamma=b.R) == _lib.SV_ERR_LEN and "2^26" in _lib.last_error()
    assert _wit(sets=big, points=(b.R,) * (_KMAX + 2)) == _lib.SV_ERR_LEN and str(_KMAX) in _lib.last_error()
    # not reduced: a point, then mu, then gamma (z' in the second call) -- before the partition
    wrong = [(0, 2, 0, 2), (1, 1, 2, 1)]
    for form in (0, 1):
        assert _quot(points=(5, b.R, 7), mu=b.R, sets=wrong, form=form) == _lib.SV_ERR_ARG
        assert "point 1 not reduced" in _lib.last_error()
        assert _quot(mu=b.R, gamma=b.R, sets=wrong, form=form) == _lib.SV_ERR_ARG and "mu" in _lib.last_error()
        assert _quot(gamma=b.R + 5, sets=wrong, form=form) == _lib.SV_ERR_ARG and "gamma" in _lib.last_error()
        assert _wit(points=(b.R, 6, 7), gamma=b.R, sets=wrong, form=form) == _lib.SV_ERR_ARG
        assert "point 0 not reduced" in _lib.last_error()
        assert _wit(gamma=b.R, z_prime=b.R, sets=wrong, form=form) == _lib.SV_ERR_ARG and "gamma" in _lib.last_error()
        assert _wit(z_prime=b.R, sets=wrong, form=form) == _lib.SV_ERR_ARG and "z_prime" in _lib.last_error()


def test_shplonk_partition_repeat_zprime_work_handle_range():
    for wrong in ([(0, 2, 0, 2), (1, 1, 2, 1)],      # polynomial 1 twice
                  [(0, 2, 0, 2), (2, 1, 1, 1)],      # point 1 twice
                  [(0, 2, 0, 2)],                    # polynomial 2 and point 2 in no set
                  [(0, 1, 0, 2), (2, 1, 2, 1)],      # polynomial 1 in no set
                  [(2, 1, 2, 1), (0, 2, 0, 2)]):     # out of order
        assert _quot(sets=wrong, points=(5, 5, 7), work_elems=0) == _lib.SV_ERR_ARG, wrong
        assert "partition" in _lib.last_error(), wrong
    assert _wit(sets=[(0, 2, 0, 2), (2, 1, 1, 1)], points=(5, 5, 7), z_prime=5, work_elems=0) == _lib.SV_ERR_ARG
    assert "partition" in _lib.last_error()
    # two equal points inside one set; the same value in two sets is fine (on to the work buffer)
    for call in (_quot, _wit):
        assert call(points=(5, 5, 7), work_elems=0) == _lib.SV_ERR_ARG and "repeated point" in _lib.last_error()
        assert call(points=(5, 6, 5), work_elems=0) == _lib.SV_ERR_ARG and "work_elems" in _lib.last_error()
    # z' on a point, before the work buffer
    for zp in (5, 6, 7):
        assert _wit(z_prime=zp, work_elems=0) == _lib.SV_ERR_ARG and "z_prime equals" in _lib.last_error()
    # the work buffer: (n_sets + 1) N = 24 elements, before the handle
    for call in (_quot, _wit):
        assert call(work_elems=23) == _lib.SV_ERR_ARG and "work_elems" in _lib.last_error()
        assert call(work_elems=24) == _lib.SV_ERR_ARG and "unknown base set handle 424242" in _lib.last_error()
        assert call(work_elems=24, offset=(1 << 64) - 1) == _lib.SV_ERR_ARG
    # d_work over a polynomial (the first call writes it while blocks still read the polynomials)
    assert _quot(ptrs=(_P, _WORK + 23 * _ROW, _P), work_elems=24) == _lib.SV_ERR_ARG and "overlaps" in _lib.last_error()


def test_python_wrappers_map_the_errors():
    import svgpu
    from svgpu import device as dv
    one = _arrays([_P], [1])
    with pytest.raises(svgpu.EmptyError, match="empty"):
        dv.eval_points_pointers(*_arrays([], []), [5], svgpu.SV_CANONICAL, 0, None)
    with pytest.raises(svgpu.EmptyError, match="points"):
        dv.eval_points_pointers(*one, [], svgpu.SV_CANONICAL, 0, None)
    with pytest.raises(svgpu.LengthError, match=str(_KMAX)):
        dv.eval_points_pointers(*one, [5] * (_KMAX + 1), svgpu.SV_CANONICAL, 0, None)
    for form in (svgpu.SV_CANONICAL, svgpu.SV_MONTGOMERY):
        with pytest.raises(svgpu.ArgumentError, match="point 2 not reduced"):
            dv.eval_points_pointers(*one, [5, 6, b.R], form, 0, None)
    with pytest.raises(svgpu.ArgumentError):
        dv.eval_points_pointers(*one, [-1], svgpu.SV_CANONICAL, 0, None)
    assert svgpu.poly_eval_points_device is not None and svgpu.poly_div_roots_device is not None
    assert svgpu.bdfg21_open is not None and svgpu.Bdfg21Opening is not None
    s = svgpu.ResidentBases.__new__(svgpu.ResidentBases)
    s.handle = None
    with pytest.raises(svgpu.ArgumentError, match="closed"):
        svgpu.bdfg21_open(s, [None], [(0, 1)], 5, (1, 2, 3))


def test_bdfg21_query_sets_group_like_the_reference():
    """bdfg21.rs:117-167.  Every polynomial first collects its distinct shifts in query order; then
    polynomials group by the SET of their shifts in order of first appearance, and a set keeps the
    shift order of its first polynomial.  The expected sets are written out by hand."""
    import svgpu
    w, u = 0xABCDEF, 0x1234567
    # the same two shifts in different order per polynomial: ONE set (GWC19 makes two, one per shift),
    # in polynomial 0's order; polynomial 1's query indices follow the set's order, not its own
    queries = [(0, 1), (0, w), (1, w), (1, 1)]
    assert svgpu.bdfg21_query_sets(queries) == [([1, w], [0, 1], [[0, 1], [3, 2]])]
    assert [s[0] for s in svgpu.gwc19_query_sets(queries)] == [1, w]
    # a repeated query is dropped (its first occurrence stands); interleaved polynomials
    queries = [(0, 1), (1, 1), (0, 1), (0, w), (1, w), (1, 1)]
    assert svgpu.bdfg21_query_sets(queries) == [([1, w], [0, 1], [[0, 3], [1, 4]])]
    # a polynomial queried at a superset of another's shifts is a set of its own, and a polynomial
    # with the first one's shifts met later still joins the first set
    queries = [(0, 1), (1, 1), (1, w), (2, w), (2, 1), (2, u), (3, 1), (4, w), (4, 1)]
    assert svgpu.bdfg21_query_sets(queries) == [
        ([1], [0, 3], [[0], [6]]),
        ([1, w], [1, 4], [[1, 2], [8, 7]]),
        ([w, 1, u], [2], [[3, 4, 5]]),
    ]
    # a single query; none
    assert svgpu.bdfg21_query_sets([(7, w)]) == [([w], [7], [[0]])]
    assert svgpu.bdfg21_query_sets([]) == []
