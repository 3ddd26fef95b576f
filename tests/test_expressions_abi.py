"""sv_bn254_fr_expressions_device (include/svgpu.h) without a GPU: every argument rule in the
documented order, each with its code and message before anything touches a device.
  1 bad form; 2 a null program, pointer array, consts or entry; 3 alignment; 4 empty; 5 log_ext, K,
  then a count above its cap; 6 the program walk, op by op, then its end; 7 a FOLD with y or d_out
  NULL; 8 y or a constant that is read not reduced; 9 the overlaps.
No call below except the last tests' is valid through its last rule, so none reaches a device where
there is one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

R = b.R
E = 32                                       # bytes per element
N = 4                                        # log_n = 1, log_ext = 1: four rows per column
_BUF = np.zeros(4 * (N * 300 + 1), np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15           # 16-byte aligned, room for 300 columns behind it
_BAD = [enc.fe_struct(v) for v in (R, R + 5, (1 << 256) - 1)]
_UNSET = object()
COLUMN, CONST, NEG, ADD, SUB, RSUB, MUL, FOLD, STORE = range(9)
# columns of the default call: 0 out, 1 acc, 2 .. 17 the stores, 20 .. 275 the columns
OUT, ACC, STORE0, COL0 = 0, 1, 2, 20
DEFAULT = [(COLUMN, 0, 0), (COLUMN, 1, 1), (MUL, 0, 0), (CONST, 0, 0), (ADD, 0, 0), (FOLD, 0, 0), (COLUMN, 2, -1),
           (STORE, 0, 0)]


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


def _ops(triples):
    arr = (_lib.sv_fr_expr_op * max(len(triples), 1))()
    for i, t in enumerate(triples):
        arr[i].op, arr[i].index, arr[i].rotation = t[:3]
        arr[i].zero = t[3] if len(t) > 3 else 0
    return arr


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _call(ops=DEFAULT, n_ops=None, cols=_UNSET, n_cols=3, consts=_UNSET, n_consts=1, stores=_UNSET, n_stores=1, y=_UNSET,
          acc=_col(ACC), out=_col(OUT), log_n=1, log_ext=1, form=0):
    program = _ops(ops) if isinstance(ops, list) else ops
    n_ops = len(ops) if n_ops is None else n_ops
    cols = _ptrs([_col(COL0 + j) for j in range(min(n_cols, 256))]) if cols is _UNSET else cols
    stores = _ptrs([_col(STORE0 + j) for j in range(min(n_stores, 16))]) if stores is _UNSET else stores
    consts = (_lib.sv_fe * max(n_consts, 1))(*[_fe(3 + j, form) for j in range(min(n_consts, 256))]) \
        if consts is _UNSET else consts
    y = _fe(7, form) if y is _UNSET else y
    return _lib.lib.sv_bn254_fr_expressions_device(program, n_ops, cols, n_cols, consts, n_consts, stores, n_stores,
                                                   _ref(y), acc, out, log_n, log_ext, form, 0, None)


def _is(rc, code, word):
    assert rc == code, (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def test_struct_and_caps_are_pinned():
    assert ctypes.sizeof(_lib.sv_fr_expr_op) == 8
    caps = dict(OPS=4096, COLUMNS=256, CONSTS=256, STORES=16, STACK=8)
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    rs = open(os.path.join(ROOT, "snark-verifier-gpu", "src", "lib.rs")).read()
    plan = open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "expr_plan.hpp")).read()
    for name, v in caps.items():
        assert getattr(_lib, f"SV_EXPR_{name}_MAX") == v
        assert int(re.search(rf"#define SV_EXPR_{name}_MAX\s+(\d+)", h).group(1)) == v
        assert int(re.search(rf"pub const SV_EXPR_{name}_MAX: usize = (\d+);", rs).group(1)) == v
        assert int(re.search(rf"kExpr{name.capitalize()}Max = (\d+);", plan).group(1)) == v
    for i, name in enumerate(("COLUMN", "CONST", "NEG", "ADD", "SUB", "RSUB", "MUL", "FOLD", "STORE")):
        assert getattr(_lib, f"SV_EXPR_{name}") == i
        assert re.search(rf"SV_EXPR_{name}\s*= {i}\b", h) and re.search(rf"pub const SV_EXPR_{name}: u8 = {i};", rs)
    assert re.search(r"pub struct SvFrExprOp \{\s*pub op: u8,\s*pub zero: u8,\s*pub index: u16,\s*pub rotation: i32,", rs)
    assert "typedef struct { uint8_t op; uint8_t zero; uint16_t index; int32_t rotation; } sv_fr_expr_op;" in h


def test_rule_1_form_and_rule_2_nulls():
    _is(_call(form=7, ops=None, n_ops=0), _lib.SV_ERR_ARG, "bad form")                 # before every other rule
    for kw in ("ops", "cols", "consts", "stores"):
        extra = dict(n_ops=len(DEFAULT)) if kw == "ops" else {}
        _is(_call(**{kw: None}, **extra), _lib.SV_ERR_ARG, "null")
        _is(_call(**{kw: None}, n_ops=0, log_ext=9, out=_col(OUT) + 8), _lib.SV_ERR_ARG, "null")   # before 3, 4, 5
    for hole in (0, 2):
        arr = _ptrs([None if j == hole else _col(COL0 + j) for j in range(3)])
        _is(_call(cols=arr), _lib.SV_ERR_ARG, "null")
        _is(_call(cols=arr, acc=_col(ACC) + 8, n_ops=0), _lib.SV_ERR_ARG, "null")      # before the alignment
    arr = _ptrs([_col(STORE0), None])
    _is(_call(stores=arr, n_stores=2), _lib.SV_ERR_ARG, "null")
    # a null array with a zero count is legal, and an entry beyond a cap is not looked at: a later rule answers
    _is(_call(ops=[(CONST, 0, 0), (FOLD, 0, 0)], cols=None, n_cols=0, stores=None, n_stores=0, log_ext=9),
        _lib.SV_ERR_LEN, "log_ext")
    arr = _ptrs([_col(COL0 + j % 3) for j in range(256)] + [None])
    _is(_call(cols=arr, n_cols=257), _lib.SV_ERR_LEN, "at most 256")


def test_rule_3_alignment():
    for off in (8, 4, 1):
        for kw in ("out", "acc"):
            _is(_call(**{kw: _col(280) + off}), _lib.SV_ERR_ARG, "aligned")
        _is(_call(cols=_ptrs([_col(COL0), _col(COL0 + 1) + off, _col(COL0 + 2)])), _lib.SV_ERR_ARG, "aligned")
        _is(_call(stores=_ptrs([_col(STORE0) + off])), _lib.SV_ERR_ARG, "aligned")
    _is(_call(out=_col(OUT) + 8, n_ops=0, log_ext=9), _lib.SV_ERR_ARG, "aligned")      # before rules 4, 5
    # a column the program never names is held to the rule all the same
    _is(_call(cols=_ptrs([_col(COL0 + j) for j in range(3)] + [_col(COL0 + 3) + 8]), n_cols=4), _lib.SV_ERR_ARG, "aligned")


def test_rules_4_and_5_empty_then_lengths():
    for form in (0, 1):
        _is(_call(n_ops=0, form=form), _lib.SV_ERR_EMPTY, "empty")
        _is(_call(n_ops=0, log_ext=9, n_cols=300, y=_BAD[0], form=form), _lib.SV_ERR_EMPTY, "empty")   # before 5
        for log_ext in (9, (1 << 32) - 1):
            _is(_call(log_ext=log_ext, form=form), _lib.SV_ERR_LEN, "log_ext")
            _is(_call(log_ext=log_ext, log_n=27, n_consts=257, form=form), _lib.SV_ERR_LEN, "log_ext")  # before K, caps
        for log_n, log_ext in ((26, 1), (19, 8), (27, 0), ((1 << 32) - 1, 0), ((1 << 32) - 1, 1)):
            _is(_call(log_n=log_n, log_ext=log_ext, form=form), _lib.SV_ERR_LEN, "2^26")
            _is(_call(log_n=log_n, log_ext=log_ext, n_stores=17, form=form), _lib.SV_ERR_LEN, "2^26")   # before a cap
        big = _ops([(CONST, 0, 0)] * 4097)
        for kw, count, word in (("n_cols", 257, "at most 256"), ("n_cols", 10**6, "at most 256"),
                                ("n_consts", 257, "at most 256"), ("n_stores", 17, "at most 16")):
            _is(_call(**{kw: count}, form=form), _lib.SV_ERR_LEN, word)
            _is(_call(**{kw: count}, ops=[(99, 0, 0)], y=_BAD[1], form=form), _lib.SV_ERR_LEN, word)   # before 6, 8
        _is(_call(ops=big, n_ops=4097, form=form), _lib.SV_ERR_LEN, "at most 4096")
        _is(_call(ops=big, n_ops=1 << 40, form=form), _lib.SV_ERR_LEN, "at most 4096")   # ops beyond the cap: not read


WALK = [
    # (program, log_n, the offending op, the message)
    ([(9, 0, 0)], 1, 0, "unknown opcode"),
    ([(CONST, 0, 0), (255, 0, 0)], 1, 1, "unknown opcode"),
    ([(CONST, 0, 0, 1), (FOLD, 0, 0)], 1, 0, "zero field"),
    ([(CONST, 0, 0), (FOLD, 0, 0, 255)], 1, 1, "zero field"),
    ([(COLUMN, 3, 0), (FOLD, 0, 0)], 1, 0, "index out of range"),
    ([(COLUMN, 65535, 0), (FOLD, 0, 0)], 1, 0, "index out of range"),
    ([(CONST, 1, 0), (FOLD, 0, 0)], 1, 0, "index out of range"),
    ([(CONST, 0, 0), (STORE, 1, 0)], 1, 1, "index out of range"),
    ([(CONST, 0, 0), (NEG, 1, 0), (FOLD, 0, 0)], 1, 1, "index out of range"),
    ([(CONST, 0, 0), (FOLD, 7, 0)], 1, 1, "index out of range"),
    ([(COLUMN, 0, 2), (FOLD, 0, 0)], 1, 0, "rotation outside"),
    ([(COLUMN, 0, -2), (FOLD, 0, 0)], 1, 0, "rotation outside"),
    ([(COLUMN, 0, 8), (FOLD, 0, 0)], 3, 0, "rotation outside"),
    ([(COLUMN, 0, -(1 << 31)), (FOLD, 0, 0)], 1, 0, "rotation outside"),
    ([(COLUMN, 0, (1 << 31) - 1), (FOLD, 0, 0)], 1, 0, "rotation outside"),
    ([(CONST, 0, 5), (FOLD, 0, 0)], 1, 0, "rotation outside"),                    # the range before the kind
    ([(CONST, 0, 1), (FOLD, 0, 0)], 1, 0, "not COLUMN"),
    ([(CONST, 0, 0), (FOLD, 0, -1)], 1, 1, "not COLUMN"),
    ([(CONST, 0, 0), (CONST, 0, 0), (ADD, 0, 1), (FOLD, 0, 0)], 3, 2, "not COLUMN"),
    ([(NEG, 0, 0)], 1, 0, "underflow"),
    ([(FOLD, 0, 0)], 1, 0, "underflow"),
    ([(STORE, 0, 0)], 1, 0, "underflow"),
    ([(CONST, 0, 0), (MUL, 0, 0)], 1, 1, "underflow"),
    ([(CONST, 0, 0), (FOLD, 0, 0), (CONST, 0, 0), (RSUB, 0, 0)], 1, 3, "underflow"),
    ([(CONST, 0, 0)] * 9, 1, 8, "deeper than"),
    ([(COLUMN, 0, 0)] * 8 + [(ADD, 0, 0), (COLUMN, 1, 1), (COLUMN, 2, 0)], 1, 10, "deeper than"),
    ([(CONST, 0, 0), (STORE, 0, 0), (CONST, 0, 0), (STORE, 0, 0)], 1, 3, "second STORE"),
    ([(CONST, 0, 0), (CONST, 0, 0), (FOLD, 0, 0)], 1, None, "not empty"),
    ([(CONST, 0, 0)], 1, None, "not empty"),
    ([(NEG, 0, 0, 1)], 1, 0, "zero field"),                                         # an op's rules in their order
    ([(9, 0, 0, 1)], 1, 0, "unknown opcode"),
    ([(NEG, 1, 5)], 1, 0, "index out of range"),
    ([(CONST, 0, 0), (STORE, 0, 0), (CONST, 0, 0), (STORE, 0, 1)], 1, 3, "not COLUMN"),
]


def test_rule_6_the_program_walk():
    for form in (0, 1):
        for program, log_n, at, word in WALK:
            for extra in ({}, dict(y=None, out=None), dict(y=_BAD[0]), dict(out=_col(COL0))):   # before 7, 8, 9
                _is(_call(ops=program, log_n=log_n, log_ext=0 if log_n > 1 else 1, form=form, **extra), _lib.SV_ERR_ARG,
                    word)
                where = f"op {at} " if at is not None else f"after op {len(program) - 1},"
                assert where in _lib.last_error(), (_lib.last_error(), where)
    # every op that is not a sink leaves a value on the stack, so through this entry point "not empty"
    # always answers before "neither FOLD nor STORE" can (tests/native/expr_plan_check.cpp reaches the
    # latter in the walk itself, with no ops)
    _is(_call(ops=[(CONST, 0, 0), (NEG, 0, 0)]), _lib.SV_ERR_ARG, "not empty")


def test_rule_7_fold_needs_y_and_out():
    fold_only = [(CONST, 0, 0), (FOLD, 0, 0)]
    for form in (0, 1):
        for kw in ("y", "out"):
            _is(_call(**{kw: None}, form=form), _lib.SV_ERR_ARG, "null")
            _is(_call(ops=fold_only, **{kw: None}, consts=(_lib.sv_fe * 1)(_BAD[0]), form=form), _lib.SV_ERR_ARG, "null")
        # a program without a FOLD reads none of them: null, unreduced, overlapping, a later rule or none answers
        store_only = [(COLUMN, 0, 0), (STORE, 0, 0)]
        _is(_call(ops=store_only, y=None, acc=None, out=None, stores=_ptrs([_col(COL0)]), form=form), _lib.SV_ERR_ARG,
            "overlaps")
        _is(_call(ops=store_only, y=_BAD[0], acc=_col(COL0), out=_col(COL0 + 1), stores=_ptrs([_col(COL0 + 2)]),
                  form=form), _lib.SV_ERR_ARG, "overlaps")


def test_rule_8_scalars_that_are_read():
    for form in (0, 1):
        for bad in _BAD:
            _is(_call(y=bad, form=form), _lib.SV_ERR_ARG, "not reduced")
            _is(_call(y=bad, out=_col(COL0), form=form), _lib.SV_ERR_ARG, "not reduced")          # before the overlap
            _is(_call(consts=(_lib.sv_fe * 1)(bad), form=form), _lib.SV_ERR_ARG, "not reduced")
            two = (_lib.sv_fe * 2)(_fe(3, form), bad)
            _is(_call(ops=[(CONST, 1, 0), (FOLD, 0, 0)], consts=two, n_consts=2, out=_col(COL0), form=form),
                _lib.SV_ERR_ARG, "not reduced")
            # a constant the program never reads is not held to the rule: the overlap answers
            _is(_call(consts=two, n_consts=2, out=_col(COL0), form=form), _lib.SV_ERR_ARG, "overlaps")


def test_rule_9_overlaps():
    for form in (0, 1):
        others = [ACC, STORE0, COL0, COL0 + 1, COL0 + 2]
        for i in others:                                     # d_out against everything else
            for off in (-3, -1, 1, 3):                       # rows: partial overlap on either side
                _is(_call(out=_col(i) + off * E, form=form), _lib.SV_ERR_ARG, "overlaps")
        for i in others[1:]:                                 # equal pointers: in place is d_acc_in only
            _is(_call(out=_col(i), form=form), _lib.SV_ERR_ARG, "overlaps")
        _is(_call(out=_col(COL0), acc=_col(COL0), form=form), _lib.SV_ERR_ARG, "overlaps")   # in place, but onto a column
        for i in (OUT, ACC, COL0, COL0 + 2):                 # the written store against everything else
            for off in (-3, 0, 2):
                _is(_call(stores=_ptrs([_col(i) + off * E]), form=form), _lib.SV_ERR_ARG, "overlaps")
        # a column that is passed but never named still may not be written
        _is(_call(n_cols=4, stores=_ptrs([_col(COL0 + 3)]), form=form), _lib.SV_ERR_ARG, "overlaps")
        # two stores: a written one onto the other, written or not
        both = [(CONST, 0, 0), (STORE, 0, 0), (CONST, 0, 0), (STORE, 1, 0)]
        _is(_call(ops=both, stores=_ptrs([_col(STORE0), _col(STORE0) + E]), n_stores=2, form=form), _lib.SV_ERR_ARG,
            "overlaps")
        _is(_call(stores=_ptrs([_col(STORE0), _col(STORE0)]), n_stores=2, form=form), _lib.SV_ERR_ARG, "overlaps")
        _is(_call(ops=[(CONST, 0, 0), (STORE, 1, 0)], stores=_ptrs([_col(STORE0) + E, _col(STORE0)]), n_stores=2,
                  form=form), _lib.SV_ERR_ARG, "overlaps")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    """Past every rule a machine without a GPU answers SV_ERR_DEVICE, like every other compute entry
    point: out of place, in place, no accumulator, a stores-only program with nothing else, the plain
    domain, the caps themselves."""
    for form in (0, 1):
        assert _call(form=form) == _lib.SV_ERR_DEVICE
        assert _call(out=_col(ACC), form=form) == _lib.SV_ERR_DEVICE                          # in place
        assert _call(acc=None, form=form) == _lib.SV_ERR_DEVICE
        assert _call(ops=[(COLUMN, 0, -3), (STORE, 0, 0)], y=None, acc=None, out=None, log_n=2, log_ext=0,
                     form=form) == _lib.SV_ERR_DEVICE
        # an unwritten store may lie anywhere, and a program without a FOLD may be handed anything as d_out
        assert _call(ops=[(COLUMN, 0, 0), (STORE, 1, 0)], stores=_ptrs([_col(COL0), _col(STORE0)]), n_stores=2,
                     out=_col(COL0), y=_BAD[0], form=form) == _lib.SV_ERR_DEVICE
        deep = [(CONST, 0, 0)] * 8 + [(MUL, 0, 0)] * 7 + [(FOLD, 0, 0)]
        assert _call(ops=deep, form=form) == _lib.SV_ERR_DEVICE
        assert _call(ops=deep * 256, n_cols=256, n_consts=256, n_stores=16, form=form) == _lib.SV_ERR_DEVICE


def test_python_wrappers_are_exported():
    import svgpu
    for name in ("expressions_device", "compile_expressions", "compress_expressions"):
        assert callable(getattr(svgpu, name)), name
