"""Running products and batch inversion (sv_bn254_fr_grand_product_device,
sv_bn254_fr_batch_invert_device; include/svgpu.h) without a GPU: both symbols in the library, the
ctypes table and the Rust crate; every argument rule in the documented order -- 1 form / null / kind
/ alignment, 2 empty, 3 length, 4 not reduced, 5 IDENTITY without omega, 6 overlap -- each with its
code and message; and the two Python builders' factor lists.  Every call below except the last
test's is invalid through the rule under test, so none reaches a device where there is one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import bn254 as b
from svgpu import _lib
from svgpu import encoding as enc

PLAIN, COLUMN, IDENTITY = _lib.SV_FACTOR_PLAIN, _lib.SV_FACTOR_COLUMN, _lib.SV_FACTOR_IDENTITY
MAX = _lib.SV_PRODUCT_FACTORS_MAX
_BUF = np.zeros(256, np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15          # 16-byte aligned; X, Y and Z are three disjoint runs of 8 elements
_X, _Y, _Z = _P, _P + 512, _P + 1024
_ONE, _ZERO = enc.fe_struct(1), enc.fe_struct(0)
_BAD = [enc.fe_struct(v) for v in (b.R, b.R + 5, (1 << 256) - 1)]
_W = enc.fe_struct(b.R - 1)                  # root_of_unity(1)


def _factors(specs):
    """specs: (kind, d_x, d_y, s, c) with s and c sv_fe -> (array, count)."""
    arr = (_lib.sv_fr_factor * max(len(specs), 1))()
    for j, (kind, x, y, s, c) in enumerate(specs):
        arr[j].kind, arr[j].d_x, arr[j].d_y, arr[j].s, arr[j].c = kind, x, y, s, c
    return arr


def plain(x=_X, c=_ZERO, s=_ZERO):
    return (PLAIN, x, None, s, c)


def column(x=_X, y=_Y, s=_ONE, c=_ZERO):
    return (COLUMN, x, y, s, c)


def identity(x=_X, s=_ONE, c=_ZERO):
    return (IDENTITY, x, None, s, c)


_DEFAULT = object()


def _gp(num=(plain(),), den=(), n=2, z0=_ONE, omega=None, form=0, d_z=_Z, total=_DEFAULT, n_num=None, n_den=None,
        num_arr=_DEFAULT, den_arr=_DEFAULT):
    na = _factors(list(num)) if num_arr is _DEFAULT else num_arr
    da = _factors(list(den)) if den_arr is _DEFAULT else den_arr
    out = _lib.sv_fe()
    return _lib.lib.sv_bn254_fr_grand_product_device(
        na, len(num) if n_num is None else n_num, da, len(den) if n_den is None else n_den, n,
        ctypes.byref(z0) if z0 is not None else None, ctypes.byref(omega) if omega is not None else None, form, d_z,
        ctypes.byref(out) if total is _DEFAULT else total, 0, None)


def _inv(d_in=_X, d_out=_X, n=2, form=0):
    return _lib.lib.sv_bn254_fr_batch_invert_device(d_in, d_out, n, form, 0, None)


def _arg(rc, word):
    assert rc == _lib.SV_ERR_ARG, (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def test_symbols_in_library_ctypes_table_and_crate():
    names = {"sv_bn254_fr_grand_product_device": 12, "sv_bn254_fr_batch_invert_device": 6}
    table = {p[0]: p for p in _lib.PROTOTYPES}
    rs = open(os.path.join(ROOT, "snark-verifier-gpu", "src", "lib.rs")).read()
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    for name, params in names.items():
        assert hasattr(_lib.lib, name)
        assert len(table[name][2]) == params
        m = re.search(r"pub fn %s\(([^)]*)\)" % name, rs, flags=re.S)
        assert m and m.group(1).count(",") + 1 == params
    assert (PLAIN, COLUMN, IDENTITY, MAX) == (0, 1, 2, 16)
    assert "#define SV_PRODUCT_FACTORS_MAX 16" in h
    assert "typedef struct { const sv_fe* d_x; const sv_fe* d_y; sv_fe s; sv_fe c; uint32_t kind; } sv_fr_factor;" in h
    assert re.search(r"pub struct SvFrFactor \{\s*pub d_x: \*const SvFe,\s*pub d_y: \*const SvFe,\s*pub s: SvFe,"
                     r"\s*pub c: SvFe,\s*pub kind: u32,", rs)
    for const, value in (("SV_FACTOR_PLAIN", 0), ("SV_FACTOR_COLUMN", 1), ("SV_FACTOR_IDENTITY", 2),
                         ("SV_PRODUCT_FACTORS_MAX", 16)):
        assert re.search(r"pub const %s: \w+ = %d;" % (const, value), rs), const
    # the struct as the C compiler lays it out: two pointers, two elements, the kind, padded to 8
    assert ctypes.sizeof(_lib.sv_fr_factor) == 88
    assert _lib.sv_fr_factor.s.offset == 16 and _lib.sv_fr_factor.c.offset == 48 and _lib.sv_fr_factor.kind.offset == 80


def test_rule_1_form_null_kind_and_alignment_come_first():
    _arg(_gp(form=7), "bad form")
    _arg(_gp(d_z=None), "null")
    _arg(_gp(z0=None), "null")
    _arg(_gp(num_arr=None, n_num=1), "null")
    _arg(_gp(den_arr=None, n_den=2), "null")
    _arg(_gp(num=[plain(x=None)]), "null")
    _arg(_gp(den=[plain(), plain(x=None)]), "null")
    _arg(_gp(num=[column(y=None)]), "null")
    _arg(_gp(den=[column(y=None)]), "null")
    for kind in (3, 7, 0xFFFFFFFF):
        _arg(_gp(num=[(kind, _X, _Y, _ONE, _ZERO)]), "kind")
        _arg(_gp(den=[plain(), (kind, _X, _Y, _ONE, _ZERO)]), "kind")
    for off in (8, 4, 1):
        _arg(_gp(num=[plain(x=_X + off)]), "aligned")
        _arg(_gp(num=[column(y=_Y + off)]), "aligned")
        _arg(_gp(den=[identity(x=_X + off)]), "aligned")
        _arg(_gp(d_z=_Z + off), "aligned")
    # a NULL array with a zero count, the d_y of a factor that is not COLUMN and a NULL out_total are
    # not looked at: these calls fail on later rules
    assert _gp(num_arr=None, n_num=0, den=[plain()], n=0) == _lib.SV_ERR_EMPTY
    assert _gp(num=[(PLAIN, _X, 8, _ZERO, _ZERO), (IDENTITY, _X, 4, _ONE, _ZERO)], n=0, total=None) == _lib.SV_ERR_EMPTY
    # ... before emptiness, the length and the scalars; the form before everything
    _arg(_gp(form=7, d_z=None, n=0), "bad form")
    _arg(_gp(d_z=None, n=0, z0=_BAD[0]), "null")
    _arg(_gp(num=[plain(x=None, c=_BAD[0])], n=(1 << 26) + 1), "null")
    _arg(_gp(num=[(5, _X, None, _BAD[1], _BAD[1])], n=0), "kind")
    _arg(_gp(d_z=_Z + 8, n=0, n_den=40, den_arr=_factors([plain()] * 16)), "aligned")


def test_rule_2_empty_then_rule_3_length():
    for form in (0, 1):
        assert _gp(n=0, form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _gp(num=[], den=[], form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _gp(num=[], den=[], n=0, z0=_BAD[0], form=form) == _lib.SV_ERR_EMPTY
        # emptiness before the length and before the scalars
        assert _gp(n=0, n_num=MAX + 1, num_arr=_factors([plain()] * (MAX + 1)), form=form) == _lib.SV_ERR_EMPTY
        assert _gp(n=0, num=[plain(c=_BAD[2])], form=form) == _lib.SV_ERR_EMPTY
        for n in ((1 << 26) + 1, 1 << 40, (1 << 64) - 1):
            assert _gp(n=n, form=form) == _lib.SV_ERR_LEN, n
            assert "2^26" in _lib.last_error()
        seventeen = _factors([plain()] * (MAX + 1))
        assert _gp(num_arr=seventeen, n_num=MAX + 1, form=form) == _lib.SV_ERR_LEN
        assert str(MAX) in _lib.last_error()
        assert _gp(den_arr=seventeen, n_den=MAX + 1, form=form) == _lib.SV_ERR_LEN
        # a count far beyond the array: only the first SV_PRODUCT_FACTORS_MAX descriptors are looked at
        assert _gp(num_arr=_factors([plain()] * MAX), n_num=1 << 62, form=form) == _lib.SV_ERR_LEN
        # the length before the scalars, omega and the overlap
        assert _gp(n=(1 << 26) + 1, z0=_BAD[0], form=form) == _lib.SV_ERR_LEN
        assert _gp(num_arr=seventeen, n_num=MAX + 1, den=[identity()], d_z=_X, form=form) == _lib.SV_ERR_LEN


def test_rule_4_scalars_not_reduced():
    for form in (0, 1):
        for bad in _BAD:
            _arg(_gp(z0=bad, form=form), "not reduced")
            _arg(_gp(num=[plain(c=bad)], form=form), "not reduced")
            _arg(_gp(den=[plain(), plain(c=bad)], form=form), "not reduced")
            _arg(_gp(num=[column(s=bad)], form=form), "not reduced")
            _arg(_gp(den=[identity(s=bad)], omega=_W, form=form), "not reduced")
            _arg(_gp(num=[identity()], omega=bad, form=form), "not reduced")
            # ... before the missing omega and before the overlap
            _arg(_gp(num=[identity(c=bad)], omega=None, form=form), "not reduced")
            _arg(_gp(z0=bad, d_z=_X, form=form), "not reduced")
            _arg(_gp(num=[column(c=bad)], d_z=_Y + 32, form=form), "not reduced")


def test_rule_5_identity_needs_omega_then_rule_6_overlap():
    for form in (0, 1):
        _arg(_gp(num=[identity()], form=form), "omega")
        _arg(_gp(num=[plain()], den=[plain(), identity()], form=form), "omega")
        _arg(_gp(num=[identity()], d_z=_X, form=form), "omega")           # before the overlap
        # n = 2: d_z on, one element into, and one element in front of a column
        for d_z in (_X, _X + 32, _X - 32):
            _arg(_gp(d_z=d_z, form=form), "overlaps")
            _arg(_gp(num=[plain(x=_Y)], den=[plain(x=_X)], d_z=d_z, form=form), "overlaps")
            _arg(_gp(num=[identity(x=_X)], omega=_W, d_z=d_z, form=form), "overlaps")
        for d_z in (_Y, _Y + 32, _Y - 32):
            _arg(_gp(den=[column()], d_z=d_z, form=form), "overlaps")
        _arg(_gp(num=[plain(x=_X)] * 3 + [plain(x=_Z + 64)], n=4, form=form), "overlaps")


def test_batch_invert_rules_in_order():
    _arg(_inv(form=7), "bad form")
    _arg(_inv(d_in=None), "null")
    _arg(_inv(d_out=None), "null")
    for off in (8, 4, 1):
        _arg(_inv(d_in=_X + off), "aligned")
        _arg(_inv(d_out=_X + off), "aligned")
    _arg(_inv(form=7, d_in=None, n=0), "bad form")
    _arg(_inv(d_in=None, n=0), "null")
    _arg(_inv(d_out=_X + 8, n=0), "aligned")
    for form in (0, 1):
        assert _inv(n=0, form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _inv(n=0, d_out=_X + 32, form=form) == _lib.SV_ERR_EMPTY
        for n in ((1 << 26) + 1, (1 << 64) - 1):
            assert _inv(n=n, form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()
        assert _inv(n=(1 << 26) + 1, d_out=_X + 32, form=form) == _lib.SV_ERR_LEN      # the length before the overlap
        for d_out in (_X + 32, _X - 32, _X + 16):
            _arg(_inv(d_out=d_out, form=form), "overlaps")
        _arg(_inv(d_out=_X + 64, n=3, form=form), "overlaps")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    for form in (0, 1):
        assert _gp(form=form) == _lib.SV_ERR_DEVICE
        assert _gp(num=[], den=[plain()], total=None, form=form) == _lib.SV_ERR_DEVICE
        assert _gp(num=[identity()] * MAX, den=[column()] * MAX, omega=_W, n=8, form=form) == _lib.SV_ERR_DEVICE
        assert _gp(num=[plain(s=_BAD[0])], form=form) == _lib.SV_ERR_DEVICE          # the s of a PLAIN factor is not read
        assert _gp(num=[plain()], omega=_BAD[0], form=form) == _lib.SV_ERR_DEVICE     # nor omega without IDENTITY
        assert _gp(d_z=_X + 64, form=form) == _lib.SV_ERR_DEVICE                      # starts where the column ends
        assert _inv(form=form) == _lib.SV_ERR_DEVICE                                  # in place
        assert _inv(d_out=_X + 64, form=form) == _lib.SV_ERR_DEVICE
        assert _inv(d_in=_X + 64, d_out=_X, form=form) == _lib.SV_ERR_DEVICE


class _Col:
    """Stands for a column tensor: the builders only pass it on."""

    def __init__(self, name):
        self.name = name


def test_builders_assemble_the_two_relations(monkeypatch):
    import svgpu
    from svgpu import device as dv
    beta, gamma, delta = 0x1234567, 0x89ABCDE, 7
    v, s = [_Col(f"v{j}") for j in range(3)], [_Col(f"sigma{j}") for j in range(3)]
    dp = [pow(delta, 5 + j, b.R) for j in range(3)]                     # a later chunk: delta^5 ..
    num, den = svgpu.permutation_factors(v, s, beta, gamma, dp)
    # z(wX) prod (v + beta sigma + gamma) = z(X) prod (v + beta delta^j X + gamma)
    assert [tuple(f) for f in num] == [(IDENTITY, v[j], None, beta * dp[j] % b.R, gamma) for j in range(3)]
    assert [tuple(f) for f in den] == [(COLUMN, v[j], s[j], beta, gamma) for j in range(3)]
    with pytest.raises(svgpu.LengthError):
        svgpu.permutation_factors(v, s[:2], beta, gamma, dp)
    a, t, ap, tp = (_Col(x) for x in ("a", "s", "a'", "s'"))
    num, den = svgpu.lookup_factors(a, t, ap, tp, beta, gamma)
    # z(wX) (a' + beta)(s' + gamma) = z(X) (a + beta)(s + gamma)
    assert [tuple(f) for f in num] == [(PLAIN, a, None, 0, beta), (PLAIN, t, None, 0, gamma)]
    assert [tuple(f) for f in den] == [(PLAIN, ap, None, 0, beta), (PLAIN, tp, None, 0, gamma)]
    # every list is a Factor's fields
    for f in num + den:
        assert dv.Factor(*f).kind == PLAIN
    # the two *_product builders hand exactly these lists to grand_product_device
    seen = []
    monkeypatch.setattr(dv, "grand_product_device", lambda num, den, **kw: seen.append((num, den, kw)) or ("z", 1))
    assert svgpu.permutation_product(v, s, beta, gamma, dp, omega=5, z0=9, form=0) == ("z", 1)
    assert svgpu.lookup_product(a, t, ap, tp, beta, gamma, out="o") == ("z", 1)
    assert seen[0] == (*svgpu.permutation_factors(v, s, beta, gamma, dp), dict(z0=9, omega=5, form=0))
    assert seen[1] == (*svgpu.lookup_factors(a, t, ap, tp, beta, gamma), dict(z0=1, out="o"))
    assert callable(svgpu.grand_product_device) and callable(svgpu.batch_invert_device)
