"""The batched lookup permutation (sv_bn254_fr_lookup_permute_batch_device; include/svgpu.h) without
a GPU: the symbol in the library, the ctypes table, the header and the Rust crate with one parameter
list; the flag and the cap in all three; every argument rule in the documented order -- 1 form / flag
/ null array / null entry / alignment, 2 empty, 3 length, 4 overlap -- each with its code and message
word, and where two rules apply the lower-numbered one; and the Python wrappers' names.  Every call
below except the last test's is invalid through the rule under test, so none reaches a device where
there is one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from svgpu import _lib

NAME = "sv_bn254_fr_lookup_permute_batch_device"
E = 32                                       # bytes per element
_BUF = np.zeros(4096, np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15          # 16-byte aligned; disjoint runs of 8 elements


def _col(k):
    return _P + 256 * k


def _call(a=None, s=None, ap=None, sp=None, count=2, n=2, form=0, flags=0, rows=True, null=()):
    """Two lookups of two rows in disjoint columns unless told otherwise; `null` names arrays to pass as NULL."""
    a = [_col(0), _col(1)] if a is None else a
    s = [_col(2), _col(3)] if s is None else s
    ap = [_col(4), _col(5)] if ap is None else ap
    sp = [_col(6), _col(7)] if sp is None else sp
    arrays = {}
    for name, v in (("a", a), ("s", s), ("ap", ap), ("sp", sp)):
        arrays[name] = None if name in null else (ctypes.c_void_p * max(len(v), 1))(*v)
    out = (ctypes.c_uint64 * max(count, 1))(*([7] * max(count, 1))) if count <= 64 else None
    failed = ctypes.c_uint64(7)
    return _lib.lib.sv_bn254_fr_lookup_permute_batch_device(arrays["a"], arrays["s"], count, n, form, flags, arrays["ap"],
                                                            arrays["sp"], out if rows else None,
                                                            ctypes.byref(failed) if rows else None, 0, None)


def _arg(rc, word):
    assert rc == _lib.SV_ERR_ARG, (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def _cols(first, count):
    return [_col(first + j) for j in range(count)]


def _wide(count, **kw):
    """`count` lookups in disjoint columns."""
    return _call(a=_cols(0, count), s=_cols(20, count), ap=_cols(40, count), sp=_cols(60, count), count=count, **kw)


def test_symbol_in_library_ctypes_table_header_and_crate():
    table = {p[0]: p for p in _lib.PROTOTYPES}
    rs = open(os.path.join(ROOT, "snark-verifier-gpu", "src", "lib.rs")).read()
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    assert hasattr(_lib.lib, NAME)
    params = 12
    assert len(table[NAME][2]) == params and table[NAME][1] is ctypes.c_int
    hm = re.search(r"int %s\(([^)]*)\) SV_NOEXCEPT;" % NAME, h, flags=re.S)
    rm = re.search(r"pub fn %s\(([^)]*)\)\s*->\s*c_int;" % NAME, rs, flags=re.S)
    assert hm and rm
    hp = [" ".join(p.split()) for p in hm.group(1).split(",")]
    rp = [" ".join(p.split()) for p in rm.group(1).split(",")]
    assert len(hp) == params and len(rp) == params
    # the parameter names agree in order, and each type is the same thing in the three languages
    names = [re.search(r"(\w+)$", p).group(1) for p in hp]
    assert names == [p.split(":")[0].strip() for p in rp]
    assert names == ["d_inputs", "d_tables", "count", "n", "form", "flags", "d_permuted_inputs", "d_permuted_tables",
                     "out_missing_rows", "out_failed", "device", "stream"]
    kinds = {"const sv_fe* const*": ("*const *const SvFe", ctypes.c_void_p),
             "sv_fe* const*": ("*const *mut SvFe", ctypes.c_void_p),
             "size_t": ("usize", ctypes.c_size_t), "int": ("c_int", ctypes.c_int), "uint32_t": ("u32", ctypes.c_uint32),
             "uint64_t*": ("*mut u64", ctypes.POINTER(ctypes.c_uint64)), "void*": ("*mut c_void", ctypes.c_void_p)}
    for hpar, rpar, cty in zip(hp, rp, table[NAME][2]):
        ctype = hpar[:hpar.rindex(" ")]
        assert kinds[ctype] == (rpar.split(":")[1].strip(), cty), (hpar, rpar, cty)
    # the cap and the flag
    cap = int(re.search(r"#define SV_LOOKUP_BATCH_MAX (\d+)", h).group(1))
    assert cap == 16 == _lib.SV_LOOKUP_BATCH_MAX == _lib.SV_TERMS_LOOKUPS_MAX
    assert int(re.search(r"pub const SV_LOOKUP_BATCH_MAX: usize = (\d+);", rs).group(1)) == cap
    flag = int(re.search(r"enum \{ SV_LOOKUP_TABLES_SORTED = (\d+) \};", h).group(1))
    assert flag == 1 == _lib.SV_LOOKUP_TABLES_SORTED
    assert int(re.search(r"pub const SV_LOOKUP_TABLES_SORTED: u32 = (\d+);", rs).group(1)) == flag
    assert re.search(r"pub unsafe fn lookup_permute_batch_device\(", rs)


def test_rule_1_form_flags_nulls_and_alignment():
    _arg(_call(form=7), "bad form")
    _arg(_call(form=-1), "bad form")
    for flags in (2, 3, 4, 1 << 31):
        _arg(_call(flags=flags), "flag")
    for name in ("a", "s", "ap", "sp"):
        _arg(_call(null=(name,)), "null")
        for j in (0, 1):
            cols = [_col(10), _col(11)]
            cols[j] = None
            _arg(_call(**{name: cols}), "null")
            for off in (8, 4, 1):
                cols[j] = _col(12) + off
                _arg(_call(**{name: cols}), "aligned")
    # the form before everything else of rule 1
    _arg(_call(form=7, flags=2, null=("a",)), "bad form")


def test_rule_2_empty():
    for form in (0, 1):
        for kw in (dict(count=0), dict(n=0), dict(count=0, n=0)):
            assert _call(form=form, **kw) == _lib.SV_ERR_EMPTY
            assert "empty" in _lib.last_error()
        assert _call(count=0, a=[], s=[], ap=[], sp=[]) == _lib.SV_ERR_EMPTY


def test_rule_3_lengths():
    for form in (0, 1):
        assert _wide(17, form=form) == _lib.SV_ERR_LEN
        assert "SV_LOOKUP_BATCH_MAX" in _lib.last_error()
        for n in ((1 << 26) + 1, (1 << 40)):
            assert _call(n=n, form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()


def test_rule_4_overlaps():
    reads = [_col(0), _col(1), _col(2), _col(3)]
    for form in (0, 1):
        for which in ("ap", "sp"):
            for j in (0, 1):
                for target in reads:
                    for off in (0, E, -E, 16):                 # on, one element into, one in front of, half into
                        outs = [_col(8), _col(9)]
                        outs[j] = target + off
                        _arg(_call(form=form, **{which: outs}), "overlaps")
        # outputs on each other: within one array and across the two
        _arg(_call(ap=[_col(4), _col(4)], form=form), "overlaps")
        _arg(_call(sp=[_col(6), _col(6) + E], form=form), "overlaps")
        _arg(_call(sp=[_col(6), _col(5) - E], form=form), "overlaps")
        _arg(_call(sp=[_col(4), _col(7)], rows=False, form=form), "overlaps")


def test_the_lower_numbered_rule_wins():
    # 1 over 2, 3 and 4
    _arg(_call(form=7, n=0), "bad form")
    _arg(_call(flags=8, count=0), "flag")
    _arg(_call(null=("sp",), n=0), "null")
    _arg(_call(ap=[_col(4), _col(5) + 8], n=(1 << 26) + 1), "aligned")
    _arg(_call(a=[_col(0), None], ap=[_col(2), _col(5)]), "null")
    _arg(_wide(17, form=3), "bad form")
    cols = _cols(0, 17)
    cols[16] = None
    _arg(_call(a=cols, s=_cols(20, 17), ap=_cols(40, 17), sp=_cols(60, 17), count=17), "null")   # entry 16 is looked at
    # 2 over 3 and 4
    assert _wide(17, n=0) == _lib.SV_ERR_EMPTY
    assert _call(n=0, ap=[_col(0), _col(5)]) == _lib.SV_ERR_EMPTY
    # 3 over 4
    assert _call(n=(1 << 26) + 1, ap=[_col(0), _col(5)]) == _lib.SV_ERR_LEN
    assert _call(a=_cols(0, 17), s=_cols(20, 17), ap=_cols(0, 17), sp=_cols(60, 17), count=17) == _lib.SV_ERR_LEN


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    for form in (0, 1):
        for flags in (0, 1):
            assert _call(form=form, flags=flags) == _lib.SV_ERR_DEVICE
            assert _call(form=form, flags=flags, rows=False) == _lib.SV_ERR_DEVICE
            # what is legal: one table for both, one input for both, tables that overlap, an input that is a table
            assert _call(s=[_col(2), _col(2)], form=form, flags=flags) == _lib.SV_ERR_DEVICE
            assert _call(a=[_col(0), _col(0)], form=form, flags=flags) == _lib.SV_ERR_DEVICE
            assert _call(s=[_col(2), _col(2) + E], form=form, flags=flags) == _lib.SV_ERR_DEVICE
            assert _call(a=[_col(0), _col(2)], form=form, flags=flags) == _lib.SV_ERR_DEVICE
            assert _call(ap=[_col(4), _col(4) + 2 * E], form=form, flags=flags) == _lib.SV_ERR_DEVICE   # abutting outputs
            assert _wide(16, form=form, flags=flags) == _lib.SV_ERR_DEVICE


def test_python_wrappers_are_exported(monkeypatch):
    import svgpu
    from svgpu import device as dv
    assert callable(svgpu.lookup_permute_batch_device) and callable(dv.lookup_permute_batch_device)
    assert callable(svgpu.lookup_arguments)
    # lookup_arguments is one batch permutation followed by the existing lookup_product per lookup
    seen = []
    monkeypatch.setattr(svgpu, "lookup_permute_batch_device",
                        lambda a, s, **kw: seen.append(("permute", a, s, kw)) or [("a0'", "s0'"), ("a1'", "s1'")])
    monkeypatch.setattr(svgpu, "lookup_product",
                        lambda a, s, ap, sp, beta, gamma, **kw: seen.append(("product", a, s, ap, sp, beta, gamma, kw)) or ("z", 9))
    assert svgpu.lookup_arguments(["a0", "a1"], "s", 3, 4, z0=9, form=0, tables_sorted=True) == [
        ("a0'", "s0'", "z", 9), ("a1'", "s1'", "z", 9)]
    assert seen == [("permute", ["a0", "a1"], "s", dict(out=None, tables_sorted=True, form=0)),
                    ("product", "a0", "s", "a0'", "s0'", 3, 4, dict(z0=9, form=0)),
                    ("product", "a1", "s", "a1'", "s1'", 3, 4, dict(z0=9, form=0))]
