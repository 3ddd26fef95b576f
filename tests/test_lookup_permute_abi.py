"""The Fr sort and the lookup permutation (sv_bn254_fr_sort_device,
sv_bn254_fr_lookup_permute_device; include/svgpu.h) without a GPU: both symbols in the library, the
ctypes table and the Rust crate; every argument rule in the documented order -- 1 form / null /
alignment, 2 empty, 3 length, 4 overlap -- each with its code and message word; the header's tile
constants; and the Python wrappers' names.  Every call below except the last test's is invalid
through the rule under test, so none reaches a device where there is one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT
from svgpu import _lib

_BUF = np.zeros(512, np.uint64)
_P = (_BUF.ctypes.data + 15) & ~15          # 16-byte aligned; four disjoint runs of 8 elements
_A, _S, _AP, _SP = _P, _P + 512, _P + 1024, _P + 1536
E = 32                                       # bytes per element


def _sort(d_in=_A, d_out=_A, n=2, form=0):
    return _lib.lib.sv_bn254_fr_sort_device(d_in, d_out, n, form, 0, None)


def _perm(a=_A, s=_S, n=2, form=0, ap=_AP, sp=_SP, row=True):
    out = ctypes.c_uint64(7)
    return _lib.lib.sv_bn254_fr_lookup_permute_device(a, s, n, form, ap, sp, ctypes.byref(out) if row else None, 0, None)


def _arg(rc, word):
    assert rc == _lib.SV_ERR_ARG, (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def test_symbols_in_library_ctypes_table_header_and_crate():
    names = {"sv_bn254_fr_sort_device": 6, "sv_bn254_fr_lookup_permute_device": 9}
    table = {p[0]: p for p in _lib.PROTOTYPES}
    rs = open(os.path.join(ROOT, "snark-verifier-gpu", "src", "lib.rs")).read()
    h = open(os.path.join(ROOT, "include", "svgpu.h")).read()
    for name, params in names.items():
        assert hasattr(_lib.lib, name)
        assert len(table[name][2]) == params
        m = re.search(r"pub fn %s\(([^)]*)\)" % name, rs, flags=re.S)
        assert m and m.group(1).count(",") + 1 == params
        m = re.search(r"int %s\(([^)]*)\) SV_NOEXCEPT;" % name, h, flags=re.S)
        assert m and m.group(1).count(",") + 1 == params
    hpp = open(os.path.join(PKG, "csrc", "lookup_permute.hpp")).read()
    tile = int(re.search(r"constexpr uint32_t kLpTile = (\d+);", hpp).group(1))
    threads = int(re.search(r"constexpr uint32_t kLpThreads = (\d+);", hpp).group(1))
    assert tile % threads == 0 and threads % 64 == 0
    assert "lookup_permute_scratch_bytes(size_t n, bool permute)" in hpp and "lookup_permute_enqueue(" in hpp
    assert "csrc/lookup_permute.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_sort_rules_in_order():
    _arg(_sort(form=7), "bad form")
    _arg(_sort(d_in=None), "null")
    _arg(_sort(d_out=None), "null")
    for off in (8, 4, 1):
        _arg(_sort(d_in=_A + off), "aligned")
        _arg(_sort(d_out=_A + off), "aligned")
    # rule 1 before emptiness and the length; the form before everything
    _arg(_sort(form=7, d_in=None, n=0), "bad form")
    _arg(_sort(d_in=None, n=0), "null")
    _arg(_sort(d_out=_A + 8, n=(1 << 26) + 1), "aligned")
    for form in (0, 1):
        assert _sort(n=0, form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _sort(n=0, d_out=_A + E, form=form) == _lib.SV_ERR_EMPTY          # emptiness before the overlap
        for n in ((1 << 26) + 1, 1 << 40, (1 << 64) - 1):
            assert _sort(n=n, form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()
        assert _sort(n=(1 << 26) + 1, d_out=_A + E, form=form) == _lib.SV_ERR_LEN  # the length before the overlap
        for d_out in (_A + E, _A - E, _A + 16):
            _arg(_sort(d_out=d_out, form=form), "overlaps")
        _arg(_sort(d_out=_A + 2 * E, n=3, form=form), "overlaps")


def test_lookup_permute_rules_in_order():
    _arg(_perm(form=7), "bad form")
    for name in ("a", "s", "ap", "sp"):
        _arg(_perm(**{name: None}), "null")
        for off in (8, 4, 1):
            _arg(_perm(**{name: _P + 2048 + off}), "aligned")
    _arg(_perm(form=7, a=None, n=0), "bad form")
    _arg(_perm(sp=None, n=0), "null")
    _arg(_perm(ap=_AP + 8, n=(1 << 26) + 1), "aligned")
    for form in (0, 1):
        assert _perm(n=0, form=form) == _lib.SV_ERR_EMPTY
        assert "empty" in _lib.last_error()
        assert _perm(n=0, ap=_A, form=form) == _lib.SV_ERR_EMPTY                  # emptiness before the overlap
        for n in ((1 << 26) + 1, (1 << 64) - 1):
            assert _perm(n=n, form=form) == _lib.SV_ERR_LEN
            assert "2^26" in _lib.last_error()
        assert _perm(n=(1 << 26) + 1, sp=_S, form=form) == _lib.SV_ERR_LEN         # the length before the overlap
        # every refused aliasing at n = 2: an output on, one element into and one element in front
        # of an input; the two outputs on each other
        for inp in (_A, _S):
            for off in (0, E, -E):
                _arg(_perm(ap=inp + off, form=form), "overlaps")
                _arg(_perm(sp=inp + off, form=form), "overlaps")
        for off in (0, E, -E):
            _arg(_perm(sp=_AP + off, form=form), "overlaps")
        _arg(_perm(sp=_AP, row=False, form=form), "overlaps")
    # the inputs may be one column (A looked up in itself): not an overlap, so this call fails only on its length
    assert _perm(s=_A, n=(1 << 26) + 1) == _lib.SV_ERR_LEN


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_valid_calls_get_device_error_without_a_gpu():
    for form in (0, 1):
        assert _sort(form=form) == _lib.SV_ERR_DEVICE                              # in place
        assert _sort(d_out=_A + 2 * E, form=form) == _lib.SV_ERR_DEVICE            # starts where the column ends
        assert _perm(form=form) == _lib.SV_ERR_DEVICE
        assert _perm(row=False, form=form) == _lib.SV_ERR_DEVICE
        assert _perm(s=_A, form=form) == _lib.SV_ERR_DEVICE                        # the two inputs may coincide
        assert _perm(ap=_A + 2 * E, sp=_A + 4 * E, s=_A + 6 * E, form=form) == _lib.SV_ERR_DEVICE


def test_python_wrappers_are_exported(monkeypatch):
    import svgpu
    from svgpu import device as dv
    for name in ("sort_device", "lookup_permute_device"):
        assert callable(getattr(svgpu, name)) and callable(getattr(dv, name))
    # lookup_argument is the permutation followed by the existing lookup_product on its output
    seen = []
    monkeypatch.setattr(dv, "lookup_permute_device", lambda a, s, **kw: seen.append(("permute", a, s, kw)) or ("a'", "s'"))
    monkeypatch.setattr(svgpu, "lookup_product",
                        lambda a, s, ap, sp, beta, gamma, **kw: seen.append(("product", a, s, ap, sp, beta, gamma, kw)) or ("z", 9))
    assert svgpu.lookup_argument("a", "s", 3, 4, z0=9, form=0) == ("a'", "s'", "z", 9)
    assert seen == [("permute", "a", "s", dict(out=None, form=0)),
                    ("product", "a", "s", "a'", "s'", 3, 4, dict(z0=9, form=0))]
