"""The device build of the 29-bit-limb field and XYZZ chain (csrc/field29.hpp, csrc/curve29.hpp) as a
unit, against Python integers and the oracle's affine group law.

The host build (tests/test_field29.py) is not the device build: is_zero_mod_p_16p's multiple
estimate is one fused multiply-add on the GPU and two roundings on the host, and the MSM, Poseidon
and decider tests reach the device code only with the values random points produce -- a handful of
multiples k p, never operands near the stated 12p / 10p / 9p / 8p bounds.  This runs the cases of
tests/f29_cases.py (every operation at its stated bounds, every multiple k p for k < 16 with its
neighbours, chain states with X up to x + 7p, doubling, cancellation, clean and garbage
identities) through tests/native/field29dev.hip (test-only, built by __graft_entry__.build()): one
thread per case, one kernel per operation, the same checker as the host tests.
"""
import ctypes
import os

import numpy as np
import pytest

import f29_cases as fc
from conftest import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "native", "build", "libfield29dev.so")


@pytest.fixture(scope="module")
def dev():
    assert os.path.exists(LIB), "tests/native/build/libfield29dev.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(LIB)
    lib.f29_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    lib.f29_run.restype = ctypes.c_int
    return lib


def _run(dev, op, field, rows, flags, n_out):
    a = np.ascontiguousarray(np.array(rows, dtype=np.uint32))
    fl = np.ascontiguousarray(np.array(flags, dtype=np.uint32))
    out = np.zeros((len(rows), 9 * n_out), np.uint32)
    rc = dev.f29_run(op, field, a.ctypes.data, out.ctypes.data, fl.ctypes.data, len(rows))
    assert rc == 0, f"f29_run hip error {rc}"
    return out.tolist(), fl.tolist()


@pytest.mark.parametrize("name,field", fc.FIELD_CASES, ids=["%s-%s" % c for c in fc.FIELD_CASES])
def test_field_op_at_stated_bounds(gpu, dev, name, field):
    rows, flags = fc.field_rows(name, field)
    out, fo = _run(dev, fc.OPS[name].id, fc.FIELD_ID[field], rows, flags, 1)
    assert fc.check_field(name, field, out, fo) == len(rows) >= 2000  # zero cases skipped


@pytest.mark.parametrize("name,neg", fc.CURVE_CASES, ids=["%s-neg%d" % c for c in fc.CURVE_CASES])
def test_curve_op_chosen_cases(gpu, dev, name, neg):
    rows, flags = fc.curve_rows(name, neg)
    out, fo = _run(dev, fc.CURVE_IDS[name], 0, rows, flags, 4)
    assert fc.check_curve(name, neg, out, fo) == len(rows)


def test_bad_arguments_are_refused(gpu, dev):
    """An operation that does not exist over Fr, or an unknown one, launches nothing."""
    buf = np.zeros(9 * 8, np.uint32)
    for op, field in ((fc.OPS["is_zero16"].id, 1), (fc.CURVE_IDS["xadd"], 1), (99, 0), (-1, 0)):
        assert dev.f29_run(op, field, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1) != 0
