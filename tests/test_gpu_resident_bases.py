"""Resident base sets (sv_bn254_g1_bases_create / sv_bn254_g1_msm_bases, svgpu.ResidentBases): N
points uploaded once, then MSMs over slices [offset, offset + n) of the set from scalars alone, on
the host-scalar and the device-scalar entry points.  Every expected value is the C++ oracle's
Pippenger over the sliced inputs, and is also what the plain sv_bn254_g1_msm gives for them.

The slices are the smallest shapes that cross every route boundary: the small-MSM route (<= 256
terms), the first pipeline size, the last size without GLV and the first with it (the phi records
sit at stride N, not n, behind a nonzero offset), a size that splits into several host-fed pieces
(one by default below 2^18 terms; test_environment_switches forces 2 and 3 pieces and the default
schedules' weights 1,3 and 1,3,4 on it), and a slice ending at N."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import bn254 as b

pytestmark = pytest.mark.gpu

N = 70000
SLICES = [(0, N), (3, 1), (100, 256), (5, 257), (1000, 16383), (12345, 16384), (37, 40000), (N - 5000, 5000)]
EDGE = [0, 1, 2, b.R - 1, b.R - 2, (b.R - 1) // 2, 1 << 127, (1 << 127) - 1, 1 << 128, b.R >> 1]
_UNREDUCED = np.array([0xffffffffffffffff] * 3 + [0x3fffffffffffffff], np.uint64)  # >= p and >= r, below 2^254


def _pt(raw):
    return b.g1_from_bytes(raw.tobytes())


def _to_mont(a, mod):
    """Canonical limbs -> Montgomery limbs (x 2^256 mod `mod`); identity points stay (0, 0)."""
    words = a.reshape(-1, 4)
    out = np.zeros_like(words)
    for i, w in enumerate(words):
        v = int.from_bytes(w.tobytes(), "little")
        out[i] = np.frombuffer(((v << 256) % mod).to_bytes(32, "little"), np.uint64)
    return out.reshape(a.shape)


class _Case:
    """The base set, three scalar vectors and the oracle's value per (vector, offset, n), computed
    once and shared (nothing here is modified by a test)."""

    def __init__(self, oracle_cpp):
        from svgpu import encoding as enc
        self.oracle = oracle_cpp
        B = oracle_cpp.gen_bases(b.SEED_BASES, N)
        self.Bgen = B.copy()          # the generator's output as it is (what dv.gen_bases writes)
        B[0] = 0                      # identity
        B[11] = B[10]                 # equal rows
        x, y = enc.g1_from_limbs(B[11])
        B[12] = enc.bases_array([(x, b.P - y)])[0]  # minus row 11
        self.B = B
        self.S = []
        for k in range(3):
            S = oracle_cpp.gen_scalars(b.SEED_SCALARS, N, start=k * N)
            S[:len(EDGE)] = enc.scalars_array(EDGE[k:] + EDGE[:k])
            self.S.append(S)
        self._exp = {}
        self._mont = {}

    def scalars(self, n, k=0):
        return self.S[k][:n]

    def exp(self, off, n, k=0):
        key = (off, n, k)
        if key not in self._exp:
            self._exp[key] = _pt(self.oracle.msm_pippenger(self.B[off:off + n], self.scalars(n, k), 0))
        return self._exp[key]

    def mont_bases(self):
        if "B" not in self._mont:
            self._mont["B"] = _to_mont(self.B, b.P)
        return self._mont["B"]

    def mont_scalars(self, n, k=0):
        if (n, k) not in self._mont:
            self._mont[(n, k)] = _to_mont(self.scalars(n, k), b.R)
        return self._mont[(n, k)]


@pytest.fixture(scope="module")
def case(oracle_cpp):
    return _Case(oracle_cpp)


@pytest.fixture(scope="module")
def rset(gpu, case):
    import svgpu
    with svgpu.ResidentBases(case.B) as s:
        yield s


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(gpu)


def test_info(gpu, rset):
    assert rset.n == N
    assert rset.device == 0
    assert rset.device_bytes >= 208 * N


@pytest.mark.parametrize("off,n", SLICES)
def test_slices_host_and_device_scalars(gpu, case, rset, off, n):
    import svgpu
    exp = case.exp(off, n)
    S = case.scalars(n)
    assert svgpu.msm_arrays(case.B[off:off + n], S) == exp      # the oracle and the plain entry point agree
    assert rset.msm_arrays(S, offset=off) == exp
    assert rset.msm_device(_dev(S, gpu), offset=off, form=svgpu.SV_CANONICAL) == exp
    from svgpu import device as dv
    st = dv.last_msm_stats()
    if n > 256:  # filled in like the other MSM calls (the small route zeroes them, as it does there)
        assert st["entries"] > 0 and st["num_windows"] > 0 and st["accumulate_ms"] > 0


@pytest.mark.parametrize("bases_form", ["canonical", "montgomery"])
@pytest.mark.parametrize("scalar_form", ["canonical", "montgomery"])
def test_forms(gpu, case, rset, bases_form, scalar_form):
    import svgpu
    sform = svgpu.SV_MONTGOMERY if scalar_form == "montgomery" else svgpu.SV_CANONICAL
    s = rset if bases_form == "canonical" else svgpu.ResidentBases(case.mont_bases(), form=svgpu.SV_MONTGOMERY)
    try:
        for off, n in ((12345, 16384), (100, 256), (5, 257)):
            S = case.mont_scalars(n) if sform == svgpu.SV_MONTGOMERY else case.scalars(n)
            assert s.msm_arrays(S, offset=off, form=sform) == case.exp(off, n), (off, n)
            assert s.msm_device(_dev(S, gpu), offset=off, form=sform) == case.exp(off, n), (off, n)
    finally:
        if s is not rset:
            s.close()


@pytest.mark.parametrize("env", [("SVGPU_H2D_PIECES", "1"), ("SVGPU_H2D_PIECES", "2"), ("SVGPU_H2D_PIECES", "3"),
                                 ("SVGPU_H2D_SPLIT", "1,7,1"), ("SVGPU_H2D_SPLIT", "1,3"), ("SVGPU_H2D_SPLIT", "1,3,4"),
                                 ("SVGPU_GLV", "0"), ("SVGPU_GLV", "1"), ("SVGPU_SORT_E32", "0")])
def test_environment_switches(gpu, case, rset, monkeypatch, env):
    import svgpu
    monkeypatch.setenv(*env)
    off, n = 37, 40000
    assert rset.msm_arrays(case.scalars(n), offset=off) == case.exp(off, n)
    assert rset.msm_device(_dev(case.scalars(n), gpu), offset=off, form=svgpu.SV_CANONICAL) == case.exp(off, n)


def test_small_route_switched_off(gpu, case, rset, monkeypatch):
    import svgpu
    monkeypatch.setenv("SVGPU_SMALL_MSM", "0")
    off, n = 100, 256
    assert rset.msm_arrays(case.scalars(n), offset=off) == case.exp(off, n)
    assert rset.msm_device(_dev(case.scalars(n), gpu), offset=off, form=svgpu.SV_CANONICAL) == case.exp(off, n)


def test_acc_r29_switch_does_not_apply(gpu, case, rset, monkeypatch):
    """A set holds only the 29-bit table: its calls keep that chain whatever SVGPU_ACC_R29 says."""
    monkeypatch.setenv("SVGPU_ACC_R29", "0")
    off, n = 12345, 16384
    assert rset.msm_arrays(case.scalars(n), offset=off) == case.exp(off, n)


def test_reuse_leaves_the_set_unchanged(gpu, case, rset):
    """Three scalar vectors through one handle, a plain MSM in between: a call that wrote into the
    set or left state in it would show in the next one."""
    import svgpu
    off, n = 12345, 16384
    for k in range(3):
        assert rset.msm_arrays(case.scalars(n, k), offset=off) == case.exp(off, n, k), k
        assert svgpu.msm_arrays(case.B[:5000], case.scalars(5000, k)) == case.exp(0, 5000, k), k
    assert rset.msm_arrays(case.scalars(N), offset=0) == case.exp(0, N)


def test_from_device_generator_output(gpu, case):
    """A set made from rows already in HBM (the device generator's output, both forms) gives what the
    host-created set gives wherever the two hold the same rows."""
    import svgpu
    from svgpu import device as dv
    for form in (svgpu.SV_MONTGOMERY, svgpu.SV_CANONICAL):
        rows = dv.gen_bases(dv.empty_bases(N, gpu), b.SEED_BASES, 0, form)
        with svgpu.ResidentBases.from_device(rows, form) as s:
            del rows  # the set keeps its own copy
            assert (s.n, s.device) == (N, 0) and s.device_bytes >= 208 * N
            for off, n in ((12345, 16384), (100, 256), (N - 5000, 5000)):  # rows the test set left as generated
                assert s.msm_arrays(case.scalars(n), offset=off) == case.exp(off, n), (form, off, n)
                assert s.msm_device(_dev(case.mont_scalars(n), gpu), offset=off) == case.exp(off, n), (form, off, n)
            whole = _pt(case.oracle.msm_pippenger(case.Bgen, case.scalars(N), 0))
            assert s.msm_arrays(case.scalars(N)) == whole


def test_unreduced_bases_rejected_at_create(gpu, case):
    import svgpu
    Bm = case.mont_bases()
    for form, rows in ((svgpu.SV_CANONICAL, case.B), (svgpu.SV_MONTGOMERY, Bm)):
        for coord in (0, 4):  # x, y
            bad = rows.copy()
            bad[N // 2, coord:coord + 4] = _UNREDUCED
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                svgpu.ResidentBases(bad, form=form)
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                svgpu.ResidentBases.from_device(_dev(bad, gpu), form)
    # a later create succeeds and holds its own rows only
    with svgpu.ResidentBases(case.B[:3000]) as s:
        assert (s.n, s.device_bytes) == (3000, 208 * 3000)
        assert s.msm_arrays(case.scalars(3000)) == _pt(case.oracle.msm_pippenger(case.B[:3000], case.scalars(3000), 0))


def test_unreduced_scalar_rejected_and_handle_stays_usable(gpu, case, rset):
    import svgpu
    for off, n in ((12345, 16384), (100, 256)):
        bad = case.scalars(n).copy()
        bad[n // 3] = _UNREDUCED
        with pytest.raises(svgpu.ArgumentError):
            rset.msm_arrays(bad, offset=off)
        with pytest.raises(svgpu.ArgumentError):
            rset.msm_device(_dev(bad, gpu), offset=off, form=svgpu.SV_CANONICAL)
        assert rset.msm_arrays(case.scalars(n), offset=off) == case.exp(off, n)


def test_range_and_handle_kinds(gpu, case, rset):
    import ctypes
    import svgpu
    from svgpu import _lib
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.msm_arrays(case.scalars(5001), offset=N - 5000)      # offset + n = N + 1
    with pytest.raises(svgpu.ArgumentError):
        rset.msm_arrays(case.scalars(1), offset=N)
    assert rset.msm_arrays(case.scalars(1, 1), offset=N - 1) == _pt(
        case.oracle.msm_pippenger(case.B[N - 1:], case.scalars(1, 1), 0))  # (scalar 1: the row itself)
    # a base table's handle is no base set's, and the reverse
    out = _lib.sv_g1_affine()
    S = case.scalars(4)
    with svgpu.BaseTable(case.B[:8]) as t:
        assert _lib.lib.sv_bn254_g1_msm_bases(t.handle, 0, S.ctypes.data, 4, 0, ctypes.byref(out)) == _lib.SV_ERR_ARG
        assert "unknown base set handle" in _lib.last_error()
        assert _lib.lib.sv_bn254_g1_bases_destroy(t.handle) == _lib.SV_ERR_ARG
        d = ctypes.c_int(-1)
        assert _lib.lib.sv_bn254_g1_table_device(rset.handle, ctypes.byref(d)) == _lib.SV_ERR_ARG
    # a destroyed handle is unknown
    s = svgpu.ResidentBases(case.B[:300])
    h = s.handle
    s.close()
    assert _lib.lib.sv_bn254_g1_msm_bases(h, 0, S.ctypes.data, 4, 0, ctypes.byref(out)) == _lib.SV_ERR_ARG
    assert _lib.lib.sv_bn254_g1_bases_destroy(h) == _lib.SV_ERR_ARG


def test_two_threads_share_one_handle(gpu, case, rset):
    """The set is read-only: concurrent calls on one handle (each with its own workspace) agree with
    the oracle.  ctypes releases the GIL around every foreign call, so the calls overlap."""
    jobs = [[(12345, 16384), (100, 256), (37, 40000), (5, 257)],
            [(1000, 16383), (N - 5000, 5000), (12345, 16384), (3, 1)]]
    for js in jobs:
        for off, n in js:
            case.exp(off, n)  # the oracle's values first, outside the threads

    def run(js):
        return [rset.msm_arrays(case.scalars(n), offset=off) == case.exp(off, n) for off, n in js]

    with ThreadPoolExecutor(max_workers=2) as ex:
        results = list(ex.map(run, jobs))
    assert all(all(r) for r in results), results
