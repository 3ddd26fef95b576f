"""KZG opening on a resident base set: the division (p - p(z)) / (X - z) on the device
(sv_bn254_fr_poly_div_linear_device) and the openings that feed its quotient to the set's MSM
(sv_bn254_kzg_open, sv_bn254_kzg_open_device; svgpu.ResidentBases.open_arrays / open_device).

No expected value comes from the code under test: the quotient and the evaluation are the Python-int
Horner below, the witness is the C++ oracle's Pippenger over the sliced set and that quotient, and
the closing test hands the accumulator to the decider.  Everything is arithmetic mod r, so every
comparison is bit for bit.

Sizes.  The division's are placed around kDivSpan (S, read from csrc/kzg_open.hpp: the coefficients
per block) -- S - 1, S, S + 1, 2 S + 1 -- and around the one other size at which a loop count of the
scan changes, 256 S + 1 (the block that scans the block totals then takes two totals per thread; the
header says so next to kDivSpan).  The openings' (offset, n) give the witness MSM of n - 1 terms no
term, one term, the last small-route size (256) and the first pipeline size (257), the first GLV size
(16384), a several-block slice behind an odd offset, a slice that ends at the set's end, and the
whole set."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import PKG
from oracle import bn254 as b
from test_gpu_resident_bases import EDGE, N, _UNREDUCED, _Case

pytestmark = pytest.mark.gpu

S = int(re.search(r"constexpr uint32_t kDivSpan = (\d+);", open(os.path.join(PKG, "csrc", "kzg_open.hpp")).read()).group(1))
DIV_SIZES = [1, 2, 3, 257, S - 1, S, S + 1, 2 * S + 1, 300001, 256 * S + 1]
KINDS = ["generated", "zero", "first", "last"]
Z_GEN = b.gen_scalar(b.SEED_SCALARS, 987654321)
ZS = [0, 1, b.R - 1, Z_GEN]
OPENS = [(3, 1), (0, 2), (100, 257), (5, 258), (1000, 16385), (37, 40001), (N - 5000, 5001), (0, N + 1)]
CANONICAL, MONTGOMERY = 0, 1


def _horner(a, z):
    """h_i = a_i + z h_{i+1}, h_n = 0 -> (q = (h_1 .. h_{n-1}), p(z) = h_0)."""
    h, hs = 0, []
    for c in reversed(a):
        hs.append(h)
        h = (c + z * h) % b.R
    return hs[::-1][:-1], h


def _ints(limbs):
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _limb_bytes(values, form):
    if form == MONTGOMERY:
        values = [(v << 256) % b.R for v in values]
    return b"".join(v.to_bytes(32, "little") for v in values)


def _limbs(values, form):
    return np.frombuffer(_limb_bytes(values, form), np.uint64).reshape(len(values), 4).copy()


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(gpu)


def _div_coeffs(oracle_cpp, n, kind):
    if kind == "generated":
        a = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, n, start=7 * N))
        # the edge values, spread from index 0 to index n - 1 (the first of them when n is smaller)
        pos = [i * (n - 1) // (len(EDGE) - 1) for i in range(len(EDGE))] if n > len(EDGE) else range(n)
        for i, e in zip(pos, EDGE):
            a[i] = e
        return a
    a = [0] * n
    if kind == "first":
        a[0] = b.R - 2
    if kind == "last":
        a[n - 1] = b.R - 3
    return a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", DIV_SIZES)
def test_division_quotient_and_evaluation(gpu, oracle_cpp, n, kind):
    from svgpu import device as dv
    a = _div_coeffs(oracle_cpp, n, kind)
    A = {form: _dev(_limbs(a, form), gpu) for form in (CANONICAL, MONTGOMERY)}
    for z in ZS:
        q, v = _horner(a, z)
        assert len(q) == n - 1
        for form in (CANONICAL, MONTGOMERY):
            ev, Q = dv.poly_div_linear_device(A[form], z, form=form)
            assert ev == v, (n, kind, z, form)
            assert tuple(Q.shape) == (n - 1, 4)
            assert Q.cpu().numpy().tobytes() == _limb_bytes(q, form), (n, kind, z, form)
            ev_only, none = dv.poly_div_linear_device(A[form], z, form=form, quotient=False)  # d_quotient = NULL
            assert none is None and ev_only == v, (n, kind, z, form)


def test_division_rejects_a_quotient_over_the_coefficients(gpu, oracle_cpp):
    """Phase 3 reads the coefficients again while it writes the quotient, so a quotient that shares a
    row with them is an error (and nothing is written); one that ends right before them or starts
    right behind them is fine.  Coefficients in rows [n, 2 n) of a 3 n-row buffer, the quotient's
    n - 1 rows from row s: they overlap for 2 <= s <= 2 n - 1."""
    import svgpu
    from svgpu import device as dv
    n = S + 1
    a = _div_coeffs(oracle_cpp, n, "generated")
    rows = np.zeros((3 * n, 4), np.uint64)
    rows[n:2 * n] = _limbs(a, CANONICAL)
    buf = _dev(rows, gpu)
    for s in (2, n, n + 1, 2 * n - 1):
        with pytest.raises(svgpu.ArgumentError, match="overlaps"):
            dv.poly_div_linear_device(buf[n:2 * n], Z_GEN, form=CANONICAL, out=buf[s:])
    with pytest.raises(svgpu.LengthError):                    # the wrapper refuses a quotient tensor that is too short
        dv.poly_div_linear_device(buf[n:2 * n], Z_GEN, form=CANONICAL, out=buf[:n - 2])
    assert buf.cpu().numpy().tobytes() == rows.view(np.int64).tobytes()
    q, v = _horner(a, Z_GEN)
    for s in (1, 2 * n):
        ev, Q = dv.poly_div_linear_device(buf[n:2 * n], Z_GEN, form=CANONICAL, out=buf[s:])
        assert ev == v and Q.cpu().numpy().tobytes() == _limb_bytes(q, CANONICAL), s
    assert buf[n:2 * n].cpu().numpy().tobytes() == rows[n:2 * n].tobytes()


class _Open:
    """The resident-set tests' base set, four coefficient vectors of N + 2 rows and the expected
    opening per (vector, offset, n, z), computed once and shared (no test modifies any of it)."""

    def __init__(self, oracle_cpp):
        self.oracle = oracle_cpp
        self.B = _Case(oracle_cpp).B
        self.A = []
        for k in range(4):
            a = oracle_cpp.gen_scalars(b.SEED_SCALARS, N + 2, start=(10 + k) * (N + 2))
            a[:len(EDGE)] = _limbs(EDGE[k:] + EDGE[:k], CANONICAL)
            self.A.append(a)
        self._ints = {}
        self._mont = {}
        self._exp = {}

    def ints(self, k):
        if k not in self._ints:
            self._ints[k] = _ints(self.A[k])
        return self._ints[k]

    def mont(self, k, n):
        if (k, n) not in self._mont:
            self._mont[(k, n)] = _limbs(self.ints(k)[:n], MONTGOMERY)
        return self._mont[(k, n)]

    def witness(self, off, q):
        if not q:
            return None
        raw = self.oracle.msm_pippenger(self.B[off:off + len(q)], _limbs(q, CANONICAL), 0)
        return b.g1_from_bytes(raw.tobytes())

    def exp(self, off, n, k=0, z=Z_GEN):
        key = (off, n, k, z)
        if key not in self._exp:
            q, v = _horner(self.ints(k)[:n], z)
            self._exp[key] = (v, self.witness(off, q))
        return self._exp[key]


@pytest.fixture(scope="module")
def case(oracle_cpp):
    return _Open(oracle_cpp)


@pytest.fixture(scope="module")
def rset(gpu, case):
    import svgpu
    with svgpu.ResidentBases(case.B) as s:
        yield s


@pytest.mark.parametrize("off,n", OPENS)
def test_open_host_and_device_coefficients(gpu, case, rset, off, n):
    import svgpu
    from svgpu import device as dv
    exp = case.exp(off, n)
    if n == 1:
        assert exp == (case.ints(0)[0], None)  # no quotient term: p(z) = a_0, no MSM
    A = case.A[0][:n]
    assert rset.open_arrays(A, Z_GEN, offset=off) == exp
    if n - 1 > 256:  # the witness MSM's figures, as after sv_bn254_g1_msm_bases (the small route zeroes them)
        st = dv.last_msm_stats()
        assert st["entries"] > 0 and st["num_windows"] > 0 and st["accumulate_ms"] > 0
    assert rset.open_device(_dev(A, gpu), Z_GEN, offset=off, form=svgpu.SV_CANONICAL) == exp
    if n - 1 > 256:
        assert dv.last_msm_stats()["entries"] > 0


@pytest.mark.parametrize("off,n", [(100, 257), (5, 258), (1000, 16385)])
def test_mixed_forms_give_the_same_opening(gpu, case, rset, off, n):
    import svgpu
    exp = case.exp(off, n)
    Am = case.mont(0, n)
    assert rset.open_arrays(Am, Z_GEN, offset=off, form=svgpu.SV_MONTGOMERY) == exp
    assert rset.open_device(_dev(Am, gpu), Z_GEN, offset=off) == exp                      # Montgomery by default
    assert rset.open_device(_dev(case.A[0][:n], gpu), Z_GEN, offset=off, form=svgpu.SV_CANONICAL) == exp


@pytest.mark.parametrize("z", [0, 1, b.R - 1])
def test_open_at_the_edge_points(gpu, case, rset, z):
    off, n = 5, 258
    assert rset.open_arrays(case.A[1][:n], z, offset=off) == case.exp(off, n, 1, z)


def test_zero_polynomial_and_zero_quotient(gpu, case, rset):
    import svgpu
    for n in (1, 2, 258, 16385):
        zero = np.zeros((n, 4), np.uint64)
        assert rset.open_arrays(zero, Z_GEN, offset=7) == (0, None), n
        assert rset.open_device(_dev(zero, gpu), Z_GEN, offset=7) == (0, None), n
        const = zero.copy()  # a constant: p(z) = a_0, the quotient is all zero
        const[0] = _limbs([b.R - 5], CANONICAL)[0]
        assert rset.open_arrays(const, Z_GEN, offset=7) == (b.R - 5, None), n
        assert rset.open_device(_dev(const, gpu), Z_GEN, offset=7, form=svgpu.SV_CANONICAL) == (b.R - 5, None), n


def test_range_of_the_quotient_terms(gpu, case, rset):
    import svgpu
    A = case.A[0]
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_arrays(A[:N + 2], Z_GEN)                       # N + 1 quotient terms
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_device(_dev(A[:N + 2], gpu), Z_GEN, form=svgpu.SV_CANONICAL)
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_arrays(A[:5002], Z_GEN, offset=N - 5000)
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_arrays(A[:2], Z_GEN, offset=(1 << 64) - 1)     # no wrap near 2^64
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_arrays(A[:1], Z_GEN, offset=N + 1)
    v0 = case.ints(0)[0]
    assert rset.open_arrays(A[:1], Z_GEN, offset=N) == (v0, None)  # no quotient term: nothing past the end
    assert rset.open_arrays(A[:2], Z_GEN, offset=N - 1) == case.exp(N - 1, 2)
    # the handle is as usable as before
    assert rset.open_arrays(A[:258], Z_GEN, offset=5) == case.exp(5, 258)


def test_unreduced_coefficients_rejected_and_handle_stays_usable(gpu, case, rset):
    import svgpu
    from svgpu import device as dv
    off, n = 37, 2 * S + 1
    good = {svgpu.SV_CANONICAL: case.A[0][:n], svgpu.SV_MONTGOMERY: case.mont(0, n)}
    for form in (svgpu.SV_CANONICAL, svgpu.SV_MONTGOMERY):
        for idx in (0, S, n - 1):
            bad = good[form].copy()
            bad[idx] = _UNREDUCED
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                rset.open_arrays(bad, Z_GEN, offset=off, form=form)
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                rset.open_device(_dev(bad, gpu), Z_GEN, offset=off, form=form)
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                dv.poly_div_linear_device(_dev(bad, gpu), Z_GEN, form=form)
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                dv.poly_div_linear_device(_dev(bad, gpu), Z_GEN, form=form, quotient=False)
            # the next valid call on the same handle is exact
            assert rset.open_arrays(good[form], Z_GEN, offset=off, form=form) == case.exp(off, n), (form, idx)
    assert rset.open_device(_dev(good[svgpu.SV_MONTGOMERY], gpu), Z_GEN, offset=off) == case.exp(off, n)
    with pytest.raises(svgpu.ArgumentError, match="not reduced"):      # z, before any device work
        rset.open_arrays(good[svgpu.SV_CANONICAL], b.R, offset=off)


def test_commit_open_decide(gpu, oracle_cpp):
    """commit -> open -> decide on one handle over an SRS s^i g: lhs = C - v g + z pi, rhs = pi is an
    accumulator the decider accepts under (g, g2, s g2); with v + 1 in v's place it is not."""
    import svgpu
    n = 300
    s = b.gen_scalar(b.SEED_TRAPDOOR, 1)
    z = b.gen_scalar(b.SEED_SCALARS, 424243)
    srs, sp = [], 1
    for _ in range(n):
        srs.append(b.g1_mul(b.G1_GEN, sp))
        sp = sp * s % b.R
    A = oracle_cpp.gen_scalars(b.SEED_SCALARS, n, start=20 * N)
    from svgpu import encoding as enc
    with svgpu.ResidentBases(enc.bases_array(srs)) as rs:
        C = rs.msm_arrays(A)
        v, pi = rs.open_arrays(A, z)
    a = _ints(A)
    assert v == _horner(a, z)[1]
    assert C == b.g1_mul(b.G1_GEN, _horner(a, s)[1])  # the commitment is p(s) g
    dk = svgpu.KzgDecidingKey(b.G1_GEN, b.G2_GEN, b.g2_mul(b.G2_GEN, s))

    def acc(value):
        lhs = b.g1_add(b.g1_add(C, b.g1_neg(b.g1_mul(b.G1_GEN, value))), b.g1_mul(pi, z))
        return svgpu.KzgAccumulator(lhs, pi)

    svgpu.KzgAs.decide_all(dk, [acc(v)])
    assert svgpu.KzgAs.first_failure(dk, [acc(v)]) == -1
    assert svgpu.KzgAs.first_failure(dk, [acc((v + 1) % b.R)]) == 0
    with pytest.raises(svgpu.AssertionFailure):
        svgpu.KzgAs.decide_all(dk, [acc((v + 1) % b.R)])


def test_four_threads_open_on_one_handle(gpu, case, rset):
    """Calls are re-entrant on one handle: four threads open four different polynomials at once
    (ctypes releases the GIL around every foreign call, so the calls overlap)."""
    jobs = [[(100, 257), (1000, 16385), (3, 1)],
            [(5, 258), (N - 5000, 5001), (0, 2)],
            [(1000, 16385), (100, 257)],
            [(37, 40001), (5, 258)]]
    for k, js in enumerate(jobs):
        for off, n in js:
            case.exp(off, n, k)  # the expected openings first, outside the threads

    def run(k):
        return [rset.open_arrays(case.A[k][:n], Z_GEN, offset=off) == case.exp(off, n, k) for off, n in jobs[k]]

    with ThreadPoolExecutor(max_workers=4) as ex:
        results = list(ex.map(run, range(4)))
    assert all(all(r) for r in results), results
