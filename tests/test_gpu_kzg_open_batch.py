"""Batched KZG opening on a resident base set: the one-pass combination and evaluation
(sv_bn254_fr_poly_combine_eval_device; svgpu.device.poly_combine_eval_device), the opening that
divides the combination and feeds ONE witness MSM (sv_bn254_kzg_open_batch_device;
svgpu.ResidentBases.open_batch_device / open_batch_arrays) and the GWC19 helper over it
(svgpu.gwc19_open).

No expected value comes from the code under test: evaluations, the combination c = sum_j v^j p_j and
the quotient are Python-int arithmetic, the witness is the C++ oracle's Pippenger over the sliced set
and that quotient, and the closing test builds Gwc19::verify's accumulator in oracle group arithmetic
and hands it to the decider.  Everything is arithmetic mod r, so every comparison is bit for bit.

Sizes.  The pass works in spans of kDivSpan coefficients (S, read from csrc/kzg_open.hpp): S - 1, S,
S + 1, 2 S + 1, and lengths that differ inside one batch (a polynomial that ends inside a span, at a
span's end, and whole spans before the longest).  Polynomials are taken one at a time (there is no
chunk of several), so the only other size at which a loop count changes is the fold's:
FOLD_STEP = kDivThreads * S + 1 = 256 S + 1, where the block that folds a polynomial's span totals
takes two per thread (the header says so next to the scratch layout)."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import PKG
from oracle import bn254 as b
from test_gpu_kzg_open import _Open, _dev, _horner, _ints, _limb_bytes, _limbs
from test_gpu_resident_bases import EDGE, N, _UNREDUCED

pytestmark = pytest.mark.gpu

_HPP = open(os.path.join(PKG, "csrc", "kzg_open.hpp")).read()
S = int(re.search(r"constexpr uint32_t kDivSpan = (\d+);", _HPP).group(1))
THREADS = int(re.search(r"constexpr uint32_t kDivThreads = (\d+);", _HPP).group(1))
FOLD_STEP = THREADS * S + 1  # the fold of the span totals goes from one total per thread to two
CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
Z_GEN = b.gen_scalar(b.SEED_SCALARS, 987654321)
V_GEN = b.gen_scalar(b.SEED_SCALARS, 123456789)
ZS = [0, 1, b.R - 1, Z_GEN]
VS = [0, 1, b.R - 1, V_GEN]
KINDS = ["generated", "zero", "first", "last"]
EQUAL_SIZES = [1, 2, 257, S - 1, S, S + 1, 2 * S + 1]
# (offset, N): N - 1 witness terms -- none, one, the last small-route size, the first pipeline size,
# the first GLV size, several blocks behind an odd offset, a slice that ends at the set's end
OPENS = [(3, 1), (0, 2), (100, 257), (5, 258), (1000, 16385), (37, 40001), (N - 5000, 5001)]


def _combine(polys, v):
    """c = sum_j v^j p_j over Python ints, N = the longest length."""
    c = [0] * max(len(a) for a in polys)
    vp = 1
    for a in polys:
        for k, x in enumerate(a):
            c[k] = (c[k] + vp * x) % b.R
        vp = vp * v % b.R
    return c


def _coeffs(oracle_cpp, n, kind, j):
    """Polynomial j of a batch: generated values with the EDGE values spread through them (rotated
    by j), all zero, only the first nonzero, only the last nonzero."""
    if kind == "generated":
        a = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, n, start=(30 + j) * N))
        e = EDGE[j % len(EDGE):] + EDGE[:j % len(EDGE)]
        pos = [i * (n - 1) // (len(e) - 1) for i in range(len(e))] if n > len(e) else range(n)
        for i, x in zip(pos, e):
            a[i] = x
        return a
    a = [0] * n
    if kind == "first":
        a[0] = b.R - 2 - j
    if kind == "last":
        a[n - 1] = b.R - 3 - j
    return a


def _check_combine_eval(polys, gpu, zs=ZS, vs=VS, forms=FORMS):
    from svgpu import device as dv
    n = max(len(a) for a in polys)
    for form in forms:
        A = [_dev(_limbs(a, form), gpu) for a in polys]
        for z in zs:
            evals = [_horner(a, z)[1] for a in polys]
            for v in vs:
                ev, C = dv.poly_combine_eval_device(A, z, v, form=form)
                assert ev == evals, (form, z, v)
                assert tuple(C.shape) == (n, 4)
                assert C.cpu().numpy().tobytes() == _limb_bytes(_combine(polys, v), form), (form, z, v)
                ev_only, none = dv.poly_combine_eval_device(A, z, v, form=form, combined=False)  # d_combined = NULL
                assert none is None and ev_only == evals, (form, z, v)


@pytest.mark.parametrize("n", EQUAL_SIZES)
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_combine_eval_equal_lengths(gpu, oracle_cpp, m, n):
    for kind in KINDS:
        _check_combine_eval([_coeffs(oracle_cpp, n, kind, j) for j in range(m)], gpu)


@pytest.mark.parametrize("order", ["longest first", "longest in the middle", "longest last"])
def test_combine_eval_unequal_lengths(gpu, oracle_cpp, order):
    """A shorter polynomial is zero past its end: inside its last span (1, S + 1, n - 1) and in every
    whole span behind it (1, S, S + 1)."""
    n = 2 * S + 1
    lens = {"longest first": [n, 1, n - 1, S, S + 1],
            "longest in the middle": [1, n - 1, n, S, S + 1],
            "longest last": [S + 1, S, n - 1, 1, n]}[order]
    _check_combine_eval([_coeffs(oracle_cpp, l, "generated", j) for j, l in enumerate(lens)], gpu)


@pytest.mark.parametrize("lens", [[FOLD_STEP, FOLD_STEP], [FOLD_STEP - 1, FOLD_STEP], [FOLD_STEP, S + 1]])
def test_combine_eval_where_the_fold_takes_two_totals_per_thread(gpu, oracle_cpp, lens):
    _check_combine_eval([_coeffs(oracle_cpp, l, "generated", j) for j, l in enumerate(lens)], gpu,
                        zs=[Z_GEN], vs=[V_GEN])


def test_cancelling_combination(gpu, oracle_cpp, rset):
    """m = 2, p_1 = p_0, v = r - 1: c == 0.  The combined rows are all zero, the evaluations are
    still p_0(z), and the opening's witness is the identity."""
    from svgpu import device as dv
    n = 2 * S + 1
    a = _coeffs(oracle_cpp, n, "generated", 0)
    e = _horner(a, Z_GEN)[1]
    for form in FORMS:
        A = _dev(_limbs(a, form), gpu)
        B = _dev(_limbs(a, form), gpu)
        ev, C = dv.poly_combine_eval_device([A, B], Z_GEN, b.R - 1, form=form)
        assert ev == [e, e]
        assert C.cpu().numpy().tobytes() == bytes(32 * n)
        assert rset.open_batch_device([A, B], Z_GEN, b.R - 1, offset=7, form=form) == ([e, e], None)
    # v = 0 with a constant p_0: the quotient is all zero too
    const = [b.R - 5]
    assert rset.open_batch_arrays([_limbs(const, CANONICAL), _limbs(a, CANONICAL)], Z_GEN, 0, offset=7) == ([b.R - 5, e], None)


class _Batch(_Open):
    """The single opening's case (its base set and four coefficient vectors of N + 2 rows) and the
    expected batched opening per (offset, lengths, z, v), computed once and shared."""

    def __init__(self, oracle_cpp):
        super().__init__(oracle_cpp)
        self._bexp = {}

    def polys(self, lens):
        return [self.ints(j % 4)[:l] for j, l in enumerate(lens)]

    def bexp(self, off, lens, z=Z_GEN, v=V_GEN):
        key = (off, tuple(lens), z, v)
        if key not in self._bexp:
            polys = self.polys(lens)
            q, _ = _horner(_combine(polys, v), z)
            self._bexp[key] = ([_horner(a, z)[1] for a in polys], self.witness(off, q))
        return self._bexp[key]

    def tensors(self, lens, form, gpu):
        return [_dev(_limbs(a, form), gpu) for a in self.polys(lens)]


@pytest.fixture(scope="module")
def case(oracle_cpp):
    return _Batch(oracle_cpp)


@pytest.fixture(scope="module")
def rset(gpu, case):
    import svgpu
    with svgpu.ResidentBases(case.B) as s:
        yield s


def _lens3(n):
    """m = 3, unequal, the longest in the middle."""
    return [max(1, n - 3), n, max(1, n // 3)]


@pytest.mark.parametrize("off,n", OPENS)
def test_open_batch_against_the_oracle(gpu, case, rset, off, n):
    from svgpu import device as dv
    lens = _lens3(n)
    exp = case.bexp(off, lens)
    if n == 1:
        assert exp[1] is None  # no quotient term: no MSM
    for form in FORMS:
        assert rset.open_batch_device(case.tensors(lens, form, gpu), Z_GEN, V_GEN, offset=off, form=form) == exp, form
        if n - 1 > 256:  # the witness MSM's figures (the small route zeroes them)
            st = dv.last_msm_stats()
            assert st["entries"] > 0 and st["num_windows"] > 0 and st["accumulate_ms"] > 0
    assert rset.open_batch_arrays([case.A[j % 4][:l] for j, l in enumerate(lens)], Z_GEN, V_GEN, offset=off) == exp
    # m = 1 is the oracle's single opening (v plays no part)
    ev, w = case.exp(off, n)
    assert rset.open_batch_arrays([case.A[0][:n]], Z_GEN, V_GEN, offset=off) == ([ev], w)


def test_the_same_tensor_twice_and_row_slices_of_one_buffer(gpu, case, rset):
    from svgpu import device as dv
    off, n = 5, 2 * S + 1
    a = case.ints(0)[:n]
    A = _dev(_limbs(a, CANONICAL), gpu)
    q, _ = _horner(_combine([a, a, a], V_GEN), Z_GEN)
    e = _horner(a, Z_GEN)[1]
    assert rset.open_batch_device([A, A, A], Z_GEN, V_GEN, offset=off, form=CANONICAL) == ([e] * 3, case.witness(off, q))
    ev, C = dv.poly_combine_eval_device([A, A], Z_GEN, V_GEN, form=CANONICAL)
    assert ev == [e, e] and C.cpu().numpy().tobytes() == _limb_bytes(_combine([a, a], V_GEN), CANONICAL)
    # three polynomials as row slices of one buffer, each from an odd row
    lens = [S + 1, n, 300]
    starts = [1]
    for l in lens[:-1]:
        starts.append((starts[-1] + l + 1) | 1)  # the next odd row with a gap behind the polynomial before
    assert all(s % 2 == 1 for s in starts)
    rows = np.zeros((starts[2] + lens[2] + 3, 4), np.uint64)
    for j, (s, l) in enumerate(zip(starts, lens)):
        rows[s:s + l] = case.A[j][:l]
    buf = _dev(rows, gpu)
    views = [buf[s:s + l] for s, l in zip(starts, lens)]
    assert rset.open_batch_device(views, Z_GEN, V_GEN, offset=off, form=CANONICAL) == case.bexp(off, lens)
    ev, C = dv.poly_combine_eval_device(views, Z_GEN, V_GEN, form=CANONICAL)
    assert ev == case.bexp(off, lens)[0]
    assert C.cpu().numpy().tobytes() == _limb_bytes(_combine(case.polys(lens), V_GEN), CANONICAL)
    assert buf.cpu().numpy().tobytes() == rows.tobytes()  # inputs are only read


def test_combined_over_an_input_is_rejected(gpu, case):
    """Other blocks still read a polynomial while one writes its span of c, so a combination that
    shares a row with an input is an error (and nothing is written); one that ends right before an
    input or starts right behind it is fine.  Inputs in rows [n, 2 n) and [3 n, 3 n + S) of the
    buffer; the combination's n rows from row s."""
    import svgpu
    from svgpu import device as dv
    n = S + 1
    polys = case.polys([n, S])
    rows = np.zeros((5 * n, 4), np.uint64)
    rows[n:2 * n] = _limbs(polys[0], CANONICAL)
    rows[3 * n:3 * n + S] = _limbs(polys[1], CANONICAL)
    buf = _dev(rows, gpu)
    views = [buf[n:2 * n], buf[3 * n:3 * n + S]]
    for s in (1, n, 2 * n - 1, 2 * n + 1, 3 * n, 3 * n + S - 1):
        with pytest.raises(svgpu.ArgumentError, match="overlaps"):
            dv.poly_combine_eval_device(views, Z_GEN, V_GEN, form=CANONICAL, out=buf[s:])
    with pytest.raises(svgpu.LengthError):  # the wrapper refuses a tensor that is too short
        dv.poly_combine_eval_device(views, Z_GEN, V_GEN, form=CANONICAL, out=buf[:n - 1])
    assert buf.cpu().numpy().tobytes() == rows.tobytes()
    evals = [_horner(a, Z_GEN)[1] for a in polys]
    want = _limb_bytes(_combine(polys, V_GEN), CANONICAL)
    for s in (0, 2 * n, 3 * n + S):
        ev, C = dv.poly_combine_eval_device(views, Z_GEN, V_GEN, form=CANONICAL, out=buf[s:])
        assert ev == evals and C.cpu().numpy().tobytes() == want, s
    assert buf[n:2 * n].cpu().numpy().tobytes() == rows[n:2 * n].tobytes()
    assert buf[3 * n:3 * n + S].cpu().numpy().tobytes() == rows[3 * n:3 * n + S].tobytes()


def test_unreduced_coefficients_rejected_and_handle_stays_usable(gpu, case, rset):
    import svgpu
    from svgpu import device as dv
    off, lens = 37, [2 * S + 1, S + 1, 2 * S]
    exp = case.bexp(off, lens)
    for form in FORMS:
        good = [_limbs(a, form) for a in case.polys(lens)]
        G = [_dev(a, gpu) for a in good]
        for j in range(3):
            for idx in (0, S, lens[j] - 1):
                bad = good[j].copy()
                bad[idx] = _UNREDUCED
                polys = G[:j] + [_dev(bad, gpu)] + G[j + 1:]
                with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                    rset.open_batch_device(polys, Z_GEN, V_GEN, offset=off, form=form)
                with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                    dv.poly_combine_eval_device(polys, Z_GEN, V_GEN, form=form)
                with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                    dv.poly_combine_eval_device(polys, Z_GEN, V_GEN, form=form, combined=False)
                # the next valid call on the same handle is exact
                assert rset.open_batch_device(G, Z_GEN, V_GEN, offset=off, form=form) == exp, (form, j, idx)
    with pytest.raises(svgpu.ArgumentError, match="not reduced"):  # v, before any device work
        rset.open_batch_device(G, Z_GEN, b.R, offset=off)


def test_range_of_the_quotient_terms(gpu, case, rset):
    import svgpu
    A = case.A
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_batch_arrays([A[0][:5], A[1][:N + 2]], Z_GEN, V_GEN)          # N + 1 quotient terms
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_batch_arrays([A[0][:5002], A[1][:7]], Z_GEN, V_GEN, offset=N - 5000)
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_batch_arrays([A[0][:1], A[1][:2]], Z_GEN, V_GEN, offset=(1 << 64) - 1)  # no wrap near 2^64
    with pytest.raises(svgpu.ArgumentError, match="reach past"):
        rset.open_batch_arrays([A[0][:1], A[1][:1]], Z_GEN, V_GEN, offset=N + 1)
    v0, v1 = case.ints(0)[0], case.ints(1)[0]
    assert rset.open_batch_arrays([A[0][:1], A[1][:1]], Z_GEN, V_GEN, offset=N) == ([v0, v1], None)  # nothing past the end
    assert rset.open_batch_arrays([A[0][:1], A[1][:2]], Z_GEN, V_GEN, offset=N - 1) == case.bexp(N - 1, [1, 2])
    # the handle is as usable as before
    assert rset.open_batch_arrays([A[j][:l] for j, l in enumerate(_lens3(258))], Z_GEN, V_GEN, offset=5) \
        == case.bexp(5, _lens3(258))


def test_four_threads_open_batches_on_one_handle(gpu, case, rset):
    """Calls are re-entrant on one handle: four threads run different batches at once (ctypes
    releases the GIL around every foreign call, so the calls overlap)."""
    jobs = [[(100, [257, 100, 31]), (1000, [16385, 16000]), (3, [1, 1])],
            [(5, [200, 258]), (N - 5000, [5001, 4000, 1]), (0, [2])],
            [(1000, [16000, 16385]), (100, [31, 257, 100])],
            [(37, [40001, 2 * S + 1]), (5, [258, 200])]]
    for js in jobs:
        for off, lens in js:
            case.bexp(off, lens)  # the expected openings first, outside the threads

    def run(k):
        return [rset.open_batch_arrays([case.A[j % 4][:l] for j, l in enumerate(lens)], Z_GEN, V_GEN, offset=off)
                == case.bexp(off, lens) for off, lens in jobs[k]]

    with ThreadPoolExecutor(max_workers=4) as ex:
        results = list(ex.map(run, range(4)))
    assert all(all(r) for r in results), results


def test_gwc19_commit_open_decide(gpu, oracle_cpp):
    """commit -> gwc19_open -> decide over an SRS s^k g: five polynomials of different lengths, six
    queries over three shifts (polynomial 0 at two of them).  The accumulator is built as
    Gwc19::verify does (gwc19.rs:50-79) in oracle group arithmetic, with the sets grouped here and
    not by the code under test:
      lhs = sum_i u^i sum_j v^j (C_ij - e_ij g) + sum_i u^i z_i W_i,   rhs = sum_i u^i W_i.
    The decider accepts it under (g, g2, s g2); with one evaluation replaced by e + 1 it does not."""
    import svgpu
    from svgpu import encoding as enc
    rows = 300
    s = b.gen_scalar(b.SEED_TRAPDOOR, 1)
    z, v, u = (b.gen_scalar(b.SEED_SCALARS, 515151 + i) for i in range(3))
    w1, w2 = (b.gen_scalar(b.SEED_SCALARS, 616161 + i) for i in range(2))
    srs, sp = [], 1
    for _ in range(rows):
        srs.append(b.g1_mul(b.G1_GEN, sp))
        sp = sp * s % b.R
    lens = [300, 201, 77, 256, 33]
    A = [oracle_cpp.gen_scalars(b.SEED_SCALARS, l, start=(40 + j) * N) for j, l in enumerate(lens)]
    ints = [_ints(a) for a in A]
    queries = [(0, 1), (1, 1), (2, w1), (0, w1), (3, 1), (4, w2)]
    sets = [(1, [0, 1, 4]), (w1, [2, 3]), (w2, [5])]  # (shift, query indices), in order of first appearance
    with svgpu.ResidentBases(enc.bases_array(srs)) as rs:
        C = [rs.msm_arrays(a) for a in A]
        evals, W = svgpu.gwc19_open(rs, [_dev(a, gpu) for a in A], queries, z, v, form=svgpu.SV_CANONICAL)
    assert evals == [_horner(ints[p], shift * z % b.R)[1] for p, shift in queries]
    assert len(W) == len(sets)
    for (shift, members), Wi in zip(sets, W):  # W_i = q_i(s) g for the quotient of set i's combination
        q, _ = _horner(_combine([ints[queries[k][0]] for k in members], v), shift * z % b.R)
        assert Wi == b.g1_mul(b.G1_GEN, _horner(q, s)[1])
    dk = svgpu.KzgDecidingKey(b.G1_GEN, b.G2_GEN, b.g2_mul(b.G2_GEN, s))

    def acc(evs):
        lhs = rhs = None
        up = 1
        for (shift, members), Wi in zip(sets, W):
            f, vp = None, 1
            for k in members:
                term = b.g1_add(C[queries[k][0]], b.g1_neg(b.g1_mul(b.G1_GEN, evs[k])))
                f = b.g1_add(f, b.g1_mul(term, vp))
                vp = vp * v % b.R
            uw = b.g1_mul(Wi, up)
            lhs = b.g1_add(lhs, b.g1_add(b.g1_mul(f, up), b.g1_mul(uw, shift * z % b.R)))
            rhs = b.g1_add(rhs, uw)
            up = up * u % b.R
        return svgpu.KzgAccumulator(lhs, rhs)

    svgpu.KzgAs.decide_all(dk, [acc(evals)])
    assert svgpu.KzgAs.first_failure(dk, [acc(evals)]) == -1
    for k in (0, 3, 5):
        wrong = list(evals)
        wrong[k] = (wrong[k] + 1) % b.R
        assert svgpu.KzgAs.first_failure(dk, [acc(wrong)]) == 0, k
    with pytest.raises(svgpu.AssertionFailure):
        svgpu.KzgAs.decide_all(dk, [acc(wrong)])
