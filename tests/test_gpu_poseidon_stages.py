"""The stages of csrc/poseidon.hip's permutation, one at a time, on words that need not be reduced.

A permutation's input cannot steer the state after the first round, so the known-answer and
random-state tests never put a word near the top of the ranges the lazily reduced schedule allows
(8 x 32-bit rounds: 2.32 r / 2 r / 1.78 r; 29-bit rounds: 12 r / 9 r / 4 r).  Here

  * the stage references (S-box plus constant, dense / pre-sparse / sparse rows) are Python integers
    from oracle.poseidon.optimized_spec, pinned by composing them into a whole permutation
    (test_stage_references_compose_to_the_permutation, no GPU);
  * test_schedule_keeps_every_contract walks the schedule with exact integer upper bounds and the
    real constants of poseidon_consts.hpp and asserts the precondition of every primitive that
    consumes a word (no GPU): a future change of the constants or the schedule that breaks a
    contract fails at once;
  * the GPU tests run each stage through tests/native/poseidoncheck.hip on the edges of its stated
    input range and assert (i) the output is congruent mod r to the reference and (ii) it is below
    the bound the comments in poseidon.hip and the contract of field29.hpp state for that stage.

A word W of the 8 x 32-bit form stands for W / 2^256 mod r, one of the 29-bit form (9 normalized
limbs) for W / 2^261 mod r.  Bounds are exact: "below 2.32 r" is 100 W < 232 r."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from oracle import bn254 as ob
from oracle import poseidon as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "poseidon_consts.hpp")
LIB = os.path.join(ROOT, "tests", "native", "build", "libposeidoncheck.so")

r = ob.R
R32, R29 = 1 << 256, 1 << 261
IR32, IR29 = pow(R32, -1, r), pow(R29, -1, r)

# the stages of poseidoncheck.hip
(PC_POW5, PC_ROW3, PC_FULL3, PC_PARTIAL3, PC_LAST3, PC_ROW5, PC_PARTIAL5, PC_LAST5, PC_CANON,
 PC29_POW5, PC29_ROW, PC29_FULL, PC29_PARTIAL, PC29_OUT, PC29_IN) = range(15)


# ---- stage references on field values (plain integers mod r) ------------------------------------
def sbox(v, c=0):
    return (pow(v, 5, r) + c) % r


def dense_row(row, st):
    return sum(m * v for m, v in zip(row, st)) % r


def full_round(st, consts, mat):
    st = [sbox(v, c) for v, c in zip(st, consts)]
    return [dense_row(row, st) for row in mat]


def partial_round(st, c, sparse):
    row, col_hat = sparse
    s0 = sbox(st[0], c)
    st = [s0] + list(st[1:])
    return [dense_row(row, st)] + [(ch * s0 + v) % r for ch, v in zip(col_hat, st[1:])]


def permutation_by_stages(state, t):
    sp = op.optimized_spec(t, *op.PARAMS[t])
    half = op.PARAMS[t][0] // 2
    st = [(x + c) % r for x, c in zip(state, sp["start"][0])]
    for k in range(1, half):
        st = full_round(st, sp["start"][k], sp["mds"])
    st = full_round(st, sp["start"][half], sp["pre_sparse"])
    for c, sm in zip(sp["partial"], sp["sparse"]):
        st = partial_round(st, c, sm)
    for cs in sp["end"]:
        st = full_round(st, cs, sp["mds"])
    return full_round(st, [0] * t, sp["mds"])


@pytest.mark.parametrize("t", [3, 5])
def test_stage_references_compose_to_the_permutation(t):
    rng = random.Random(900 + t)
    states = [[0] * t, [r - 1] * t] + [[rng.randrange(r) for _ in range(t)] for _ in range(6)]
    for s in states:
        assert permutation_by_stages(s, t) == op.permutation(s, t, *op.PARAMS[t])


def heaviest_partial_round(t):
    """The partial round whose sparse row and column hold the largest constants (their sum)."""
    sparse = op.optimized_spec(t, *op.PARAMS[t])["sparse"]
    return max(range(len(sparse)), key=lambda k: sum(sparse[k][0]) + sum(sparse[k][1]))


# ---- the constants the kernels multiply by ------------------------------------------------------
def _macro(text, name):
    m = re.search(r"#define %s \{([^}]*)\}" % name, text)
    assert m, name
    return [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]


def header_constants(t, r29=False):
    """poseidon_consts.hpp's tables as integers (the Montgomery words c 2^256 mod r, or c 2^261 mod r
    from the 29-bit limbs), shaped like optimized_spec's."""
    text = open(HDR).read()
    bits, per = (29, 9) if r29 else (32, 8)

    def words(key):
        w = _macro(text, "SV_POSEIDON_T%d_%s%s_INIT" % (t, key, "_R29" if r29 else ""))
        assert len(w) % per == 0 and all(x < (1 << bits) for x in w)
        return [sum(x << (bits * i) for i, x in enumerate(w[per * k:per * k + per])) for k in range(len(w) // per)]

    rf, rp = op.PARAMS[t]
    half = rf // 2
    start, partial, end = words("START"), words("PARTIAL"), words("END")
    mds, pre, sparse = words("MDS"), words("PRE"), words("SPARSE")
    assert (len(start), len(partial), len(end)) == ((half + 1) * t, rp, (half - 1) * t)
    assert (len(mds), len(pre), len(sparse)) == (t * t, t * t, rp * (2 * t - 1))
    rows = lambda v, n: [v[n * k:n * k + n] for k in range(len(v) // n)]  # noqa: E731
    return {"start": rows(start, t), "partial": partial, "end": rows(end, t), "mds": rows(mds, t),
            "pre_sparse": rows(pre, t),
            "sparse": [(v[:t], v[t:]) for v in rows(sparse, 2 * t - 1)]}


@pytest.mark.parametrize("t,r29", [(3, False), (5, False), (3, True)])
def test_header_constants_are_the_references(t, r29):
    """The words the kernels multiply by are optimized_spec's constants in Montgomery form, so the
    stage references and the bound walk below speak about the same numbers."""
    f = R29 if r29 else R32
    hc, sp = header_constants(t, r29), op.optimized_spec(t, *op.PARAMS[t])
    mont = lambda v: [x * f % r for x in v]  # noqa: E731
    for key in ("start", "end", "mds", "pre_sparse"):
        assert hc[key] == [mont(row) for row in sp[key]], key
    assert hc["partial"] == mont(sp["partial"])
    assert hc["sparse"] == [(mont(row), mont(col)) for row, col in sp["sparse"]]


# ---- B4: the schedule with exact integer upper bounds -------------------------------------------
# Every function takes and returns INCLUSIVE maxima.  A Montgomery product sum of words a_i with
# constants (or words) b_i is (sum a_i b_i + m r) / F with m < F, so it is at most
# floor((sum max_i b_i + (F - 1) r) / F) (below floor(sum bound_i b_i / F) + r).
def _mont_max(pairs, f):
    return (sum(a * b for a, b in pairs) + (f - 1) * r) // f


def _wrap_max(m, k):
    """One conditional subtraction of k r from a word of at most m."""
    return m if m < k * r else max(k * r - 1, m - k * r)


def _below(m, num, den=1):
    return m * den < num * r


class Walk32:
    """permute<T> of poseidon.hip over field.hpp's lazily reduced words."""

    def __init__(self, t):
        self.t, self.c = t, header_constants(t)
        self.peak = 0  # the largest state word met

    def product(self, pairs):
        m = _mont_max(pairs, R32)
        assert m < R32, "a lazy product must stay below 2^256"
        return m

    def pow5(self, x):
        assert x < R32
        x2 = self.product([(x, x)])
        return self.product([(self.product([(x2, x2)]), x)])

    def add2p(self, a, b):  # fe_add2p: no carry out of 256 bits, wraps at 2 r
        assert a + b < R32
        return _wrap_max(a + b, 2)

    def row(self, st, consts, lazy):
        t = self.t
        if t == 3:
            m = self.product(list(zip(st, consts)))
            return m if lazy else _wrap_max(m, 1)  # fe_mul_sum<3, kReduce>: one subtraction of r
        # t = 5: fe_mul_sum of three products + fe_mul_sum of two, each reduced once, then operator+
        a = _wrap_max(self.product(list(zip(st[:3], consts[:3]))), 1)
        b = _wrap_max(self.product(list(zip(st[3:], consts[3:]))), 1)
        assert a + b < R32
        return _wrap_max(a + b, 1)

    def full(self, st, consts, mat, lazy):
        st = [self.add2p(self.pow5(x), c) if consts else self.pow5(x) for x, c in zip(st, consts or [0] * self.t)]
        return [self.row(st, rowc, lazy) for rowc in mat]

    def see(self, st):
        self.peak = max(self.peak, *st)
        # the comment above pow5: t = 3 words stay below 2.32 r, t = 5 words below 2 r
        for x in st:
            assert _below(x, 232, 100) if self.t == 3 else _below(x, 2), x / r
        return st

    def run(self):
        t, c = self.t, self.c
        half = op.PARAMS[t][0] // 2
        lazy = t == 3
        st = [_wrap_max((r - 1) + k, 1) for k in c["start"][0]]  # reduced inputs, operator+
        self.see(st)
        for k in range(1, half):
            st = self.see(self.full(st, c["start"][k], c["mds"], lazy))
        st = self.see(self.full(st, c["start"][half], c["pre_sparse"], lazy))
        for k, (row, col) in zip(c["partial"], c["sparse"]):
            s0 = self.add2p(self.pow5(st[0]), k)
            assert _below(s0, 2)
            rest = [self.add2p(x, self.product([(s0, ch)])) for x, ch in zip(st[1:], col)]
            st = self.see([self.row([s0] + st[1:], row, lazy)] + rest)
        for cs in c["end"]:
            st = self.see(self.full(st, cs, c["mds"], lazy))
        st = self.full(st, None, c["mds"], False)
        for x in st:
            assert _below(x, 2), "fe_canon2p takes words below 2 r"
            if t == 3:
                assert _below(x, 132, 100)  # "rows reduced once: below 1.32 r"
        return st


class Walk29:
    """p29::permute over field29.hpp's words: mul / sqr take words below 12 r, mul_sum3 words below
    9 r with constants below r, csub<4> words below 8 r, to_r32 words below 4 r."""

    def __init__(self):
        self.c = header_constants(3, True)

    def mul(self, a, b):
        assert _below(a, 12) and _below(b, 12)
        m = _mont_max([(a, b)], R29)
        assert _below(m, 2)  # the contract's output bound
        return m

    def pow5(self, x):
        x2 = self.mul(x, x)
        return self.mul(self.mul(x2, x2), x)

    def add(self, a, b):
        assert a + b < R29
        return a + b

    def row(self, st, consts):
        assert all(_below(x, 9) for x in st) and all(k < r for k in consts)
        m = _mont_max(list(zip(st, consts)), R29)
        assert _below(m, 2)
        return m

    def full(self, st, consts, mat):
        st = [self.add(self.pow5(x), k) if consts else self.pow5(x) for x, k in zip(st, consts or [0] * 3)]
        assert all(_below(x, 3) for x in st)  # "+ constant makes it below 3 r"
        return [self.row(st, rowc) for rowc in mat]

    def run(self):
        c = self.c
        st = [self.add(2 * r - 1, k) for k in c["start"][0]]  # to_r29 leaves words below 2 r
        for k in range(1, 4):
            st = self.full(st, c["start"][k], c["mds"])
        st = self.full(st, c["start"][4], c["pre_sparse"])
        for k, (row, col) in zip(c["partial"], c["sparse"]):
            a = self.add(self.pow5(st[0]), k)
            rest = []
            for x, ch in zip(st[1:], col):
                assert _below(x, 4)
                s = self.add(x, self.mul(a, ch))
                assert _below(s, 8), "csub<4> takes words below 8 r"
                rest.append(_wrap_max(s, 4))
            st = [self.row([a] + st[1:], row)] + rest
        for cs in c["end"]:
            st = self.full(st, cs, c["mds"])
        st = self.full(st, None, c["mds"])
        assert all(_below(x, 4) for x in st), "to_r32 takes words below 4 r"
        return st


def test_schedule_keeps_every_contract():
    w3 = Walk32(3)
    w3.run()
    w5 = Walk32(5)
    w5.run()
    Walk29().run()
    # t = 5 feeds fe_mul_sum<., 3, true> + fe_mul_sum<., 2, true> words below 2 r: for constants
    # anywhere below r a row may leave in [r, 1.14 r) (the three-product sum scans up to 2.14 r and
    # loses r once) ...
    top = w5.row([2 * r - 1] * 5, [r - 1] * 5, False)
    assert r <= top and _below(top, 114, 100)
    # ... but no row of the real tables has constants that large (it takes c_0 + c_1 + c_2 above
    # 2^255), so with them every row leaves below r
    c5 = w5.c
    for rowc in c5["mds"] + c5["pre_sparse"] + [s[0] for s in c5["sparse"]]:
        assert w5.row([2 * r - 1] * 5, rowc, False) < r and sum(rowc[:3]) < 1 << 255


# ---- the GPU stages -----------------------------------------------------------------------------
_lib = None


def _pc():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(LIB)
        _lib.pc_stage.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        _lib.pc_words.argtypes = [ctypes.c_int, ctypes.c_int]
    return _lib


def _run(stage, sel, cases, in29, out29):
    """cases: lists of input words (integers) -> lists of output words; limbs are raw both ways."""
    lib = _pc()
    ib, ipw = (29, 9) if in29 else (32, 8)
    obits, opw = (29, 9) if out29 else (32, 8)
    nin, nout = lib.pc_words(stage, 0) // ipw, lib.pc_words(stage, 1) // opw
    assert all(len(c) == nin for c in cases)
    a = np.array([[(w >> (ib * i)) & ((1 << ib) - 1) for w in c for i in range(ipw)] for c in cases], np.uint32)
    assert all(w >> (ib * ipw) == 0 for c in cases for w in c)
    out = np.full((len(cases), nout * opw), 0xffffffff, np.uint32)
    assert lib.pc_stage(stage, sel, a.ctypes.data, out.ctypes.data, len(cases)) == 0
    if out29:
        assert int(out.max()) < (1 << 29), "29-bit limbs must leave normalized"
    return [[sum(int(x) << (obits * i) for i, x in enumerate(row[opw * k:opw * k + opw])) for k in range(nout)]
            for row in out]


def _top(num, den=1):
    """The largest word below num / den r."""
    return (num * r - 1) // den


def _cases(tops, bits, seed):
    """Input tuples for words with inclusive maxima `tops`: 0, 1, r - 1, r, r + 1, 2 r - 1, 2 r, the
    top of the range and the word below it, words whose low limbs are all ones -- each on every word
    alone (the others random) and on all words together -- and 48 random tuples."""
    rng = random.Random(seed)
    ones = []
    for k in (1, 4, 7):
        ones += [(1 << (bits * k)) - 1, "low%d" % k]
    special = [0, 1, r - 1, r, r + 1, 2 * r - 1, 2 * r, "top", "top-1"] + ones

    def word(sp, top):
        if sp == "top":
            return top
        if sp == "top-1":
            return top - 1
        if isinstance(sp, str):  # the top of the range with its low limbs turned to ones
            sh = bits * int(sp[3:])
            return (((top >> sh) - 1) << sh) | ((1 << sh) - 1)
        return min(sp, top)

    rnd = lambda: [rng.randrange(t + 1) for t in tops]  # noqa: E731
    out = []
    for sp in special:
        out.append([word(sp, t) for t in tops])
        if len(tops) > 1:
            for i in range(len(tops)):
                c = rnd()
                c[i] = word(sp, tops[i])
                out.append(c)
    out += [rnd() for _ in range(48)]
    assert all(0 <= w <= t for c in out for w, t in zip(c, tops))
    return out


gpu_only = pytest.mark.gpu


def _sp(t):
    return op.optimized_spec(t, *op.PARAMS[t])


def _rows_sel(t):
    """(sel, reference row) for every dense and pre-sparse row and three sparse rows."""
    sp = _sp(t)
    rp = op.PARAMS[t][1]
    sels = [(0 | i << 8, sp["mds"][i]) for i in range(t)] + [(1 | i << 8, sp["pre_sparse"][i]) for i in range(t)]
    return sels + [(2 | k << 8, sp["sparse"][k][0]) for k in sorted({0, rp - 1, heaviest_partial_round(t)})]


def _partial_rounds(t):
    return sorted({0, op.PARAMS[t][1] - 1, heaviest_partial_round(t)})


def _full_sel(t):
    """(sel, constants, matrix) for every full round with constants."""
    sp = _sp(t)
    half = op.PARAMS[t][0] // 2
    return ([(0 | k << 8, sp["start"][k], sp["mds"]) for k in range(1, half)] +
            [(1, sp["start"][half], sp["pre_sparse"])] +
            [(2 | k << 8, sp["end"][k], sp["mds"]) for k in range(half - 1)])


def _val(w, inv):
    return w * inv % r


@gpu_only
def test_pow5_32(gpu):
    """pow5 of a word below 2.32 r is x^5 and below 1.78 r."""
    cases = _cases([_top(232, 100)], 32, 1)
    for (x,), (y,) in zip(cases, _run(PC_POW5, 0, cases, False, False)):
        assert _val(y, IR32) == sbox(_val(x, IR32)), hex(x)
        assert _below(y, 178, 100), (hex(x), y / r)


@gpu_only
def test_mds_row3_lazy(gpu):
    """A t = 3 row of words below 2.32 r is kept as scanned: the row's value, below 2.316 r."""
    for sel, row in _rows_sel(3):
        cases = _cases([_top(232, 100)] * 3, 32, 100 + sel)
        for c, (y,) in zip(cases, _run(PC_ROW3, sel, cases, False, False)):
            assert _val(y, IR32) == dense_row(row, [_val(x, IR32) for x in c]), (sel, [hex(x) for x in c])
            assert _below(y, 2316, 1000), (sel, y / r)


@gpu_only
def test_full_round3(gpu):
    """full_round<3> of words below 2.32 r: the round's value, every word below 2.316 r."""
    for sel, consts, mat in _full_sel(3):
        cases = _cases([_top(232, 100)] * 3, 32, 200 + sel)
        for c, out in zip(cases, _run(PC_FULL3, sel, cases, False, False)):
            assert [_val(y, IR32) for y in out] == full_round([_val(x, IR32) for x in c], consts, mat), sel
            assert all(_below(y, 2316, 1000) for y in out), (sel, [y / r for y in out])


@gpu_only
def test_partial_round3(gpu):
    """One t = 3 partial round of words below 2.32 r: state[0] leaves below 2.316 r, state[i]
    never grows past max(2 r, what it was)."""
    sp = _sp(3)
    for k in _partial_rounds(3):
        cases = _cases([_top(232, 100)] * 3, 32, 300 + k)
        for c, out in zip(cases, _run(PC_PARTIAL3, k, cases, False, False)):
            want = partial_round([_val(x, IR32) for x in c], sp["partial"][k], sp["sparse"][k])
            assert [_val(y, IR32) for y in out] == want, (k, [hex(x) for x in c])
            assert _below(out[0], 2316, 1000), (k, out[0] / r)
            assert all(y < max(2 * r, x) for x, y in zip(c[1:], out[1:])), (k, [y / r for y in out])


@gpu_only
def test_last_round3(gpu):
    """The last full round reduces its rows once (below 1.32 r) and fe_canon2p makes them canonical."""
    mat = _sp(3)["mds"]
    cases = _cases([_top(232, 100)] * 3, 32, 400)
    for c, out in zip(cases, _run(PC_LAST3, 0, cases, False, False)):
        want = full_round([_val(x, IR32) for x in c], [0] * 3, mat)
        assert [_val(y, IR32) for y in out[:3]] == want
        assert all(_below(y, 132, 100) for y in out[:3]), [y / r for y in out[:3]]
        assert out[3:] == [w * R32 % r for w in want]           # canonical: the one word below r


@gpu_only
def test_width5_rows_and_partial_round(gpu):
    """t = 5 keeps fe_mul_sum's subtraction: a row of words below 2 r leaves below 1.14 r (for
    constants anywhere below r it could be in [r, 1.14 r); test_schedule_keeps_every_contract shows
    that the real tables keep it below r), a partial round keeps state[i] below 2 r."""
    sp = _sp(5)
    tops = [_top(2)] * 5
    for sel, row in _rows_sel(5):
        cases = _cases(tops, 32, 500 + sel)
        for c, (y,) in zip(cases, _run(PC_ROW5, sel, cases, False, False)):
            assert _val(y, IR32) == dense_row(row, [_val(x, IR32) for x in c]), (sel, [hex(x) for x in c])
            assert _below(y, 114, 100), (sel, y / r)
    for k in _partial_rounds(5):
        cases = _cases(tops, 32, 600 + k)
        for c, out in zip(cases, _run(PC_PARTIAL5, k, cases, False, False)):
            want = partial_round([_val(x, IR32) for x in c], sp["partial"][k], sp["sparse"][k])
            assert [_val(y, IR32) for y in out] == want, (k, [hex(x) for x in c])
            assert _below(out[0], 114, 100) and all(_below(y, 2) for y in out[1:]), (k, [y / r for y in out])


@gpu_only
def test_width5_last_round_and_canon(gpu):
    """The end of permute<5>: the last round's rows (below 1.14 r) and fe_canon2p on them, and
    fe_canon2p alone on every kind of word below 2 r, [r, 1.14 r) included."""
    mat = _sp(5)["mds"]
    cases = _cases([_top(2)] * 5, 32, 700)
    for c, out in zip(cases, _run(PC_LAST5, 0, cases, False, False)):
        want = full_round([_val(x, IR32) for x in c], [0] * 5, mat)
        assert [_val(y, IR32) for y in out[:5]] == want
        assert all(_below(y, 114, 100) for y in out[:5]), [y / r for y in out[:5]]
        assert out[5:] == [w * R32 % r for w in want]
    words = _cases([_top(2)], 32, 701) + [[w] for w in (_top(114, 100), _top(114, 100) - 1, r + (1 << 224) - 1)]
    for (x,), (y,) in zip(words, _run(PC_CANON, 0, words, False, False)):
        assert y == x % r, hex(x)


@gpu_only
def test_pow5_29(gpu):
    """p29::pow5 of a word below 12 r is x^5 and below 2 r."""
    cases = _cases([_top(12)], 29, 800)
    for (x,), (y,) in zip(cases, _run(PC29_POW5, 0, cases, True, True)):
        assert _val(y, IR29) == sbox(_val(x, IR29)), hex(x)
        assert _below(y, 2), (hex(x), y / r)


@gpu_only
def test_row_29(gpu):
    """p29::row of words below 9 r: the row's value, below 2 r."""
    for sel, row in _rows_sel(3):
        cases = _cases([_top(9)] * 3, 29, 900 + sel)
        for c, (y,) in zip(cases, _run(PC29_ROW, sel, cases, True, True)):
            assert _val(y, IR29) == dense_row(row, [_val(x, IR29) for x in c]), (sel, [hex(x) for x in c])
            assert _below(y, 2), (sel, y / r)


@gpu_only
def test_full_round_29(gpu):
    """p29::full of words below 12 r: the round's value, every word below 2 r."""
    for sel, consts, mat in _full_sel(3):
        cases = _cases([_top(12)] * 3, 29, 1000 + sel)
        for c, out in zip(cases, _run(PC29_FULL, sel, cases, True, True)):
            assert [_val(y, IR29) for y in out] == full_round([_val(x, IR29) for x in c], consts, mat), sel
            assert all(_below(y, 2) for y in out), (sel, [y / r for y in out])


@gpu_only
def test_partial_round_29(gpu):
    """One partial round of p29::permute: state[0] below 12 r and state[1..] below 4 r in, state[0]
    below 2 r and state[1..] back below 4 r (csub<4>) out."""
    sp = _sp(3)
    for k in _partial_rounds(3):
        cases = _cases([_top(12), _top(4), _top(4)], 29, 1100 + k)
        for c, out in zip(cases, _run(PC29_PARTIAL, k, cases, True, True)):
            want = partial_round([_val(x, IR29) for x in c], sp["partial"][k], sp["sparse"][k])
            assert [_val(y, IR29) for y in out] == want, (k, [hex(x) for x in c])
            assert _below(out[0], 2) and all(_below(y, 4) for y in out[1:]), (k, [y / r for y in out])


@gpu_only
def test_form_changes_29(gpu):
    """to_r32 on the way out: a 29-bit word below 4 r becomes the canonical 8 x 32-bit word of the
    same value; to_r29 on the way in: a reduced word becomes a 29-bit word below 2 r."""
    cases = _cases([_top(4)], 29, 1200)
    for (x,), (y,) in zip(cases, _run(PC29_OUT, 0, cases, True, False)):
        assert y == _val(x, IR29) * R32 % r, hex(x)
    cases = _cases([r - 1], 32, 1201)
    for (x,), (y,) in zip(cases, _run(PC29_IN, 0, cases, False, True)):
        assert _val(y, IR29) == _val(x, IR32) and _below(y, 2), hex(x)
