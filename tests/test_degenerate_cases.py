"""The degenerate-addition cases (tests/degenerate_cases.py) proved on the CPU: a multiplier-level
model of every reduction the GPU tests send them through, in Python integers.

A bucket's value is the integer multiple of P it holds (a random row counts as a 200-bit integer of
its own, so sums of random rows never coincide), read back from the case's own arrays: the scalars
through a plain restatement of the signed-digit rule, the bases through the lattice table.  The
model then performs the additions of the reduction and files every operand pair (a, b) under its
level and one of five classes:

  same       a == b != 0       the doubling branch
  neg        a == -b != 0      the identity comes out
  one_zero   exactly one operand is the identity
  both_zero  both are
  generic    everything else

A case passes when every level it claims holds at least one pair of every claimed class: the GPU
test cannot pass without meeting its case.  The counts are a property of the inputs (the sums
commute); where a kernel pairs operands in a particular order the pairing is taken from its code:

  running sums           k_wsum / k_wsum_tree<true>, msm.hip: `run = add(run, cur)`, `acc = add(acc, run)`
  in-block tree          k_wsum_tree level 0 ("level 0 (lane pairs ...)": A[2i] + A[2i+1], T[2i] + T[2i+1])
                         and tr_task ("task tau of tree level l ..."): slots dst and dst + 2^l of rows A, T
  k_group_fin            "U_k, k >= 8: the totals of the blocks with bit k - 8 set"; a quad adds its four
                         members as (0 + 1) + (2 + 3), then lanes + 32 .. + 4, then wave 1 into wave 0
  k_group_sum(_q)        group_member's bit interleave ("member m of group q of window w"), members strided
                         by 512 per thread, slices [H pp / P, H (pp + 1) / P), the LDS / shuffle tree
  host_combine           one chain over every exponent: A_lo, A_hi at c w, U_k at c w + logL + k
  batch                  the Hillis-Steele suffix scan and the tree over 16 (or 128) buckets, the window
                         Horner, horner_msm's bucket-wise Horner, k_batch_uwin's member(j), member(j + 4)

Not marked gpu: runs anywhere."""
import hashlib
from collections import Counter, defaultdict

import numpy as np
import pytest

import degenerate_cases as dc
from oracle import bn254 as b

R = b.R
SAME, NEG, ONE, BOTH, GEN = "same", "neg", "one_zero", "both_zero", "generic"


def classify(a, c):
    if a == 0 and c == 0:
        return BOTH
    if a == 0 or c == 0:
        return ONE
    if a == c:
        return SAME
    if a == -c:
        return NEG
    return GEN


class Tally:
    def __init__(self):
        self.n = defaultdict(Counter)

    def add(self, level, a, c):
        self.n[level][classify(a, c)] += 1
        return a + c

    def require(self, claims, what):
        for level, classes in claims.items():
            for cl in classes:
                assert self.n[level][cl] > 0, (what, level, cl, dict(self.n[level]))


def pseudo(row):
    """A random row's stand-in multiplier: 200 bits of its hash."""
    return int.from_bytes(hashlib.sha256(np.ascontiguousarray(row).tobytes()).digest()[:25], "little") | 1 << 199


def signed_digits(s, c, nwin):
    """for_each_digit (msm.hip): window values above 2^(c-1) become negative digits with a carry.
    Returns ([digit per window], whether any window carried)."""
    out, carry, carried = [], 0, False
    for w in range(nwin):
        bits = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        if bits > 1 << (c - 1):
            out.append(bits - (1 << c))
            carry, carried = 1, True
        else:
            out.append(bits)
            carry = 0
    assert carry == 0
    return out, carried


def bucket_table(bases, scalars, c, nwin, lat, allow_carry=False):
    """X[w][b], present[w][b] and the entries of every bucket, from the arrays alone."""
    nb = 1 << (c - 1)
    X = [[0] * nb for _ in range(nwin)]
    ent = [[[] for _ in range(nb)] for _ in range(nwin)]
    mult = {}
    for row, s in zip(bases, dc.limbs_to_ints(scalars)):
        if s == 0:
            continue
        key = row.tobytes()
        m = mult.get(key)
        if m is None:
            m = lat.mult_of(row)
            m = mult[key] = pseudo(row) if m is None else m
        if m == 0:
            continue  # the identity base: skipped by every kernel
        digits, carried = signed_digits(s, c, nwin)
        assert allow_carry or not carried, hex(s)
        for w, d in enumerate(digits):
            if d:
                v = m if d > 0 else -m
                X[w][abs(d) - 1] += v
                ent[w][abs(d) - 1].append(v)
    return X, ent


def value_of(X, c):
    return sum((bk + 1) * v << (c * w) for w, row in enumerate(X) for bk, v in enumerate(row) if v)


# ---- the single-MSM reduction --------------------------------------------------------------------
def running_sums(x, present, L, T):
    J = len(x) // L
    acc, tot = [0] * J, [0] * J
    for j in range(J):
        run = a = 0
        for i in range(j * L + L - 1, j * L - 1, -1):
            if present[i]:
                run = T.add("run+cur", run, x[i])
            a = T.add("acc+run", a, run)
        acc[j], tot[j] = a, run
    return acc, tot


def tree_block(acc, tot, T):
    """One block of k_wsum_tree over 256 segments (acc None: the tree straight over the buckets) ->
    [A,] CT, U_0 .. U_7."""
    run = acc is not None
    rowT, rowA = list(tot), list(acc) if run else None
    for i in range(128):
        if run:
            rowA[2 * i] = T.add("tree.l0", acc[2 * i], acc[2 * i + 1])
        rowT[2 * i] = T.add("tree.l0", tot[2 * i], tot[2 * i + 1])
    for l in range(1, 8):
        s, npair = 1 << l, 256 >> (l + 1)
        for tau in range(((2 if run else 1) + l) * npair):
            if run and tau < npair:
                row, dst = rowA, 2 * tau * s
            else:
                r = tau - npair if run else tau
                kk, i = divmod(r, npair)
                row, dst = rowT, 2 * i * s + ((1 << (kk - 1)) if kk else 0)
            row[dst] = T.add("tree.l%d" % l, row[dst], row[dst + s])
    return ([rowA[0]] if run else [None]) + [rowT[0]] + [rowT[1 << k] for k in range(8)]


def group_fin(blocks, NG, aslot, T):
    """k_group_fin over one window's per-block outputs -> the NG group sums."""
    bpw = len(blocks)
    out = []
    for q in range(NG):
        if q < 2:
            h = (bpw + 1) // 2
            members = h if q == 0 else bpw - h
            pick = lambda t: blocks[(0 if q == 0 else h) + t][aslot]
        elif q - 2 < 8:
            members = bpw
            pick = lambda t: blocks[t][q]
        else:
            m = q - 2 - 8
            members = bpw // 2
            pick = lambda t: blocks[((t >> m) << (m + 1)) | (1 << m) | (t & ((1 << m) - 1))][1]
        sums = []
        for wv in range(2):
            if wv > 0 and wv * 64 >= members:
                continue
            v = [pick(t) if t < members else 0 for t in range(wv * 64, wv * 64 + 64)]
            s = [T.add("fin.q1", T.add("fin.q0", v[4 * i], v[4 * i + 1]), T.add("fin.q0", v[4 * i + 2], v[4 * i + 3]))
                 for i in range(16)]
            live = (min(64, members - wv * 64) + 3) // 4 * 4
            for off in (32, 16, 8, 4):
                if off >= live:
                    continue
                for i in range(off // 4):
                    s[i] = T.add("fin.w%d" % off, s[i], s[i + off // 4])
            sums.append(s[0])
        out.append(T.add("fin.wave1", sums[0], sums[1]) if members > 64 else sums[0])
    return out


def group_sum(acc, tot, P, quad, T):
    """k_group_sum / k_group_sum_q over one window's running sums -> the NG group sums.  The block
    that folds part[] is the one that finishes last; the model takes slice P - 1."""
    J = len(acc)
    logJ, H = J.bit_length() - 1, J // 2
    out = []
    for q in range(2 + logJ):
        if q < 2:
            mem = lambda m: acc[q * H + m]
        else:
            k = q - 2
            mem = lambda m: tot[((m >> k) << (k + 1)) | (1 << k) | (m & ((1 << k) - 1))]
        part = []
        for pp in range(P):
            m0, m1 = H * pp // P, H * (pp + 1) // P
            s = [0] * 512
            for t in range(512):
                m = m0 + t
                while m + 512 < m1:
                    s[t] = T.add("gs.serial", T.add("gs.serial", s[t], mem(m)), mem(m + 512))
                    m += 1024
                if m < m1:
                    s[t] = T.add("gs.serial", s[t], mem(m))
            if quad:
                w8 = []
                for wv in range(8):
                    v = s[64 * wv: 64 * wv + 64]
                    z = [T.add("gs.q1", T.add("gs.q0", v[4 * i], v[4 * i + 1]), T.add("gs.q0", v[4 * i + 2], v[4 * i + 3]))
                         for i in range(16)]
                    for off in (32, 16, 8, 4):
                        for i in range(off // 4):
                            z[i] = T.add("gs.w%d" % off, z[i], z[i + off // 4])
                    w8.append(z[0])
                for off in (16, 8, 4):
                    for i in range(off // 4):
                        w8[i] = T.add("gs.x%d" % off, w8[i], w8[i + off // 4])
                part.append(w8[0])
            else:
                for st in (256, 128, 64):
                    for t in range(st):
                        s[t] = T.add("gs.lds%d" % st, s[t], s[t + st])
                for off in (32, 16, 8, 4, 2, 1):
                    for t in range(off):
                        s[t] = T.add("gs.w%d" % off, s[t], s[t + off])
                part.append(s[0])
        s = part[P - 1]
        for k in range(P - 1):
            s = T.add("gs.part", s, part[k])
        out.append(s)
    return out


def host_combine(A, c, logL, logJ, T):
    acc = 0
    for e in range((len(A) - 1) * c + logL + logJ - 1, -1, -1):
        acc *= 2
        w, r = divmod(e, c)
        if r == 0:
            acc = T.add("combine", T.add("combine", acc, A[w][0]), A[w][1])
        if r >= logL and r - logL < logJ:
            acc = T.add("combine", acc, A[w][2 + r - logL])
    return acc


def model_single(case, glv, tree, P=1, quad=True, all_present=False):
    """The whole single-MSM reduction of a case -> (tally, the multiplier that comes out, tables)."""
    c, logL = case.c, (0 if tree == 2 else case.red_log)
    W = -(-(128 if glv else 255) // c)
    lat = dc.lattice()
    X, ent = bucket_table(case.bases, case.scalars, c, W, lat)
    T = Tally()
    J = (1 << (c - 1)) >> logL
    logJ = J.bit_length() - 1
    A = []
    for w in range(W):
        present = [all_present or bool(e) for e in ent[w]]
        if tree == 2:
            blocks = [tree_block(None, [x if p else 0 for x, p in zip(X[w][k:k + 256], present[k:k + 256])], T)
                      for k in range(0, J, 256)]
            A.append(group_fin(blocks, 2 + logJ, 1, T))
            continue
        acc, tot = running_sums(X[w], present, 1 << logL, T)
        if tree == 1:
            blocks = [tree_block(acc[k:k + 256], tot[k:k + 256], T) for k in range(0, J, 256)]
            A.append(group_fin(blocks, 2 + logJ, 0, T))
        else:
            A.append(group_sum(acc, tot, P, quad, T))
    got = host_combine(A, c, logL, logJ, T)
    assert got == value_of(X, c), "the model does not add up"
    return T, got, (X, ent)


@pytest.fixture(scope="module")
def rand_rows(oracle_cpp):
    return oracle_cpp.gen_bases(b.SEED_BASES, 1 << 12, start=424242)


def check_inputs(case, oracle_cpp):
    """Scalars below 2^125 (so the GLV split leaves them alone), no base off the table in a pure
    case, and the closed form equal to the oracle's Pippenger."""
    ints = dc.limbs_to_ints(case.scalars)
    top = max(ints)
    assert top < dc.SCALAR_BOUND < 1 << 126
    assert dc.glv_coefficients(top) == (0, 0) and dc.glv_coefficients(dc.SCALAR_BOUND - 1) == (0, 0)
    want = b.g1_from_bytes(oracle_cpp.msm_pippenger(case.bases, case.scalars, 0).tobytes())
    if case.pure:
        assert dc.expected_point(case) == want


def test_glv_bound_is_tight():
    """Below 2^125 the Babai coefficients are 0; just under 2^126 the second one is 1, so the issue's
    2^126 would not do."""
    assert dc.glv_coefficients((1 << 125) - 1) == (0, 0)
    assert dc.glv_coefficients((1 << 126) - 1) == (0, 1)


LEVELS = ["tree.l%d" % l for l in range(8)]


@pytest.mark.parametrize("glv,c,red_log", [(1, 11, 2), (0, 12, 3)])
def test_levels_case_on_the_default_tree(oracle_cpp, glv, c, red_log):
    case = dc.case_levels(c, red_log)
    check_inputs(case, oracle_cpp)
    T, got, _ = model_single(case, glv, tree=1)
    assert got % R == case.sum_mult
    claims = {lv: {SAME, NEG} for lv in LEVELS}
    claims.update({"run+cur": {SAME}, "acc+run": {SAME}})
    T.require(claims, case.name)


@pytest.mark.parametrize("glv", [0, 1])
def test_levels_case_on_the_pure_tree(oracle_cpp, glv):
    case = dc.case_levels(9, 0)
    check_inputs(case, oracle_cpp)
    T, got, _ = model_single(case, glv, tree=2)
    assert got % R == case.sum_mult
    T.require({lv: {SAME, NEG} for lv in LEVELS}, case.name)
    assert not T.n["run+cur"]


@pytest.mark.parametrize("glv,c,red_log,tree", [(1, 11, 2, 1), (0, 12, 3, 1), (1, 9, 0, 2), (0, 9, 0, 2)])
def test_mixed_case(oracle_cpp, rand_rows, glv, c, red_log, tree):
    case = dc.case_mixed(c, red_log, rand_rows)
    assert not case.pure
    check_inputs(case, oracle_cpp)
    T, _, (X, ent) = model_single(case, glv, tree)
    win = {name: w for w, name in case.patterns.items()}
    claims = {"combine": {SAME, NEG}, "tree.l0": {SAME, NEG, GEN}}
    L = 1 << (0 if tree == 2 else red_log)
    if tree == 1:
        # the stored cancelled record (P and -P in one bucket) is read as a bucket that is not empty
        w = win["segment_cancel"]
        assert any(len(e) == 2 and x == 0 for e, x in zip(ent[w], X[w]))
        claims.update({"run+cur": {NEG, ONE, BOTH}, "acc+run": {NEG}})
        T1 = Tally()
        running_sums(X[w], [bool(e) for e in ent[w]], L, T1)
        T1.require({"run+cur": {NEG}, "acc+run": {NEG}}, "segment_cancel alone")
    T.require(claims, case.name)
    # one wave (64 consecutive segments) of each mixed window holds a degenerate pair beside a generic
    # one: level 0 is the only level that pairs two lattice segments (4i, 4i + 1)
    for name, cls in (("mixed", SAME), ("mixed_cancel(0)", NEG)):
        w = win[name]
        tot = [sum(X[w][j * L:(j + 1) * L]) for j in range(64)]
        pairs = Counter(classify(tot[2 * i], tot[2 * i + 1]) for i in range(32))
        assert pairs[GEN] > 0 and pairs[cls] > 0, (name, pairs)
    # a window whose every record is a stored identity, beside one that is really empty
    w = win["empty_but_cancelled"]
    assert all(len(e) == 2 for e in ent[w]) and not any(X[w]) and not any(ent[win["empty"]])


@pytest.mark.parametrize("glv,c,red_log,tree,levels,claims", [
    (1, 13, 2, 1, (8, 9), {"fin.q0": {SAME, NEG}, "fin.q1": {SAME, NEG}}),
    (0, 14, 3, 1, (8, 9), {"fin.q0": {SAME, NEG}, "fin.q1": {SAME, NEG}}),
    (1, 12, 0, 2, (8, 9, 10), {"fin.q0": {SAME, NEG}, "fin.q1": {SAME, NEG}, "fin.w4": {SAME, NEG}}),
    (1, 16, 0, 2, (14,), {"fin.wave1": {SAME, NEG}, "fin.w32": {SAME}, "fin.w16": {SAME}, "fin.w8": {SAME},
                          "fin.w4": {SAME}, "fin.q0": {SAME}, "fin.q1": {SAME}}),
])
def test_block_cases_reach_k_group_fin(oracle_cpp, glv, c, red_log, tree, levels, claims):
    """k_group_fin's levels are block-index bits: bit l - 8 of the block for cancel_at(l).  More than
    64 members (wave 1 into wave 0) exist only for the pure tree at c = 16 (128 blocks): msm_plan
    leaves the default tree at more than 64 blocks per window."""
    case = dc.case_blocks(c, red_log, levels)
    check_inputs(case, oracle_cpp)
    T, got, _ = model_single(case, glv, tree)
    assert got % R == case.sum_mult
    T.require(claims, case.name)


@pytest.mark.parametrize("glv,c,red_log", [(1, 11, 2), (0, 12, 3)])
@pytest.mark.parametrize("quad,P", [(True, 1), (True, 4), (False, 1), (False, 4)])
def test_levels_case_on_k_wsum_and_the_group_sums(oracle_cpp, glv, c, red_log, quad, P):
    """J = 256 segments, H = 128 members a group: a thread holds at most one member, so every
    addition that meets two members is in the tree (and, at P = 4, in the fold of part[])."""
    case = dc.case_levels(c, red_log)
    T, got, _ = model_single(case, glv, tree=0, P=P, quad=quad)
    assert got % R == case.sum_mult
    both = {SAME, NEG}
    if quad:
        lv = ["gs.q0", "gs.q1", "gs.w16", "gs.w8", "gs.w4"] + (["gs.w32", "gs.x4"] if P == 1 else [])
    else:
        lv = ["gs.w16", "gs.w8", "gs.w4", "gs.w2", "gs.w1"] + (["gs.lds64", "gs.w32"] if P == 1 else [])
    claims = {k: both for k in lv}
    claims.update({"run+cur": {SAME}, "acc+run": {SAME}})
    if P > 1:
        claims["gs.part"] = both
    T.require(claims, (case.name, quad, P))


def test_pieces_case(oracle_cpp):
    """Three sections +mult, -mult, +mult on section boundaries that piece_bounds keeps (multiples of
    1024 rows): the first two cancel in every bucket, all three leave case_levels' table."""
    size = 12288
    case = dc.case_pieces(11, 2, size)
    assert case.bases.shape[0] == 3 * size and size % 1024 == 0
    check_inputs(case, oracle_cpp)
    lat = dc.lattice()
    one = dc.case_levels(11, 2)
    X1, _ = bucket_table(one.bases, one.scalars, 11, 12, lat)
    X12, e12 = bucket_table(case.bases[:2 * size], case.scalars[:2 * size], 11, 12, lat)
    X, ent = bucket_table(case.bases, case.scalars, 11, 12, lat)
    assert X == X1 and not any(any(r) for r in X12)
    assert sum(len(e) for r in e12 for e in r) == 2 * sum(1 for r in X1 for v in r if v)
    assert case.sum_mult == one.sum_mult
    T, got, _ = model_single(case, 1, tree=1, all_present=True)
    T.require({lv: {SAME, NEG} for lv in LEVELS}, case.name)


# ---- the batch ---------------------------------------------------------------------------------
def batch_arrays(msms, lat):
    """(bases, scalars, offsets) of a list of [(scalar, multiple of P)] MSMs."""
    off, sc, ms = [0], [], []
    for terms in msms:
        sc += [s for s, _ in terms]
        ms += [m for _, m in terms]
        off.append(len(sc))
    S = np.array([[(s >> (64 * k)) & (2 ** 64 - 1) for k in range(4)] for s in sc], dtype=np.uint64)
    return lat.rows_of(ms), S, off


def scan_and_tree(s, T, name):
    nb = len(s)
    d = 1
    while d < nb:  # Hillis-Steele: every bucket reads the old value of bucket b + d
        s = [T.add("%s.scan%d" % (name, d), s[k], s[k + d]) if k + d < nb else s[k] for k in range(nb)]
        d *= 2
    h = nb // 2
    while h >= 1:
        for k in range(h):
            s[k] = T.add("%s.tree%d" % (name, h), s[k], s[k + h])
        h //= 2
    return s[0]


def model_batch(terms, c):
    """One small MSM through the batch reductions at window width c (all routes at once)."""
    lat = dc.lattice()
    W = -(-128 // c)
    bases, S, _ = batch_arrays([terms], lat)
    X, ent = bucket_table(bases, S, c, W, lat)
    T = Tally()
    nb = 1 << (c - 1)
    for w in range(W):
        for e in ent[w]:
            for stride, name in ((1, "chain1"), (4, "chain4"), (16, "chain16")):
                parts = []
                for k in range(stride):
                    a = 0
                    for v in e[k::stride]:
                        a = T.add(name, a, v)
                    parts.append(a)
                if stride == 4:  # bucket_sum_q: (0 + 1) + (2 + 3)
                    T.add("bq1", T.add("bq0", parts[0], parts[1]), T.add("bq0", parts[2], parts[3]))
    tw = [scan_and_tree(list(X[w]), T, "win") for w in range(W)]
    assert [sum((k + 1) * v for k, v in enumerate(X[w])) for w in range(W)] == tw
    acc = tw[W - 1]
    for w in range(W - 2, -1, -1):
        acc = T.add("horner", acc << c, tw[w])
    hb = []
    for k in range(nb):
        a = X[W - 1][k]
        for w in range(W - 2, -1, -1):
            a = T.add("bhorner", a << c, X[w][k])
        hb.append(a)
    assert scan_and_tree(hb, T, "hb") == acc == value_of(X, c)
    if c == 5:  # k_batch_uwin: U_kk = sum of the S_b whose magnitude b + 1 has bit kk set
        for w in range(W):
            for kk in range(4):
                member = lambda i: (((i >> kk) << (kk + 1)) | (1 << kk) | (i & ((1 << kk) - 1))) - 1
                x = [T.add("u5", X[w][member(j)], X[w][member(j + 4)]) for j in range(4)]
                x = [T.add("u6", x[0], x[2]), T.add("u6", x[1], x[3])]
                T.add("u7", x[0], x[1])
    return T, acc


BATCH_CLAIMS = {
    "buckets_equal": {5: {"win.scan1": {SAME}, "win.scan2": {SAME}, "win.scan4": {SAME}, "win.scan8": {SAME},
                          "hb.scan1": {SAME}, "hb.scan8": {SAME},
                          "u5": {SAME}, "u6": {SAME}, "u7": {SAME}},
                      8: {"win.scan1": {SAME}, "win.scan64": {SAME}}},
    "buckets_alternate": {5: {"win.scan1": {NEG}, "hb.scan1": {NEG}, "u5": {SAME}}, 8: {"win.scan1": {NEG}}},
    "buckets_half_neg": {5: {"u5": {NEG}}, 8: {}},
    "horner_dbl": {5: {"horner": {SAME}}, 8: {"horner": {SAME}}},
    "horner_dbl_two_terms": {5: {"horner": {SAME}, "chain1": {SAME}}, 8: {"horner": {SAME}, "chain1": {SAME}}},
    "horner_neg": {5: {"horner": {NEG}}, 8: {"horner": {NEG}}},
    "bucket_horner_dbl": {5: {"bhorner": {SAME}}, 8: {"bhorner": {SAME}}},
    "bucket_horner_neg": {5: {"bhorner": {NEG}}, 8: {"bhorner": {NEG}}},
    "quad_partials_equal": {5: {"bq0": {SAME}, "bq1": {SAME}, "chain4": {SAME}, "chain1": {SAME}},
                            8: {"chain1": {SAME}}},
    "quad_partials_cancel": {5: {"bq0": {NEG}, "chain1": {NEG}}, 8: {"chain1": {NEG}}},
}


@pytest.mark.parametrize("c", [5, 8])
def test_batch_cases(oracle_cpp, c):
    lat = dc.lattice()
    msms = dc.batch_msms(c)
    assert {n for n, _ in msms} == set(BATCH_CLAIMS)
    for name, terms in msms:
        bases, S, _ = batch_arrays([terms], lat)
        top = max(s for s, _ in terms)
        assert top < dc.SCALAR_BOUND and dc.glv_coefficients(top) == (0, 0)
        T, acc = model_batch(terms, c)
        closed = sum(s * m for s, m in terms) % R
        assert acc % R == closed
        assert lat.point(closed) == b.g1_from_bytes(oracle_cpp.msm_pippenger(bases, S, 1).tobytes()), name
        T.require(BATCH_CLAIMS[name][c], (name, c))


def test_edge_msms_are_the_edge_suite():
    """The 8 MSMs of test_gpu_msm_batch.py::test_edge_suite_per_msm, and what each one sums to."""
    msms = dc.edge_msms()
    assert [len(m) for m in msms] == [2, 2, 2, 40, 2, 37, 70, 33]
    want = [b.native_msm([s for s, _ in p], [q for _, q in p]) for p in msms]
    assert want[0] is None and want[2] is None and want[4] is None and want[1] is not None


# ---- fixed tables ------------------------------------------------------------------------------
def model_fixed(terms, mults):
    """k_msm_batch_fixed on multiples of P: 32 signed 8-bit digits of the whole scalar, digit d of
    window w adds 2^(8 w) row to bucket |d| - 1; two threads per bucket sum every other entry."""
    T = Tally()
    chunks = [terms[k:k + 256] for k in range(0, len(terms), 256)]
    half = [[0, 0] for _ in range(128)]
    for chunk in chunks:
        ent = [[] for _ in range(128)]
        for s, row in chunk:
            digits, _ = signed_digits(s, 8, 32)
            for w, d in enumerate(digits):
                if d and mults[row]:
                    ent[abs(d) - 1].append((mults[row] << (8 * w)) * (1 if d > 0 else -1))
        for k in range(128):
            for part in range(2):
                for v in ent[k][part::2]:
                    half[k][part] = T.add("fx.chain", half[k][part], v)
    s = [T.add("fx.halves", h[0], h[1]) for h in half]
    return T, scan_and_tree(s, T, "fx")


FIXED_CLAIMS = {
    "coincide_two_halves": {"fx.halves": {SAME}},
    "coincide_chain": {"fx.chain": {SAME}, "fx.halves": {SAME}},
    "opposite_halves": {"fx.halves": {NEG}},
    "opposite_chain": {},  # which entries share a thread depends on the scatter's order: no claim
    "identity_row": {"fx.halves": {SAME}},
    "buckets_equal": {"fx.scan%d" % d: {SAME} for d in (1, 2, 4, 8, 16, 32, 64)},
    "buckets_alternate": {"fx.scan1": {NEG}},
    "two_chunks": {"fx.chain": {SAME}},
}
# (the tree over the suffix sums R_b = (nb - b) P never doubles: they are all different.  It meets the
# identity and cancellations in buckets_alternate: R_b = P, 0, P, 0, ...)
FIXED_CLAIMS["buckets_alternate"].update({"fx.tree64": {BOTH, SAME}})


def test_fixed_cases():
    pts, mults = dc.fixed_table()
    assert len({dc.point_rows([p]).tobytes() for p in pts}) == len(pts) == len(dc.FIXED_ROWS)  # no row repeats
    assert b.g1_mul(pts[0], 1 << 8) == pts[1] and b.g1_neg(pts[1]) == pts[3]      # yet Q_1(P) == Q_0(2^8 P)
    msms = dc.fixed_msms()
    assert {n for n, _ in msms} == set(FIXED_CLAIMS)
    q = 1 << 200 | 12345  # the stand-in multiplier of row Q
    for name, terms in msms:
        T, acc = model_fixed(terms, [q if m is None else m for m in mults])
        assert acc == sum(s * (q if mults[r] is None else mults[r]) for s, r in terms), name
        T.require(FIXED_CLAIMS[name], name)
