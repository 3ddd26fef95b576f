"""Case builders of the degenerate-addition suite (not collected by pytest; no GPU, no torch, nothing
here imports the library).  tests/test_degenerate_cases.py proves on the CPU that every case meets
the operand classes it claims; tests/test_gpu_msm_degenerate.py and
tests/test_gpu_msm_batch_degenerate.py run the cases through the kernels.

The lattice MSM.  Every base is a multiple m P of one point P = 987654321 G, taken from a small
table (Lattice: built once with b.g1_mul, expanded by numpy indexing), and every term is
(d 2^(c w), m P) with a digit d in [1, 2^(c-1)].  The signed-digit rule (for_each_digit, msm.hip;
the same rule in k_batch_prep, k_msm_batch_windows and k_msm_batch_fixed) maps a window value
<= 2^(c-1) to itself without a carry, so the term adds exactly m P to bucket d - 1 of window w and
nothing anywhere else: a case is a table mult[w][b] of the multiple of P each bucket holds, realised
by one or two terms per entry.

Every scalar is below 2^125.  The GLV split (glv.hpp) rounds c1 = round(k b2 / r) and
c2 = round(k B1 / r); with b2 < 2^64, B1 < 2^127 and r > 2^253 both quotients are below 1/2 for
k < 2^125, so c1 = c2 = 0 and the split leaves k1 = k, k2 = 0: the same arrays drive the same
buckets with the split on and off.  (Below 2^126 alone the second quotient reaches 0.57: a scalar
just under 2^126 rounds to c2 = 1.  glv_coefficients() restates the rounding in integers;
tests/test_degenerate_cases.py checks it for every case.)

Expected values.  A pure lattice MSM expects ((sum s_i m_i) mod r) P, one b.g1_mul, independent of
any bucket method; a case with random rows expects oracle_cpp.msm_pippenger on the same arrays.
"""
from collections import namedtuple

import numpy as np

from oracle import bn254 as b

R = b.R
SEED_MULT = 987654321
SCALAR_BOUND = 1 << 125

# glv.hpp: g_i = floor(2^256 x_i / r) for x_1 = b2 (GLV_G1), x_2 = B1 (GLV_G2)
GLV_G1 = 0x00000002_d91d232e_c7e0b3d7
GLV_G2 = 0x00000002_4ccef014_a773d2cf_7a7bd9d4_391eb18d


def glv_coefficients(k):
    """(c1, c2) of glv_split: floor((k g_i + 2^255) / 2^256)."""
    return (k * GLV_G1 + (1 << 255)) >> 256, (k * GLV_G2 + (1 << 255)) >> 256


def point_rows(points):
    """(n, 8) u64 canonical affine rows of the C ABI; None is the identity (0, 0)."""
    return np.frombuffer(b"".join(b.g1_bytes(p) for p in points), dtype=np.uint64).reshape(-1, 8).copy()


class Lattice:
    """Rows of m P for |m| in `mults` (and the identity for m = 0)."""

    def __init__(self, mults=(1, 2, 3, 4, 32, 256), seed_mult=SEED_MULT):
        self.P = b.g1_mul(b.G1_GEN, seed_mult)
        self.mults = sorted({abs(m) for m in mults} - {0})
        pts, self.slot = [None], {0: 0}
        for m in self.mults:
            pt = b.g1_mul(self.P, m)
            for sm, q in ((m, pt), (-m, b.g1_neg(pt))):
                self.slot[sm] = len(pts)
                pts.append(q)
        self.points = pts
        self.rows = point_rows(pts)
        self._mult_of = {self.rows[i].tobytes(): m for m, i in self.slot.items()}

    def rows_of(self, mults):
        return self.rows[np.array([self.slot[int(m)] for m in mults], dtype=np.int64)]

    def mult_of(self, row):
        """The multiple of P a base row holds; None for a row that is not in the table."""
        return self._mult_of.get(np.ascontiguousarray(row, dtype=np.uint64).tobytes())

    def point(self, k):
        return b.g1_mul(self.P, k % R)


_LATTICE = None


def lattice():
    global _LATTICE
    if _LATTICE is None:
        _LATTICE = Lattice()
    return _LATTICE


def scalar_rows(digits, shifts):
    """(n, 4) u64 limbs of d_i 2^(shift_i), d_i < 2^16, shift_i + 16 <= 192."""
    d = np.asarray(digits, dtype=np.uint64)
    sh = np.asarray(shifts, dtype=np.uint64)
    q, r = (sh >> np.uint64(6)).astype(np.int64), sh & np.uint64(63)
    out = np.zeros((d.shape[0], 4), dtype=np.uint64)
    idx = np.arange(d.shape[0])
    out[idx, q] = d << r
    hi = np.where(r > 0, d >> ((np.uint64(64) - r) & np.uint64(63)), np.uint64(0)).astype(np.uint64)
    out[idx, q + 1] |= hi
    return out


def limbs_to_ints(rows):
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in np.asarray(rows)]


Case = namedtuple("Case", "name c red_log patterns bases scalars sum_mult pure")
Case.__doc__ = """One MSM: `patterns` {window: pattern name}; `sum_mult` = sum s_i m_i mod r over the lattice
terms (the whole MSM when `pure`); bases (n, 8) and scalars (n, 4) u64, canonical."""


class Builder:
    """Collects deposits (window, bucket, multiple of P or a random row) and realises them as terms."""

    def __init__(self, c, red_log, lat=None):
        self.c, self.red_log = c, red_log
        self.B, self.L = 1 << (c - 1), 1 << red_log
        self.J = self.B >> red_log
        self.lat = lat or lattice()
        self.w, self.bk, self.rows, self.m = [], [], [], []
        self.patterns = {}
        self.pure = True

    def _check(self, w, buckets):
        assert self.c * w + self.c <= 125, "the window's largest digit would pass 2^125"
        assert len(buckets) == 0 or (0 <= int(np.min(buckets)) and int(np.max(buckets)) < self.B)

    def deposit(self, w, buckets, mults):
        buckets = np.asarray(buckets, dtype=np.int64)
        mults = np.broadcast_to(np.asarray(mults, dtype=np.int64), buckets.shape)
        self._check(w, buckets)
        self.w.append(np.full(buckets.shape, w, dtype=np.int64))
        self.bk.append(buckets)
        self.rows.append(self.lat.rows_of(mults))
        self.m.append(mults.copy())

    def deposit_rows(self, w, buckets, rows):
        buckets = np.asarray(buckets, dtype=np.int64)
        self._check(w, buckets)
        assert rows.shape == (buckets.shape[0], 8)
        self.w.append(np.full(buckets.shape, w, dtype=np.int64))
        self.bk.append(buckets)
        self.rows.append(np.asarray(rows, dtype=np.uint64))
        self.m.append(np.zeros(buckets.shape, dtype=np.int64))
        self.pure = False

    def name(self, w, pattern):
        assert w not in self.patterns
        self.patterns[w] = pattern

    # ---- the patterns of the issue; seg(b) = b >> red_log is the running-sum segment of bucket b
    def all_equal(self, w):
        """Every bucket holds P."""
        self.name(w, "all_equal")
        self.deposit(w, np.arange(self.B), 1)

    def cancel_at(self, w, level):
        """+P where bit `level` of the segment index is 0, -P where it is 1."""
        assert (1 << level) < self.J
        self.name(w, "cancel_at(%d)" % level)
        bk = np.arange(self.B)
        self.deposit(w, bk, np.where(((bk >> self.red_log) >> level) & 1, -1, 1))

    def segment_cancel(self, w):
        """Cancellations inside the running sums.  Read from a segment's top bucket down, groups of
        four buckets hold P, -2P, (P and -P: the stored cancelled record), P: `run + cur` adds the
        cancelled record and then meets run == -cur, `acc + run` meets acc == -run at the second
        bucket."""
        assert self.L >= 4
        self.name(w, "segment_cancel")
        bk = np.arange(self.B)
        pos = (self.L - 1 - (bk & (self.L - 1))) & 3  # 0 at the segment's top bucket
        self.deposit(w, bk[pos != 2], np.array([1, -2, 0, 1])[pos[pos != 2]])
        self.deposit(w, bk[pos == 2], 1)
        self.deposit(w, bk[pos == 2], -1)

    def mixed(self, w, rand_rows, level=None):
        """Segments 0, 1 (mod 4) from all_equal (level None) or cancel_at(level), the others distinct
        random points, one per bucket."""
        self.name(w, "mixed" if level is None else "mixed_cancel(%d)" % level)
        bk = np.arange(self.B)
        seg = bk >> self.red_log
        lat = (seg & 3) < 2
        m = np.ones(self.B, dtype=np.int64) if level is None else np.where((seg >> level) & 1, -1, 1)
        self.deposit(w, bk[lat], m[lat])
        k = int((~lat).sum())
        assert rand_rows.shape[0] >= k
        self.deposit_rows(w, bk[~lat], rand_rows[:k])
        return k

    def combine_pair(self, w, sign):
        """host_combine (msm.hip) is ONE chain over every exponent, not a Horner per window, so the
        issue's T_w = +-2^c T_(w+1) is built for that chain: with nothing but identities above,
        window w + 1 holds P in bucket 0 (A at exponent c (w + 1)) and window w holds sign 4P in the
        first bucket of segment J / 2, whose total is U_(logJ-1) at exponent c w + c - 2.  Two
        doublings after A the chain holds 4P and adds sign 4P: a == b for +1, a == -b for -1.  The
        -1 pair also holds 4P in bucket 0 of window w, so that A of window w is the identity (or
        A_lo = -A_hi) and the chain is back at the identity below it: the +1 pair goes under it."""
        self.name(w, "combine(%+d)" % sign)
        self.name(w + 1, "combine_top(%+d)" % sign)
        self.deposit(w + 1, [0], 1)
        self.deposit(w, [(self.J // 2) << self.red_log], 4 * sign)
        if sign < 0:
            self.deposit(w, [0], 4)

    def empty_but_cancelled(self, w):
        """Every bucket received P and -P: all records are stored identities, none is empty."""
        self.name(w, "empty_but_cancelled")
        bk = np.arange(self.B)
        self.deposit(w, bk, 1)
        self.deposit(w, bk, -1)

    def really_empty(self, w):
        self.name(w, "empty")

    def terms(self):
        """(windows, buckets, rows, multiples) of the deposits, in deposit order."""
        return (np.concatenate(self.w), np.concatenate(self.bk), np.concatenate(self.rows), np.concatenate(self.m))

    def build(self, name, sections=None):
        """The MSM.  `sections` = (signs, size): the terms repeated once per sign, each repeat padded
        with zero scalars to `size` rows and its lattice bases negated for sign -1 (the pieces of a
        host-fed call: piece 2 adds -mult to what piece 1 stored)."""
        w, bk, rows, m = self.terms()
        sc = scalar_rows(bk + 1, w * self.c)
        if sections is not None:
            assert self.pure
            signs, size = sections
            pad = size - rows.shape[0]
            assert pad >= 0
            pad_rows, pad_sc = np.tile(self.lat.rows_of([1]), (pad, 1)), np.zeros((pad, 4), dtype=np.uint64)
            rows = np.concatenate([x for sg in signs for x in (self.lat.rows_of(sg * m), pad_rows)])
            sc = np.concatenate([x for _ in signs for x in (sc, pad_sc)])
            m = np.concatenate([x for sg in signs for x in (sg * m, np.zeros(pad, dtype=np.int64))])
        s_int = limbs_to_ints(sc)
        total = sum(s * int(k) for s, k in zip(s_int, m) if k) % R
        return Case(name, self.c, self.red_log, dict(self.patterns), np.ascontiguousarray(rows),
                    np.ascontiguousarray(sc), total, self.pure)


def expected_point(case, oracle_cpp=None, lat=None):
    """The closed form of a pure lattice case, the oracle's Pippenger otherwise."""
    if case.pure:
        return (lat or lattice()).point(case.sum_mult)
    return b.g1_from_bytes(oracle_cpp.msm_pippenger(case.bases, case.scalars, 0).tobytes())


# ---- the single-MSM cases ---------------------------------------------------------------------
def case_levels(c, red_log):
    """all_equal and cancel_at(l) for every in-block level l < min(8, logJ), one window each."""
    bd = Builder(c, red_log)
    bd.all_equal(0)
    for l in range(min(8, c - 1 - red_log)):
        bd.cancel_at(1 + l, l)
    return bd.build("levels-c%d-L%d" % (c, red_log))


def case_blocks(c, red_log, levels):
    """all_equal and cancel_at(l) for the given block-index levels (l >= 8: k_group_fin's)."""
    bd = Builder(c, red_log)
    bd.all_equal(0)
    for i, l in enumerate(levels):
        bd.cancel_at(1 + i, l)
    return bd.build("blocks-c%d-L%d-%s" % (c, red_log, "_".join(map(str, levels))))


def case_mixed(c, red_log, rand_rows):
    """segment_cancel (L >= 4), mixed, mixed_cancel, the two host_combine pairs, a cancelled window
    beside an empty one."""
    bd = Builder(c, red_log)
    w = 0
    if bd.L >= 4:
        bd.segment_cancel(w)
        w += 1
    used = bd.mixed(w, rand_rows)
    bd.mixed(w + 1, rand_rows[used:], level=0)  # level 0 is the only one that pairs two lattice segments
    bd.combine_pair(w + 2, +1)
    bd.combine_pair(w + 4, -1)  # the upper pair: everything above it sums to the identity
    bd.empty_but_cancelled(w + 6)
    bd.really_empty(w + 7)
    return bd.build("mixed-c%d-L%d" % (c, red_log))


def mixed_rand_count(c):
    return 1 << (c - 1)  # two windows, half the buckets each


def case_pieces(c, red_log, size):
    """case_levels' table as three sections (+mult, -mult, +mult) of `size` rows: fed in three
    pieces, piece 2 ends every bucket on the identity and piece 3 starts from those records; in one
    piece every bucket holds P, -P, P."""
    bd = Builder(c, red_log)
    bd.all_equal(0)
    for l in range(min(8, c - 1 - red_log)):
        bd.cancel_at(1 + l, l)
    return bd.build("pieces-c%d-L%d" % (c, red_log), sections=((1, -1, 1), size))


# ---- the batch cases --------------------------------------------------------------------------
# One small MSM each: (name, [(scalar, multiple of P or a point)]).  c = 5: 16 buckets, windows
# 0 .. 24 (5 w + 5 <= 125); c = 8: 128 buckets, windows 0 .. 14.
def _term(c, w, d, m):
    assert 1 <= d <= 1 << (c - 1) and c * w + c <= 125
    return (d << (c * w), m)


def batch_msms(c=5):
    """The degenerate small MSMs at window width c (5 or 8) as lists of (scalar, multiple of P)."""
    nb = 1 << (c - 1)
    top = 24 if c == 5 else 14
    big = 1 << c  # 32 or 256: both are in the lattice table
    out = []
    # every bucket of windows 0 and 7 holds P: the suffix scan and the tree over R_b double at every step
    out.append(("buckets_equal", [_term(c, w, d, 1) for w in (0, 7) for d in range(1, nb + 1)]))
    # alternate +-P: the scan's first step cancels, the later ones add identities
    out.append(("buckets_alternate", [_term(c, w, d, 1 if d & 1 else -1) for w in (1, 5) for d in range(1, nb + 1)]))
    # the sign follows bit 3 of the magnitude: k_batch_uwin's members j and j + 4 of U_0 are opposite
    out.append(("buckets_half_neg", [_term(c, 2, d, -1 if (d >> 3) & 1 else 1) for d in range(1, 17)]))
    # window sums: T_top = P, T_(top-1) = +-2^c P (digit 2^(c-1) of 2P; two digit-2^(c-1) terms of P)
    out.append(("horner_dbl", [_term(c, top, 1, 1), _term(c, top - 1, nb, 2)]))
    out.append(("horner_dbl_two_terms", [_term(c, top, 1, 1), _term(c, top - 1, nb, 1), _term(c, top - 1, nb, 1)]))
    out.append(("horner_neg", [_term(c, top, 1, 1), _term(c, top - 1, nb, -2)]))
    # the same in ONE bucket (the bucket-wise Horner H_b of horner_msm): bucket 2 holds P, then +-2^c P
    out.append(("bucket_horner_dbl", [_term(c, top, 3, 1), _term(c, top - 1, 3, big)]))
    out.append(("bucket_horner_neg", [_term(c, 9, 3, 1), _term(c, 8, 3, -big)]))
    # 4k copies of one term in one bucket: bucket_chain strides by 4, the quad's four partial sums are equal
    out.append(("quad_partials_equal", [_term(c, 3, 7, 1)] * 8 + [_term(c, 2, 16, 2)] * 4))
    # and opposite: the partial sums cancel pairwise
    out.append(("quad_partials_cancel", [_term(c, 3, 7, m) for m in (1, -1, 1, -1)] +
                [_term(c, 4, 1, m) for m in (1, 1, -1, -1)] + [_term(c, 6, 2, 1)]))
    return out


def edge_msms():
    """The 8 MSMs of test_gpu_msm_batch.py::test_edge_suite_per_msm, unchanged, as (scalar, point)."""
    import random
    P = b.g1_mul(b.G1_GEN, 987654321)
    Q = b.g1_mul(b.G1_GEN, 5)
    return [
        [(0, P), (0, Q)],
        [(3, None), (4, P)],
        [(7, P), (7, b.g1_neg(P))],
        [(11, P)] * 40,
        [(R - 1, P), (1, P)],
        [(1 << k, Q) for k in range(0, 254, 7)],
        [(R - 1, Q)] * 70,
        [(random.Random(3).randrange(R), P) for _ in range(33)],
    ]


# ---- fixed tables (k_msm_batch_fixed: c = 8, 128 buckets, 32 windows of the WHOLE scalar, no split;
# row i is expanded to Q_w(row i) = 2^(8 w) row i, and a digit d of window w adds Q_w to bucket d - 1)
FIXED_ROWS = ("P", "2^8 P", "2^16 P", "-2^8 P", "identity", "Q")


def fixed_table(lat=None):
    """Rows {P, 2^8 P, 2^16 P, -(2^8 P), identity, Q}: Q_1(P) == Q_0(2^8 P) though no row repeats."""
    lat = lat or lattice()
    P = lat.P
    p8 = b.g1_mul(P, 1 << 8)
    pts = [P, p8, b.g1_mul(P, 1 << 16), b.g1_neg(p8), None, b.g1_mul(b.G1_GEN, 5)]
    mults = [1, 1 << 8, 1 << 16, -(1 << 8), 0, None]  # of P; Q is 5 G
    return pts, mults


def fixed_msms():
    """(name, [(scalar, row)]) over fixed_table()'s rows."""
    d = lambda w, k: k << (8 * w)  # digit k of window w
    out = []
    # one bucket (digit 9): Q_1(P) and Q_0(2^8 P) coincide -> the two threads of the bucket hold equal halves
    out.append(("coincide_two_halves", [(d(1, 9), 0), (d(0, 9), 1)]))
    # the same point four times: each half doubles inside its chain, then the halves are equal
    out.append(("coincide_chain", [(d(2, 9), 0), (d(1, 9), 1), (d(0, 9), 2), (d(2, 9), 0)]))
    # opposite: Q_1(P) and Q_0(-2^8 P) in one bucket, in one half (entries 0 and 2) and across the halves
    out.append(("opposite_halves", [(d(1, 9), 0), (d(0, 9), 3)]))
    out.append(("opposite_chain", [(d(1, 9), 0), (d(0, 77), 5), (d(0, 9), 3), (d(0, 77), 5)]))
    # identity row among them
    out.append(("identity_row", [(d(1, 9), 4), (d(1, 9), 0), (d(0, 9), 1), (d(3, 9), 4)]))
    # every bucket holds P: neighbouring S_b equal, the 7-level scan and tree double at every step
    out.append(("buckets_equal", [(d(0, k), 0) for k in range(1, 129)]))
    # alternate +-2^8 P
    out.append(("buckets_alternate", [(d(0, k), 1 if k & 1 else 3) for k in range(1, 129)]))
    # more than one LDS chunk (256 terms): bucket sums carried across chunks meet their own value again
    out.append(("two_chunks", [(d(0, k % 128 + 1), 0) for k in range(300)]))
    return out
