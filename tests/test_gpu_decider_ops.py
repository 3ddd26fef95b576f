"""The KZG decider's Fq12 lane operations (csrc/decider.hip), one operation per launch, against a
plain big-integer reference -- exact comparisons, no tolerance anywhere.

tests/test_gpu_decider.py pushes random accumulators through the whole pairing; the code's
correctness argument is about bounds that random values never come near.  Here, through the
test-only harness tests/native/decidercheck.hip (built by __graft_entry__.build()):

  (a) norm24 / lz_reduce over the whole range of signed 24-bit limb sums and 9-word values;
  (b) the workgroup kernel's slot operations w_mul (all conj flags), w_sqr, w_frob, w_conj and
      w_norm_inv on edge operands in BOTH representatives x and x + p of every residue (slots are
      [0, 2p)), and on sparse operands that isolate single lane roles;
  (c) operand families that drive a coefficient's signed lane sum toward both ends of its range,
      with the multiplier table of wlane_init / keep_send restated here (MUL_Q, SQR_TERMS, _xi_wrap);
  (d) the single-wave kernel's group operations at S = 4 and S = 8 (the half-product forms), the
      prologue's conv6 and the merge_products pair.

The reference (r_mul, r_sqr, r_line, r_frob, r_conj, r_inv) is Fq2[w] / (w^6 - (9 + u)) written
out below; test_reference_matches_the_oracle pins it to oracle.bn254's tower arithmetic and to its
generic degree-12 polynomial form.  The two tests without the gpu mark run anywhere.

Device values are Montgomery residues x R (R = 2^256) as 8 x u32 limbs; an Fq12 value is six Fq2
(c0, c1), coefficient k of w^k (csrc/fq12_lanes.hpp).  "raw" below means such limbs as an integer,
"plain" the residue it stands for.
"""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

from conftest import ROOT
from oracle import bn254 as ob

P = ob.P
RP = ob.RP
RINV = pow(1 << 256, -1, P)
BN_X = 0x44E992B44A6909F1
LIB = os.path.join(ROOT, "tests", "native", "build", "libdecidercheck.so")
FIELD_LIB = os.path.join(ROOT, "tests", "native", "build", "libfieldcheck.so")

WG_MUL, WG_SQR, WG_FROB, WG_CONJ, WG_NORM_INV = range(5)
LN_MUL, LN_MSQ, LN_MLINE, LN_MUL_LDS, LN_FROB1, LN_FROB2, LN_FROB3, LN_CONJ, LN_INV, LN_POW_X = range(10)
PR_CONV6, PR_MERGE, PR_MERGE_WIDE = range(3)
FC_MUL_LAZY = 6  # fieldcheck.hip's OP_MUL_LAZY
HIP_INVALID = 1  # hipErrorInvalidValue


# ------------------------------------------------------------------ reference: Fq2[w] / (w^6 - xi)
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2xi(a):  # times 9 + u
    return ((9 * a[0] - a[1]) % P, (a[0] + 9 * a[1]) % P)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


def f2inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, -a[1] * n % P)


ONE12 = [(1, 0)] + [(0, 0)] * 5


def r_mul(a, b):
    out = []
    for k in range(6):
        acc = (0, 0)
        for i in range(6):
            t = f2mul(a[i], b[(k - i) % 6])
            acc = f2add(acc, f2xi(t) if i > k else t)
        out.append(acc)
    return out


def r_sqr(a):
    """Over unordered pairs: a_i a_j lands on w^(i + j), twice when i != j."""
    out = [(0, 0)] * 6
    for i in range(6):
        for j in range(i, 6):
            t = f2mul(a[i], a[j])
            if i != j:
                t = f2add(t, t)
            if i + j >= 6:
                t = f2xi(t)
            out[(i + j) % 6] = f2add(out[(i + j) % 6], t)
    return out


def r_line(f, l0, l1, l3):
    """f (l0 + l1 w + l3 w^3): the 034-type sparse product."""
    out = [(0, 0)] * 6
    for sh, l in ((0, l0), (1, l1), (3, l3)):
        for i in range(6):
            t = f2mul(f[i], l)
            if i + sh >= 6:
                t = f2xi(t)
            out[(i + sh) % 6] = f2add(out[(i + sh) % 6], t)
    return out


@functools.lru_cache(maxsize=None)
def _gammas(n):
    return [f2pow((9, 1), k * (P ** n - 1) // 6) for k in range(6)]


def r_frob(a, n):
    """(g w^k)^(p^n) = conj^n(g) xi^(k (p^n - 1) / 6) w^k."""
    return [f2mul((g[0], -g[1] % P) if n & 1 else g, gam) for g, gam in zip(a, _gammas(n))]


def r_conj(a):
    return [g if k % 2 == 0 else (-g[0] % P, -g[1] % P) for k, g in enumerate(a)]


def r_inv6(nn):
    """1 / N for N on the even coefficients (Fq6 = Fq2[v], v = w^2), by its Frobenius norm to Fq2:
    N^-1 = N^(p^2) N^(p^4) / (N N^(p^2) N^(p^4))."""
    assert all(nn[k] == (0, 0) for k in (1, 3, 5))
    n2 = r_frob(nn, 2)
    n4 = r_frob(n2, 2)
    adj = r_mul(n2, n4)
    norm = r_mul(nn, adj)
    assert all(c == (0, 0) for c in norm[1:]), "the norm of an Fq6 element lies in Fq2"
    ninv = f2inv(norm[0])
    return [f2mul(c, ninv) for c in adj]


def r_inv(a):
    ac = r_conj(a)
    return r_mul(ac, r_inv6(r_mul(a, ac)))


def r_pow(a, e):
    r = ONE12
    for bit in bin(e)[2:]:
        r = r_sqr(r)
        if bit == "1":
            r = r_mul(r, a)
    return r


def to_tower(a):
    """w-basis -> the oracle's tower ((c0.c0, c0.c1, c0.c2), (c1.c0, c1.c1, c1.c2)): tower_coeff's slot map."""
    return ((a[0], a[2], a[4]), (a[1], a[3], a[5]))


def _rand12(rng):
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


def test_reference_matches_the_oracle():
    """The reference above, through the slot map of tower_coeff, equals oracle.bn254's tower
    arithmetic (Karatsuba over Fq6) and its degree-12 polynomial form (w^12 = 18 w^6 - 82)."""
    rng = random.Random(0xDEC1DE)
    for it in range(12):
        a, b = _rand12(rng), _rand12(rng)
        ta, tb = to_tower(a), to_tower(b)
        assert to_tower(r_mul(a, b)) == ob.f12_mul(ta, tb)
        assert to_tower(r_sqr(a)) == ob.f12_sqr(ta)
        assert to_tower(r_conj(a)) == ob.f12_conj(ta)
        for n in (1, 2, 3):
            assert to_tower(r_frob(a, n)) == ob.f12_frob_n(ta, n)
        l0, l1, l3 = b[0], b[1], b[2]
        assert to_tower(r_line(a, l0, l1, l3)) == ob.f12_mul_by_034(ta, l0, l1, l3)
        assert r_line(a, l0, l1, l3) == r_mul(a, [l0, l1, (0, 0), l3, (0, 0), (0, 0)])
        if it < 4:
            assert to_tower(r_inv(a)) == ob.f12_inv(ta)
            assert r_mul(a, r_inv(a)) == ONE12
            assert ob.tower_to_poly(to_tower(r_mul(a, b))) == ob._p12_mul(ob.tower_to_poly(ta), ob.tower_to_poly(tb))
    a = _rand12(rng)
    assert r_pow(a, 11) == r_mul(r_sqr(r_mul(r_sqr(r_sqr(a)), a)), a)
    assert BN_X == ob.U


# ------------------------------------------------- the lane multiplier table of wlane_init / keep_send
# A lane's product v in [0, 2p) enters its coefficient's (re, im) as (m_re v, m_im v).  Partial
# product q of a term x y: 0 x0 y0 (re +), 1 x1 y1 (re -), 2 x0 y1 (im), 3 x1 y0 (im); a wrapped
# term (index sum >= 6) carries xi = 9 + u; a conj flag negates the terms of odd coefficients.
MUL_Q = [(1, 0), (-1, 0), (0, 1), (0, 1)]
# c_sqr (csrc/fq12_lanes.hpp SV_SQR_TERMS): per coefficient the pairs (i, j, doubled, xi)
SQR_TERMS = [
    [(0, 0, 0, 0), (3, 3, 0, 1), (1, 5, 1, 1), (2, 4, 1, 1)],
    [(0, 1, 1, 0), (2, 5, 1, 1), (3, 4, 1, 1)],
    [(1, 1, 0, 0), (0, 2, 1, 0), (4, 4, 0, 1), (3, 5, 1, 1)],
    [(0, 3, 1, 0), (1, 2, 1, 0), (4, 5, 1, 1)],
    [(2, 2, 0, 0), (0, 4, 1, 0), (1, 3, 1, 0), (5, 5, 0, 1)],
    [(0, 5, 1, 0), (1, 4, 1, 0), (2, 3, 1, 0)],
]


def _xi_wrap(re, im):
    return 9 * re - im, re + 9 * im


def mul_roles(conj):
    """(k, (i, comp of a_i), (j, comp of b_j), m_re, m_im) for each of w_mul's 144 lanes."""
    roles = []
    for k in range(6):
        for i in range(6):
            j, wrap = (k - i) % 6, i > k
            flip = bool(conj & 1 and i & 1) != bool(conj & 2 and j & 1)
            for q in range(4):
                re, im = MUL_Q[q]
                if wrap:
                    re, im = _xi_wrap(re, im)
                if flip:
                    re, im = -re, -im
                roles.append((k, (i, q & 1), (j, 1 if q in (1, 2) else 0), re, im))
    return roles


def sqr_roles():
    """w_sqr's live lanes: a square term a_i^2 = a0^2 - a1^2 + 2 a0 a1 u on three lanes, a cross
    term 2 a_i a_j on four (twice the w_mul partial products)."""
    roles = []
    for k, terms in enumerate(SQR_TERMS):
        for (i, j, dbl, xi) in terms:
            assert (i + j) % 6 == k and bool(dbl) == (i != j) and bool(xi) == (i + j >= 6)
            if i == j:
                lanes = [((i, 0), (i, 0), 1, 0), ((i, 1), (i, 1), -1, 0), ((i, 0), (i, 1), 0, 2)]
            else:
                lanes = [((i, q & 1), (j, 1 if q in (1, 2) else 0), 2 * MUL_Q[q][0], 2 * MUL_Q[q][1]) for q in range(4)]
            for x, y, re, im in lanes:
                if xi:
                    re, im = _xi_wrap(re, im)
                roles.append((k, x, y, re, im))
    return roles


def frob_roles(n):
    """w_frob: coefficient k's four partial products of a_k gamma_(n, k); odd n conjugates a_k, i.e.
    negates the lanes that read a_k's c1 (odd q)."""
    roles = []
    for k in range(6):
        for q in range(4):
            re, im = MUL_Q[q]
            if n & 1 and q & 1:
                re, im = -re, -im
            roles.append((k, (k, q & 1), (k, 1 if q in (1, 2) else 0), re, im))
    return roles


def _table_eval(roles, a, b):
    """The coefficients the table stands for, mod p (plain operands)."""
    acc = [[0, 0] for _ in range(6)]
    for k, (i, ci), (j, cj), re, im in roles:
        v = a[i][ci] * b[j][cj]
        acc[k][0] += re * v
        acc[k][1] += im * v
    return [(c[0] % P, c[1] % P) for c in acc]


def _figures(roles):
    """Per coefficient component: (sum of the positive multipliers, of the negative ones' sizes)."""
    out = {}
    for k, _, _, re, im in roles:
        for comp, m in ((0, re), (1, im)):
            pos, neg = out.get((k, comp), (0, 0))
            out[(k, comp)] = (pos + max(m, 0), neg + max(-m, 0))
    return out


def test_lane_multiplier_table_figures():
    """The figures csrc/decider.hip states next to lane_sum24, from the table restated above: over
    one coefficient component the multipliers' sizes sum to at most 102, and 102 (2^24 - 1) < 2^31,
    so every partial lane sum stays an int32 per limb.  Without conj flags (w_mul plain, w_sqr,
    w_frob) the positive ones sum to at most 97 and the negative ones to at most 56, which with
    products in [0, 2p) puts a coefficient in (-112 p, 194 p).  A conj flag negates whole terms, so
    the negative figure does NOT hold under flags: it is 59 with kConjA or kConjB alone and 80 with
    both (every term of an odd coefficient negated), the positive one stays within 97 -- a range of
    (-160 p, 194 p), still positive after the 240 p bias and below 434 p, which is what matters.
    The table also has to BE the operation: evaluated on random operands it equals the reference."""
    rng = random.Random(0x7AB1E)
    a, b = _rand12(rng), _rand12(rng)
    variants = [("w_mul conj=%d" % c, mul_roles(c), c) for c in range(4)]
    variants += [("w_sqr", sqr_roles(), 0)] + [("w_frob n=%d" % n, frob_roles(n), 0) for n in (1, 2, 3)]
    assert len(mul_roles(0)) == 144 and len(sqr_roles()) <= 96
    for name, roles, conj in variants:
        fig = _figures(roles)
        pos, neg = max(v[0] for v in fig.values()), max(v[1] for v in fig.values())
        tot = max(v[0] + v[1] for v in fig.values())
        print(f"{name}: positive <= {pos}, negative <= {neg}, total <= {tot}")
        assert tot <= 102, name
        assert tot * ((1 << 24) - 1) < 1 << 31
        if conj == 0:
            assert pos <= 97 and neg <= 56, name
        else:
            assert pos <= 97 and neg <= 80, name
        # the biased sum is positive and fits what lz_reduce takes
        assert 2 * neg <= 240 and (2 * pos + 240) * P < 1 << 263, name
    assert 102 * ((1 << 24) - 1) < 1 << 31
    fig = _figures(mul_roles(0))
    assert max(v[0] for v in fig.values()) == 97 and max(v[1] for v in fig.values()) == 56
    fig = _figures(sqr_roles())
    assert max(v[0] for v in fig.values()) == 97 and max(v[1] for v in fig.values()) == 56
    for c in range(4):
        ac = r_conj(a) if c & 1 else a
        bc = r_conj(b) if c & 2 else b
        assert _table_eval(mul_roles(c), a, b) == r_mul(ac, bc)
    assert _table_eval(sqr_roles(), a, a) == r_sqr(a)
    for n in (1, 2, 3):
        assert _table_eval(frob_roles(n), a, _gammas(n)) == r_frob(a, n)
    # the tests bite: the sign or the x9 of any single role changed makes the table differ from the
    # reference on the sparse case that isolates the role (see _sparse_pairs)
    for idx in range(144):
        k, x, y, re, im = mul_roles(0)[idx]
        for bad in ((-re, -im), (re if abs(re) != 9 else 1, im if abs(im) != 9 else 1)):
            if bad == (re, im):
                continue
            roles = mul_roles(0)
            roles[idx] = (k, x, y) + bad
            sa, sb = _sparse_one(x[0], x[1], 3), _sparse_one(y[0], y[1], 5)
            assert _table_eval(roles, sa, sb) != r_mul(sa, sb)
            assert _table_eval(mul_roles(0), sa, sb) == r_mul(sa, sb)


# ------------------------------------------------------------------------------ operands
def _edge_raw():
    """Raw limb values below p: 0, 1, R (the Montgomery 1), R^2, the top of the field, halves, powers
    of two, all-ones low limbs, values just below p with ragged low limbs."""
    v = [0, 1, 2, RP, RP * RP % P, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 253, (1 << 253) - 1]
    v += [1 << k for k in range(5, 254, 31)]
    v += [(1 << (32 * k)) - 1 for k in range(1, 8)]
    v += [P - ((1 << (32 * k)) - 1) for k in range(1, 7)]
    v += [(P - 1) ^ ((1 << 32) - 1)]
    out = []
    for x in v:
        if x % P not in out:
            out.append(x % P)
    return out


EDGE = _edge_raw()
EDGE_2P = EDGE + [x + P for x in EDGE]  # both representatives of every residue: x + p < 2p always
assert all(0 <= x < 2 * P for x in EDGE_2P)


def _plain(case):
    """raw Fq12 (any representative) -> plain residues"""
    return [(c0 * RINV % P, c1 * RINV % P) for c0, c1 in case]


def _raw(case):
    return [(c0 * RP % P, c1 * RP % P) for c0, c1 in case]


def _sparse_one(pos, comp, val):
    z = [(0, 0)] * 6
    z[pos] = (val, 0) if comp == 0 else (0, val)
    return z


def _dense(rng, pool, n):
    return [[(rng.choice(pool), rng.choice(pool)) for _ in range(6)] for _ in range(n)]


def _rep_variants(case):
    """The same residues as x + p everywhere, and alternating."""
    hi = [(c0 + P, c1 + P) for c0, c1 in case]
    alt = [(c0 + P * (k & 1), c1 + P * (1 - (k & 1))) for k, (c0, c1) in enumerate(case)]
    return [hi, alt]


def _sparse_pairs(rng):
    """One non-zero coefficient in a (position i) and in b (position j), each real-only or
    imaginary-only: the product has ONE live lane -- w_mul's role (k = i + j mod 6, term i,
    q from the two components) -- so all 6 x 6 x 4 = 144 roles are isolated, every wrap
    (i + j >= 6) alone; under a conj flag the same cases isolate the flipped roles."""
    A, B, seen = [], [], set()
    for i in range(6):
        for ca in range(2):
            for j in range(6):
                for cb in range(2):
                    x = rng.choice([rng.randrange(1, P), P - 1, 1, RP]) + P * rng.randrange(2)
                    y = rng.choice([rng.randrange(1, P), P - 1, 1, RP]) + P * rng.randrange(2)
                    A.append(_sparse_one(i, ca, x))
                    B.append(_sparse_one(j, cb, y))
                    seen.add(((i + j) % 6, i, {(0, 0): 0, (1, 1): 1, (0, 1): 2, (1, 0): 3}[(ca, cb)]))
    assert len(seen) == 144
    return A, B


def _sparse_squares(rng):
    """w_sqr's roles: one non-zero coefficient, real-only / imaginary-only / both (the square
    terms' three lanes), and two non-zero coefficients i < j, each real- or imaginary-only (one lane
    of the cross term {i, j} alone)."""
    A = []
    for i in range(6):
        for ca in range(2):
            A.append(_sparse_one(i, ca, rng.randrange(1, P) + P * rng.randrange(2)))
        z = [(0, 0)] * 6
        z[i] = (rng.randrange(1, 2 * P), rng.randrange(1, 2 * P))
        A.append(z)
        for j in range(i + 1, 6):
            for ca in range(2):
                for cb in range(2):
                    z = _sparse_one(i, ca, rng.randrange(1, 2 * P))
                    z[j] = _sparse_one(j, cb, rng.randrange(1, 2 * P))[j]
                    A.append(z)
    return A


def _extreme_cases():
    top = 2 * P - 1
    return [[(v, v)] * 6 for v in (0, P, top, P - 1, P + 1, 1)]


@pytest.fixture(scope="module")
def wg_operands():
    """(A, B, twins): operand pairs in [0, 2p) for the workgroup operations, shared by the tests
    below; twins are the indices of the groups of four cases that hold the same residues."""
    rng = random.Random(0xDEC0)
    A = _dense(rng, EDGE_2P, 160)
    B = _dense(rng, EDGE_2P, 160)
    # both representatives of the same residues: results must be congruent
    base_a, base_b = _dense(rng, EDGE, 24), _dense(rng, EDGE, 24)
    for a, b in zip(base_a, base_b):
        A += [a] + _rep_variants(a) + [a]
        B += [b] + _rep_variants(b) + [_rep_variants(b)[0]]
    ext = _extreme_cases()
    A += [x for x in ext for _ in ext]
    B += [y for _ in ext for y in ext]
    sa, sb = _sparse_pairs(rng)
    A += sa
    B += sb
    A += _dense(rng, [rng.randrange(2 * P) for _ in range(400)], 32)  # 32 random pairs
    B += _dense(rng, [rng.randrange(2 * P) for _ in range(400)], 32)
    twins = range(160, 160 + 4 * 24)
    return A, B, twins


# ------------------------------------------------------------------------------ device plumbing
def _pack(cases):
    """list of cases, each a list of (c0, c1) raw pairs -> (n, len, 2, 8) uint32"""
    buf = b"".join(c.to_bytes(32, "little") for case in cases for pair in case for c in pair)
    return np.frombuffer(buf, dtype="<u4").reshape(len(cases), len(cases[0]), 2, 8).copy()


def _unpack(arr):
    n, m = arr.shape[0], arr.shape[1]
    raw = arr.astype("<u4").tobytes()
    vals = [int.from_bytes(raw[o:o + 32], "little") for o in range(0, len(raw), 32)]
    return [[(vals[(c * m + k) * 2], vals[(c * m + k) * 2 + 1]) for k in range(m)] for c in range(n)]


@pytest.fixture(scope="module")
def dc():
    assert os.path.exists(LIB), "tests/native/build/libdecidercheck.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(LIB)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.dc_info.argtypes, lib.dc_info.restype = [ci], ci
    lib.dc_wg.argtypes, lib.dc_wg.restype = [ci, ci, vp, vp, vp, sz], ci
    lib.dc_norm24.argtypes, lib.dc_norm24.restype = [ci, vp, vp, sz], ci
    lib.dc_lanes.argtypes, lib.dc_lanes.restype = [ci, ci, vp, vp, vp, vp, sz], ci
    lib.dc_prologue.argtypes, lib.dc_prologue.restype = [ci, vp, vp, vp, sz], ci
    return lib


@pytest.fixture(scope="module")
def fc():
    assert os.path.exists(FIELD_LIB), "tests/native/build/libfieldcheck.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(FIELD_LIB)
    lib.fc_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    lib.fc_run.restype = ctypes.c_int
    return lib


def _wg(dc, op, imm, A, B):
    a, b = _pack(A), _pack(B)
    out = np.zeros_like(a)
    rc = dc.dc_wg(op, imm, a.ctypes.data, b.ctypes.data, out.ctypes.data, len(A))
    assert rc == 0, f"dc_wg hip error {rc}"
    return _unpack(out)


def _lanes(dc, S, op, A, B=None, L=None):
    B = A if B is None else B
    L = [A[0][:3]] * len(A) if L is None else L
    a, b, l = _pack(A), _pack(B), _pack(L)
    out = np.zeros_like(a)
    rc = dc.dc_lanes(S, op, a.ctypes.data, b.ctypes.data, l.ctypes.data, out.ctypes.data, len(A))
    assert rc == 0, f"dc_lanes hip error {rc}"
    return _unpack(out)


def _check_2p(got, want_plain, what):
    """every raw component below 2p and congruent to the expected plain residue"""
    for c, (g, w) in enumerate(zip(got, want_plain)):
        for k in range(6):
            for comp in range(2):
                r = g[k][comp]
                assert r < 2 * P, f"{what} case {c} coefficient {k}.{comp}: {r:#x} is not below 2p"
                assert r * RINV % P == w[k][comp], f"{what} case {c} coefficient {k}.{comp}"


def _check_canonical(got, want_plain, what):
    for c, (g, w) in enumerate(zip(got, want_plain)):
        assert g == _raw(w), f"{what} case {c}"


# ------------------------------------------------------------------ (a) norm24 / lz_reduce
def _limbs24(x):
    """x (possibly negative) as 11 limbs: the low ten in [0, 2^24), the top one signed"""
    s = [(x >> (24 * i)) & 0xFFFFFF for i in range(10)]
    s.append(x >> 240)
    return s


def _neighbours(lo, hi):
    """values inside (lo, hi) at the edges the code estimates and carries at"""
    v = [lo + 1, lo + 2, hi - 1, hi - 2, 0, 1, -1, P, -P]
    for j in range(lo // P, hi // P + 2):
        v += [j * P - 1, j * P, j * P + 1]
    for m in range(lo >> 256, (hi >> 256) + 2):  # every multiple of 2^256
        v += [(m << 256) - 1, m << 256, (m << 256) + 1]
    # multiples of 2^224 (the estimate reads a >> 224): where the estimated quotient steps, i.e. the
    # top words j (p_top + 1) and their neighbours, and a random few hundred
    rng = random.Random(0x224)
    ptop1 = (P >> 224) + 1
    tops = [j * ptop1 + d for j in range(lo // (ptop1 << 224) - 1, hi // (ptop1 << 224) + 2) for d in (-1, 0, 1)]
    tops += [rng.randrange(lo >> 224, hi >> 224) for _ in range(300)]
    for m in tops:
        v += [(m << 224) - 1, m << 224, (m << 224) + 1, (m << 224) + (1 << 224) - 1]
    return [x for x in v if lo < x < hi]


def _norm24_inputs():
    lo, hi = -112 * P, 194 * P
    rng = random.Random(0x24)
    vecs = [_limbs24(x) for x in _neighbours(lo, hi)]
    # ... and the same edges of the biased sum, which is what the carry pass and lz_reduce see
    vecs += [_limbs24(y - 240 * P) for y in _neighbours(lo + 240 * P, hi + 240 * P)]
    vecs += [_limbs24(rng.randrange(lo + 1, hi)) for _ in range(300)]
    # redundant forms: the low ten limbs at the extremes a lane sum can reach, +-102 (2^24 - 1), in
    # runs of one sign (carries that ripple through every limb, both directions) and alternating;
    # the top limb places the total at the bottom, the middle and the top of the range
    m = 102 * ((1 << 24) - 1)
    patterns = [[m] * 10, [-m] * 10, [m if i & 1 else -m for i in range(10)], [-m if i & 1 else m for i in range(10)],
                [m] * 5 + [-m] * 5, [-m] * 5 + [m] * 5, [m, 0] * 5, [0, -m] * 5]
    for low in patterns:
        base = sum(s << (24 * i) for i, s in enumerate(low))
        for target in (lo + 1, lo + (1 << 240), 0, 41 * P, hi - (1 << 240), hi - 1):
            top = (target - base) >> 240
            for t in (top, top + 1):
                if lo < base + (t << 240) < hi:
                    vecs.append(low + [t])
    assert all(abs(s) <= m for v in vecs for s in v)
    return vecs


def _lz_inputs():
    top = (1 << 264) - 1
    rng = random.Random(0x9)
    return _neighbours(-1, top + 1) + [top, 434 * P, 434 * P - 1] + [rng.randrange(top) for _ in range(300)]


def _value24(v):
    return sum(s << (24 * i) for i, s in enumerate(v))


@pytest.mark.gpu
def test_norm24_and_reduce_over_the_whole_sum_range(gpu, dc):
    """lz_reduce(norm24(s)) for signed limb sums s of value in (-112 p, 194 p) -- the bias, the one
    signed carry pass, the byte gathers and the quotient estimate: below 2p, congruent to s."""
    vecs = _norm24_inputs()
    assert dc.dc_info(3) == 11
    arr = np.array(vecs, dtype=np.int64).astype(np.int32)
    out = np.zeros((len(vecs), 8), np.uint32)
    rc = dc.dc_norm24(0, arr.ctypes.data, out.ctypes.data, len(vecs))
    assert rc == 0, f"dc_norm24 hip error {rc}"
    print(f"norm24: {len(vecs)} limb vectors")
    for v, row in zip(vecs, out):
        r = sum(int(w) << (32 * i) for i, w in enumerate(row))
        x = _value24(v)
        assert r < 2 * P, f"sum {x / P:.3f} p: {r:#x} is not below 2p"
        assert (r - x) % P == 0, f"sum {x / P:.3f} p ({v})"


@pytest.mark.gpu
def test_lz_reduce_over_nine_words(gpu, dc):
    """lz_reduce alone on 9-word values: everything the biased sums can be (up to 434 p) and on up
    to its documented limit 2^264 - 1, at multiples of p and at the words the estimate reads."""
    vals = _lz_inputs()
    arr =np.zeros((len(vals), 9), np.uint32)
    for i, x in enumerate(vals):
        for k in range(9):
            arr[i, k] = (x >> (32 * k)) & 0xFFFFFFFF
    out = np.zeros((len(vals), 8), np.uint32)
    rc = dc.dc_norm24(1, arr.ctypes.data, out.ctypes.data, len(vals))
    assert rc == 0, f"dc_norm24 hip error {rc}"
    print(f"lz_reduce: {len(vals)} values")
    for x, row in zip(vals, out):
        r = sum(int(w) << (32 * i) for i, w in enumerate(row))
        assert r < 2 * P and (r - x) % P == 0, f"{x / P:.3f} p -> {r:#x}"


# ------------------------------------------------------------------ (b) the workgroup operations
@pytest.mark.gpu
@pytest.mark.parametrize("conj", [0, 1, 2, 3])
def test_wg_mul(gpu, dc, wg_operands, conj):
    A, B, twins = wg_operands
    got = _wg(dc, WG_MUL, conj, A, B)
    want = []
    for a, b in zip(A, B):
        pa, pb = _plain(a), _plain(b)
        want.append(r_mul(r_conj(pa) if conj & 1 else pa, r_conj(pb) if conj & 2 else pb))
    _check_2p(got, want, f"w_mul conj={conj}")
    for c in twins:  # groups of four cases hold the same residues in different representatives
        assert _plain(got[c]) == _plain(got[c - c % 4]), c


@pytest.mark.gpu
def test_wg_sqr(gpu, dc, wg_operands):
    A, _, twins = wg_operands
    A = A + _sparse_squares(random.Random(0x5A))
    got = _wg(dc, WG_SQR, 0, A, A)
    _check_2p(got, [r_sqr(_plain(a)) for a in A], "w_sqr")
    for c in twins:
        assert _plain(got[c]) == _plain(got[c - c % 4]), c


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_wg_frob(gpu, dc, wg_operands, n):
    A, _, _ = wg_operands
    rng = random.Random(0xF0 + n)
    A = A + [_sparse_one(k, comp, rng.randrange(1, 2 * P)) for k in range(6) for comp in range(2)]
    got = _wg(dc, WG_FROB, n, A, A)
    _check_2p(got, [r_frob(_plain(a), n) for a in A], f"w_frob n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("neg_odd", [0, 1])
def test_wg_conj(gpu, dc, wg_operands, neg_odd):
    """Both representatives of every residue are valid inputs, and the result is a slot value again:
    below 2p.  Regression: the negation of a RAW ZERO on an odd coefficient used to be 2p itself
    (fq_neg2p maps [0, 2p] to [0, 2p]); the extreme cases of wg_operands hold it."""
    A, _, _ = wg_operands
    assert any(a[1] == (0, 0) for a in A)
    got = _wg(dc, WG_CONJ, neg_odd, A, A)
    _check_2p(got, [r_conj(_plain(a)) if neg_odd else _plain(a) for a in A], f"w_conj neg_odd={neg_odd}")
    if not neg_odd:
        assert got == A  # a copy keeps the representative


@pytest.mark.gpu
def test_wg_norm_inv(gpu, dc):
    """ni = N^-1 for N on the even coefficients, each from the edge set in both representatives; the
    odd coefficients of the input are arbitrary and must be ignored."""
    rng = random.Random(0x1AB)
    cases = []
    for x in EDGE_2P:
        for slot in range(3):
            n = [(rng.choice(EDGE_2P), rng.choice(EDGE_2P)) for _ in range(6)]
            n[2 * slot] = (x, rng.choice(EDGE_2P)) if slot != 1 else (rng.choice(EDGE_2P), x)
            for k in (1, 3, 5):
                n[k] = (rng.randrange(2 * P), rng.randrange(2 * P))
            cases.append(n)
    # a single live component: 1 / (c v^j) for each j, real-only and imaginary-only, both representatives
    for k in (0, 2, 4):
        for comp in range(2):
            for val in (1, RP, P - 1, RP + P, 2 * P - 1):
                cases.append(_sparse_one(k, comp, val))
    evens = [[c if k % 2 == 0 else (0, 0) for k, c in enumerate(_plain(n))] for n in cases]
    excluded = sum(1 for e in evens if all(c == (0, 0) for c in e))  # Fq6 is a field: only N = 0 has no inverse
    print(f"w_norm_inv: {len(cases)} cases, {excluded} excluded for a zero norm")
    assert excluded == 0
    got = _wg(dc, WG_NORM_INV, 0, cases, cases)
    for c, (g, e) in enumerate(zip(got, evens)):
        assert all(max(pair) < 2 * P for pair in g), c
        assert all(g[k] == (0, 0) for k in (1, 3, 5)), c
        assert r_mul(_plain(g), e) == ONE12, c


# ------------------------------------------------------------------ (c) lane-sum extremes
def _lazy_products(fc, pairs):
    """fe_mul_lazy(x, y) on the device for each distinct raw pair: the representative in [0, 2p) that
    the lane really adds up"""
    pairs = sorted(pairs)
    a = np.zeros((len(pairs), 8), np.uint32)
    b = np.zeros_like(a)
    for i, (x, y) in enumerate(pairs):
        for k in range(8):
            a[i, k] = (x >> (32 * k)) & 0xFFFFFFFF
            b[i, k] = (y >> (32 * k)) & 0xFFFFFFFF
    out = np.zeros_like(a)
    rc = fc.fc_run(FC_MUL_LAZY, 0, a.ctypes.data, b.ctypes.data, a.ctypes.data, b.ctypes.data, out.ctypes.data, len(pairs))
    assert rc == 0, f"fc_run hip error {rc}"
    res = {}
    for (x, y), row in zip(pairs, out):
        v = sum(int(w) << (32 * i) for i, w in enumerate(row))
        assert v < 2 * P and v % P == x * y * RINV % P
        res[(x, y)] = v
    return res


def _exact_sums(fc, roles, cases):
    """per case, the exact pre-reduction lane sum of every coefficient component (an integer)"""
    need = {(a[i][ci], b[j][cj]) for a, b in cases for _, (i, ci), (j, cj), _, _ in roles}
    lazy = _lazy_products(fc, need)
    sums = []
    for a, b in cases:
        acc = [[0, 0] for _ in range(6)]
        for k, (i, ci), (j, cj), re, im in roles:
            v = lazy[(a[i][ci], b[j][cj])]
            acc[k][0] += re * v
            acc[k][1] += im * v
        sums.append(acc)
    return sums


def _masked(u, a_mask, idx_mask):
    """all components u, with the real (bit 0) / imaginary (bit 1) parts switched on by a_mask and
    the coefficients by idx_mask"""
    return [(u if a_mask & 1 and idx_mask >> k & 1 else 0, u if a_mask & 2 and idx_mask >> k & 1 else 0) for k in range(6)]


def _extreme_families(u, v):
    fam = []
    for am in (1, 2, 3):
        for bm in (1, 2, 3):
            for ia in (0b111111, 0b010101, 0b101010):
                for ib in (0b111111, 0b010101, 0b101010):
                    fam.append((_masked(u, am, ia), _masked(v, bm, ib)))
    return fam


@pytest.mark.gpu
def test_wg_mul_lane_sum_extremes(gpu, dc, fc):
    """Operands u, v with u v / R = p - 1 in every component (switched on and off by real / imaginary
    part and by coefficient parity, under every conj flag), in both representatives of u and v: every
    lane product is the largest residue, so a coefficient's signed lane sum goes as far toward both
    ends as its multipliers allow (+92 and, with kConjA | kConjB, -76 lane products).  The exact sums
    are rebuilt from the multiplier table and the representative fe_mul_lazy really returns.
    Reached on an MI355X: +92.000 p and -76.000 p (fe_mul_lazy returns p - 1 itself for these
    operands, also from x + p inputs); the switched-off families reach no further than the
    all-components-equal one.  Asserted: some coefficient >= 90 p, some <= -74 p."""
    rng = random.Random(0xE7)
    u = rng.randrange(1, P)
    v = (P - 1) * RP * pow(u, -1, P) % P
    assert u * v * RINV % P == P - 1
    hi, lo = 0, 0
    for conj in range(4):
        cases = []
        for uu, vv in ((u, v), (u + P, v + P), (u, v + P)):
            cases += _extreme_families(uu, vv)
        sums = _exact_sums(fc, mul_roles(conj), cases)
        flat = [s for acc in sums for pair in acc for s in pair]
        hi, lo = max(hi, max(flat)), min(lo, min(flat))
        assert all(0 <= s + 240 * P < 434 * P for s in flat)  # what norm24 / lz_reduce are given
        got = _wg(dc, WG_MUL, conj, [c[0] for c in cases], [c[1] for c in cases])
        want = []
        for (a, b), acc in zip(cases, sums):
            pa, pb = _plain(a), _plain(b)
            w = r_mul(r_conj(pa) if conj & 1 else pa, r_conj(pb) if conj & 2 else pb)
            assert [(s[0] * RINV % P, s[1] * RINV % P) for s in acc] == w  # the table's sum IS the product
            want.append(w)
        _check_2p(got, want, f"w_mul extremes conj={conj}")
    print(f"w_mul lane sums reach {hi / P:.3f} p and {lo / P:.3f} p")
    assert hi >= 90 * P and lo <= -74 * P


@pytest.mark.gpu
def test_wg_sqr_lane_sum_extremes(gpu, dc, fc):
    """u with u^2 / R = p - 1 - t for the smallest t that makes it a square (-R is a non-residue:
    p = 3 mod 4), all components equal and switched as above: +92 / -46 lane products.
    Reached on an MI355X: +92.000 p and -46.000 p (t = 2).  Asserted: some coefficient >= 90 p,
    some <= -44 p."""
    t = 0
    while ob.sqrt_fp((P - 1 - t) * RP % P) is None:
        t += 1
    u = ob.sqrt_fp((P - 1 - t) * RP % P)
    assert u * u * RINV % P == P - 1 - t and t < 64
    cases = []
    for uu in (u, P - u, u + P):
        for am in (1, 2, 3):
            for ia in (0b111111, 0b010101, 0b101010, 0b001111, 0b111100):
                a = _masked(uu, am, ia)
                cases.append((a, a))
    roles = sqr_roles()
    sums = _exact_sums(fc, roles, cases)
    flat = [s for acc in sums for pair in acc for s in pair]
    assert all(0 <= s + 240 * P < 434 * P for s in flat)
    got = _wg(dc, WG_SQR, 0, [c[0] for c in cases], [c[0] for c in cases])
    want = [r_sqr(_plain(a)) for a, _ in cases]
    for acc, w in zip(sums, want):
        assert [(s[0] * RINV % P, s[1] * RINV % P) for s in acc] == w
    _check_2p(got, want, "w_sqr extremes")
    print(f"w_sqr lane sums reach {max(flat) / P:.3f} p and {min(flat) / P:.3f} p (t = {t})")
    assert max(flat) >= 90 * P and min(flat) <= -44 * P


# ------------------------------------------------------------------ (d) the single-wave operations
@pytest.fixture(scope="module")
def lane_operands():
    """Canonical operand pairs (this kernel works fully reduced): edge and sparse cases interleaved
    with random ones so that at S = 4 the two groups of a wave hold (edge, random), then
    (random, edge) -- leakage between the groups through DPP or LDS would show."""
    rng = random.Random(0x1A9E5)
    ea, eb = _dense(rng, EDGE, 64), _dense(rng, EDGE, 64)
    sa, sb = _sparse_pairs(random.Random(0x5B))
    ea += [[(c0 % P, c1 % P) for c0, c1 in a] for a in sa]
    eb += [[(c0 % P, c1 % P) for c0, c1 in b] for b in sb]
    ea += [[(v, v)] * 6 for v in (0, P - 1, 1, RP)]
    eb += [[(v, v)] * 6 for v in (P - 1, P - 1, 0, RP)]
    A, B = [], []
    for i, (a, b) in enumerate(zip(ea, eb)):
        ra, rb = _raw(_rand12(rng)), _raw(_rand12(rng))
        A += [a, ra] if i % 2 == 0 else [ra, a]
        B += [b, rb] if i % 2 == 0 else [rb, b]
    return A, B


def _lines(n):
    """line coefficients (l0, l1, l3) from the edge set; every fourth the neutral line 1 (identity points)"""
    rng = random.Random(0x11E)
    L = []
    for i in range(n):
        if i % 4 == 3:
            L.append([(RP, 0), (0, 0), (0, 0)])
        else:
            L.append([(rng.choice(EDGE), rng.choice(EDGE)) for _ in range(3)])
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 8])
def test_lanes_products(gpu, dc, lane_operands, S):
    """g_mul, g_msq (g_sqr at S = 4, the half-product g_sqr_h at S = 8), g_mline (g_line / g_line_h),
    g_mul_lds"""
    A, B = lane_operands
    pa, pb = [_plain(a) for a in A], [_plain(b) for b in B]
    want_mul = [r_mul(a, b) for a, b in zip(pa, pb)]
    _check_canonical(_lanes(dc, S, LN_MUL, A, B), want_mul, f"g_mul S={S}")
    _check_canonical(_lanes(dc, S, LN_MUL_LDS, A, B), want_mul, f"g_mul_lds S={S}")
    _check_canonical(_lanes(dc, S, LN_MSQ, A), [r_sqr(a) for a in pa], f"g_msq S={S}")
    _check_canonical(_lanes(dc, S, LN_MSQ, B), [r_sqr(b) for b in pb], f"g_msq S={S} (b)")
    L = _lines(len(A))
    want = [r_line(a, *_plain(l)) for a, l in zip(pa, L)]
    _check_canonical(_lanes(dc, S, LN_MLINE, A, A, L), want, f"g_mline S={S}")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 8])
def test_lanes_frob_conj(gpu, dc, lane_operands, S):
    A, _ = lane_operands
    pa = [_plain(a) for a in A]
    for n, op in ((1, LN_FROB1), (2, LN_FROB2), (3, LN_FROB3)):
        _check_canonical(_lanes(dc, S, op, A), [r_frob(a, n) for a in pa], f"g_frob n={n} S={S}")
    _check_canonical(_lanes(dc, S, LN_CONJ, A), [r_conj(a) for a in pa], f"g_conj S={S}")


def _cyclotomic(f):
    """f^((p^6 - 1)(p^2 + 1)): conj(f) / f, then frob^2(.) * (.)"""
    g = r_mul(r_conj(f), r_inv(f))
    return r_mul(r_frob(g, 2), g)


@pytest.fixture(scope="module")
def cyclotomic_elements():
    rng = random.Random(0xC7C)
    src = [_rand12(rng) for _ in range(6)] + [_plain(a) for a in _dense(rng, EDGE[1:], 2)]
    out = [_cyclotomic(f) for f in src]
    for h in out:
        assert r_mul(h, r_conj(h)) == ONE12  # the conjugate is the inverse here
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 8])
def test_lanes_inv(gpu, dc, lane_operands, cyclotomic_elements, S):
    """f g_inv(f) = 1 on every operand of non-zero norm (Fq12 is a field: f != 0), and on elements
    of the cyclotomic subgroup."""
    A, _ = lane_operands
    A = [a for a in A if any(c != (0, 0) for c in a)]
    A = A[:len(A) & ~1] + [_raw(h) for h in cyclotomic_elements]
    got = _lanes(dc, S, LN_INV, A)
    for c, (a, g) in enumerate(zip(A, got)):
        assert all(max(pair) < P for pair in g), c
        assert r_mul(_plain(a), _plain(g)) == ONE12, f"g_inv S={S} case {c}"


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 8])
def test_lanes_pow_x(gpu, dc, cyclotomic_elements, S):
    """g_pow_x against pow(., BN_X) -- on cyclotomic-subgroup elements only: its negative NAF digits
    multiply by the conjugate, which is the inverse only there."""
    A = [_raw(h) for h in cyclotomic_elements]
    want = [r_pow(h, BN_X) for h in cyclotomic_elements]
    _check_canonical(_lanes(dc, S, LN_POW_X, A), want, f"g_pow_x S={S}")


@pytest.mark.gpu
def test_prologue_conv6(gpu, dc, lane_operands):
    A, B = lane_operands
    a, b = _pack(A), _pack(B)
    out = np.zeros_like(a)
    rc = dc.dc_prologue(PR_CONV6, a.ctypes.data, b.ctypes.data, out.ctypes.data, len(A))
    assert rc == 0, f"dc_prologue hip error {rc}"
    _check_canonical(_unpack(out), [r_mul(_plain(x), _plain(y)) for x, y in zip(A, B)], "conv6")


@pytest.mark.gpu
def test_prologue_merge_products_pair(gpu, dc):
    """merge_products and merge_products_wide on the same 5-sparse pair products D: both equal the
    reference product of the two pairs of every merged step (the step table itself, c_merge, is
    read from the harness; the end-to-end decider tests cover it)."""
    lines, nm, max_merge = dc.dc_info(0), dc.dc_info(1), dc.dc_info(2)
    first = [dc.dc_info(16 + m) for m in range(nm)]
    assert 0 < nm <= max_merge and all(0 <= f and f + 1 < lines for f in first)
    rng = random.Random(0x3E6)
    cases = []
    for c in range(3):
        pool = EDGE if c == 0 else [rng.randrange(P) for _ in range(64)]
        cases.append([(rng.choice(pool), rng.choice(pool)) if k % 6 != 5 else (0, 0) for k in range(lines * 6)])
    d = _pack(cases)
    outs = []
    for op in (PR_MERGE, PR_MERGE_WIDE):
        out = np.zeros((len(cases), max_merge * 6, 2, 8), np.uint32)
        rc = dc.dc_prologue(op, d.ctypes.data, None, out.ctypes.data, len(cases))
        assert rc == 0, f"dc_prologue hip error {rc}"
        outs.append(_unpack(out))
    assert outs[0] == outs[1]
    for case, got in zip(cases, outs[0]):
        for m, f in enumerate(first):
            da, db = _plain(case[6 * f:6 * f + 6]), _plain(case[6 * f + 6:6 * f + 12])
            assert got[6 * m:6 * m + 6] == _raw(r_mul(da, db)), m
        assert all(g == (0, 0) for g in got[6 * nm:])


@pytest.mark.gpu
def test_harness_rejects_malformed_calls(gpu, dc):
    buf = np.zeros((4, 6, 2, 8), np.uint32)
    p = buf.ctypes.data
    assert dc.dc_wg(5, 0, p, p, p, 1) == HIP_INVALID           # no such op
    assert dc.dc_wg(WG_MUL, 4, p, p, p, 1) == HIP_INVALID      # conj flags are 0-3
    assert dc.dc_wg(WG_FROB, 0, p, p, p, 1) == HIP_INVALID     # n = 1..3
    assert dc.dc_wg(WG_MUL, 0, p, p, p, (1 << 16) + 1) == HIP_INVALID
    assert dc.dc_norm24(2, p, p, 1) == HIP_INVALID
    assert dc.dc_lanes(2, LN_MUL, p, p, p, p, 2) == HIP_INVALID  # S is 4 or 8
    assert dc.dc_lanes(4, LN_MUL, p, p, p, p, 3) == HIP_INVALID  # whole waves only at S = 4
    assert dc.dc_lanes(8, 10, p, p, p, p, 1) == HIP_INVALID
    assert dc.dc_prologue(3, p, p, p, 1) == HIP_INVALID
    assert dc.dc_wg(WG_MUL, 0, p, p, p, 0) == 0
