"""Cases and checks for csrc/field29.hpp and csrc/curve29.hpp, shared by the host run
(tests/test_field29.py through tests/native/field29check.cpp) and the device run
(tests/test_gpu_field29.py through tests/native/field29dev.hip).  Both builds are judged against
Python integers and the oracle's affine group law (oracle/bn254.py), never against each other.

Deterministic (fixed seeds).  Every case lies inside its operation's contract by construction: the
checkers skip nothing and assert that they checked every case.  An operand below a bound B = K *
modulus is drawn from 0, 1, modulus - 1, modulus, modulus + 1, B - 1, the worst-limb value (low
eight limbs all 0x1fffffff, top limb one below B - 1's), powers of two, and uniform values below B;
every operation also gets the tuples with all operands at B - 1 and all at the worst-limb value.

A case travels as slots of 9 u32 (tests/native/f29_ops.hpp): 9 x 29-bit limbs, or 8 x 32-bit words
and a zero where the operation takes or gives words; plus one flag word in (the sign) and out.
"""
import random
import zlib

from oracle import bn254 as ob

MASK = (1 << 29) - 1
MODULI = {"fq": ob.P, "fr": ob.R}
FIELD_ID = {"fq": 0, "fr": 1}
N_FIELD = 2048  # cases per field operation (at least 2,000)
N_KIND = 208    # cases per kind of curve case (at least 200)


# ---------------------------------------------------------------- slots
def enc_limbs(v):
    assert 0 <= v < 1 << 261
    return [(v >> (29 * i)) & MASK for i in range(9)]


def enc_words(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]


def dec_limbs(s):
    """A result must be normalized: every limb below 2^29."""
    assert len(s) == 9 and all(0 <= x <= MASK for x in s), s
    return sum(int(x) << (29 * i) for i, x in enumerate(s))


def dec_words(s):
    assert len(s) == 9 and s[8] == 0 and all(0 <= x <= 0xFFFFFFFF for x in s), s
    return sum(int(x) << (32 * i) for i, x in enumerate(s[:8]))


# ---------------------------------------------------------------- operand values
def worst_limb(B):
    """Low eight limbs all ones, the top limb one below B - 1's: every column of a product at its
    largest, still below B."""
    top = ((B - 1) >> 232) - 1
    return None if top < 0 else (top << 232) | ((1 << 232) - 1)


def named(B, m):
    """The seven named values of a slot, in a fixed order (so that index j of every slot is the
    same kind); one that does not lie below B is replaced by B - 1."""
    vals = [0, 1, m - 1, m, m + 1, B - 1, worst_limb(B)]
    return [v if v is not None and 0 <= v < B else B - 1 for v in vals]


def edge_pool(B, m):
    vals = named(B, m)
    vals += [1 << k for k in range(0, 261, 7)] + [(1 << k) - 1 for k in range(29, 262, 29)]
    vals += [k * m + d for k in range(2, 24) for d in (-1, 0, 1)]
    return sorted({v for v in vals if 0 <= v < B})


def tuples(bounds, m, rng, n=N_FIELD):
    """n operand tuples for slots with the given bounds."""
    k = len(bounds)
    nm = [named(B, m) for B in bounds]
    pools = [edge_pool(B, m) for B in bounds]
    out = [tuple(nm[s][j] for s in range(k)) for j in range(7)]  # all at B - 1, all worst-limb, ...
    if k <= 2:
        out += [tuple(nm[s][(j // 7 ** s) % 7] for s in range(k)) for j in range(7 ** k)]
    else:
        for rest in (5, 6):  # one slot through every named value, the others at B - 1 / worst-limb
            out += [tuple(nm[t][j if t == s else rest] for t in range(k)) for s in range(k) for j in range(7)]
    out += [tuple(rng.choice(pools[s]) for s in range(k)) for _ in range(600)]
    out += [tuple(rng.choice(pools[s]) if rng.random() < 0.5 else rng.randrange(bounds[s]) for s in range(k))
            for _ in range(300)]
    while len(out) < n:
        out.append(tuple(rng.randrange(B) for B in bounds))
    return out


# ---------------------------------------------------------------- field operations
class FieldOp:
    """id: f29_ops.hpp's number.  bounds(m): the input bound of every slot.  check(m, rinv, ins,
    flag, r, flag_out): asserts the value and the stated output bound of one case."""

    def __init__(self, id, bounds, check, words_in=False, words_out=False, fields=("fq", "fr"), gen=None):
        self.id, self.bounds, self.check = id, bounds, check
        self.words_in, self.words_out, self.fields, self.gen = words_in, words_out, fields, gen


def _mont(out_k, want):
    """A Montgomery product form: the result is below out_k * modulus and equals want / R'."""
    def check(m, rinv, a, flag, r, fo):
        assert r < out_k * m and r % m == want(*a) * rinv % m
    return check


def _chk_mul_sub8(m, rinv, a, flag, r, fo):
    assert r < 10 * m and r % m == (a[0] * a[1] * rinv - a[2]) % m


def _chk_sqr_sub2c6(m, rinv, a, flag, r, fo):
    assert 0 < r < 8 * m and r % m == (a[0] * a[0] * rinv - a[1] - 2 * a[2]) % m


def _exact(want):
    def check(m, rinv, a, flag, r, fo):
        w = want(m, *a)
        assert 0 <= w < 1 << 261 and r == w
    return check


def _chk_sub_sgn4(m, rinv, a, flag, r, fo):
    w = (-a[0] if flag & 1 else a[0]) + 4 * m - a[1]
    assert 0 <= w < 1 << 261 and r == w


def _chk_csub(k):
    def check(m, rinv, a, flag, r, fo):
        assert a[0] < 2 * k * m and r < k * m and r == (a[0] if a[0] < k * m else a[0] - k * m)
    return check


def _chk_to_r29(m, rinv, a, flag, r, fo):
    assert a[0] < m and r < 2 * m and r % m == 32 * a[0] % m


def _chk_to_r32(m, rinv, a, flag, r, fo):
    assert a[0] < 4 * m and r < m and r == a[0] * pow(32, -1, m) % m


def _chk_is_zero16(m, rinv, a, flag, r, fo):
    assert a[0] < 16 * m and fo == (1 if a[0] % m == 0 else 0)


def _gen_sub_sgn4(m, rng):
    """(a, b, neg).  +a + 4p - b: a below 12p, b below 4p.  -a + 4p - b must not go negative:
    a below 4p + 1 and b up to 4p - a, the value 0 included."""
    cases = [(a, b, 0) for a, b in tuples([12 * m, 4 * m], m, rng, N_FIELD // 2)]
    pool_a = edge_pool(4 * m + 1, m)
    neg = []
    for a in pool_a:
        nb = named(4 * m - a + 1, m)
        neg += [(a, b, 1) for b in nb]
    while len(neg) < N_FIELD // 2 + 200:
        a = rng.choice(pool_a) if rng.random() < 0.3 else rng.randrange(4 * m + 1)
        Bb = 4 * m - a + 1
        b = rng.choice(edge_pool(Bb, m)) if rng.random() < 0.3 else rng.randrange(Bb)
        neg.append((a, b, 1))
    return cases + neg


def _gen_is_zero16(m, rng):
    """Every multiple k p below 16p, its neighbours at +-1 and at +-2^232 (limb 0 unchanged, the
    top limb moves), values whose limb 0 is that of a multiple (their own rounded k's: the full
    comparison runs and must say no; another j's), top limbs at the rounding's half-way points, and
    uniform values below 16p."""
    B = 16 * m
    ptop = m / (1 << 232)
    v = []
    for k in range(16):
        v += [k * m, k * m + 1, k * m - 1, k * m + (1 << 232), k * m - (1 << 232), k * m + (1 << 29), k * m - (1 << 29),
              k * m + (1 << 231), k * m - (1 << 231)]
        half = int((k + 0.5) * ptop)
        for top in (half - 1, half, half + 1):  # k's and k + 1's limb 0 under a half-way top limb
            for j in (k, k + 1):
                v.append((top << 232) | (rng.getrandbits(203) << 29) | ((j * m) & MASK))
    for _ in range(400):
        a = rng.randrange(B)
        k = int((a >> 232) / ptop + 0.5)
        j = k if rng.random() < 0.5 else rng.randrange(16)
        v.append((a & ~MASK) | ((j * m) & MASK))
    for k in range(16):  # the whole of k p but one middle limb
        for i in range(1, 8):
            v.append(k * m ^ (1 << (29 * i + rng.randrange(29))))
    v = [a for a in v if 0 <= a < B]
    while len(v) < N_FIELD:
        v.append(rng.randrange(B))
    return [(a, 0) for a in v]


def _b(*ks):
    return lambda m: [k * m for k in ks]


OPS = {
    "mul": FieldOp(0, _b(12, 12), _mont(2, lambda a, b: a * b)),
    "mul_ilp": FieldOp(1, _b(12, 12), _mont(2, lambda a, b: a * b)),
    "sqr": FieldOp(2, _b(12), _mont(2, lambda a: a * a)),
    "mul_sum2": FieldOp(3, _b(9, 9, 9, 9), _mont(2, lambda a, b, c, d: a * b + c * d)),
    "mul_sum3": FieldOp(4, _b(9, 1, 9, 1, 9, 1), _mont(2, lambda a, b, c, d, e, f: a * b + c * d + e * f)),
    "mul_sub8": FieldOp(5, _b(12, 12, 8), _chk_mul_sub8),
    "sqr_sub2c6": FieldOp(6, _b(12, 2, 2), _chk_sqr_sub2c6),
    # add: bound(a) + bound(b) must stay below 2^261 = 169.6 p
    "add": FieldOp(7, _b(84, 84), _exact(lambda m, a, b: a + b)),
    "sub2": FieldOp(8, _b(12, 2), _exact(lambda m, a, b: a - b + 2 * m)),
    "sub4": FieldOp(9, _b(12, 4), _exact(lambda m, a, b: a - b + 4 * m)),
    "sub8": FieldOp(10, _b(12, 8), _exact(lambda m, a, b: a - b + 8 * m)),
    "sub_2c6": FieldOp(11, _b(12, 2, 2), _exact(lambda m, a, b, c: a + 6 * m - b - 2 * c)),
    "sub_sgn4": FieldOp(12, _b(12, 4), _chk_sub_sgn4, gen=_gen_sub_sgn4),
    "csub1": FieldOp(13, _b(2), _chk_csub(1)),
    "csub2": FieldOp(14, _b(4), _chk_csub(2)),
    "csub4": FieldOp(15, _b(8), _chk_csub(4)),
    "csub8": FieldOp(16, _b(16), _chk_csub(8)),
    "from_words": FieldOp(17, lambda m: [1 << 256], _exact(lambda m, a: a), words_in=True),
    "to_words": FieldOp(18, lambda m: [1 << 256], _exact(lambda m, a: a), words_out=True),
    "to_r29": FieldOp(19, _b(1), _chk_to_r29, words_in=True),
    "to_r32": FieldOp(20, _b(4), _chk_to_r32, words_out=True),
    "is_zero16": FieldOp(21, _b(16), _chk_is_zero16, fields=("fq",), gen=_gen_is_zero16),
}
FIELD_CASES = [(name, field) for name, op in OPS.items() for field in op.fields]


def _rng(*key):
    return random.Random(zlib.crc32(repr(key).encode()))


_cache = {}


def field_cases(name, field):
    """(operand tuples, flags) of one operation over one modulus; computed once."""
    if (name, field) not in _cache:
        op, m = OPS[name], MODULI[field]
        rng = _rng("f29", name, field)
        if op.gen is not None:
            rows = op.gen(m, rng)
            ins, flags = [r[:-1] for r in rows], [r[-1] for r in rows]
        else:
            ins = tuples(op.bounds(m), m, rng)
            flags = [0] * len(ins)
        assert len(ins) >= 2000
        _cache[name, field] = (ins, flags)
    return _cache[name, field]


def field_rows(name, field):
    """The cases as rows of u32 (n_in * 9 each) and their flags."""
    op = OPS[name]
    ins, flags = field_cases(name, field)
    enc = enc_words if op.words_in else enc_limbs
    return [[x for v in a for x in enc(v)] for a in ins], flags


def check_field(name, field, out_rows, out_flags):
    """out_rows: a row of 9 u32 per case.  Checks every case; returns how many."""
    op, m = OPS[name], MODULI[field]
    rinv = pow((1 << 261) % m, -1, m)
    ins, flags = field_cases(name, field)
    assert len(out_rows) == len(ins) == len(out_flags)
    dec = dec_words if op.words_out else dec_limbs
    bounds = op.bounds(m)
    checked = 0
    for a, fl, row, fo in zip(ins, flags, out_rows, out_flags):
        try:
            # inside the contract by construction (sub_sgn's depends on the sign: its check has it)
            assert op.gen is _gen_sub_sgn4 or all(0 <= v < B for v, B in zip(a, bounds)), "out of contract"
            op.check(m, rinv, a, fl, dec([int(x) for x in row]), int(fo))
        except AssertionError as e:
            raise AssertionError("%s/%s: inputs %s flag %d -> %s flag %d %s" % (
                name, field, [hex(v) for v in a], fl, [hex(int(x)) for x in row], fo, e)) from None
        checked += 1
    assert checked == len(ins)  # nothing skipped
    return checked


# ---------------------------------------------------------------- curve operations (Fq)
P = ob.P
RP = (1 << 261) % P  # R' = 2^261
RINV = pow(RP, -1, P)
CURVE_IDS = {"madd": 22, "maddl": 23, "xadd": 24, "xadd8": 25}
CURVE_CASES = [("madd", 0), ("madd", 1), ("maddl", 0), ("maddl", 1), ("xadd", 0), ("xadd8", 0)]  # (op, neg)

_points = []


def points():
    """A fixed pool of affine points (multiples of the generator by fixed random scalars)."""
    if not _points:
        rng = _rng("f29 points")
        _points.extend(ob.g1_mul(ob.G1_GEN, rng.randrange(1, ob.R)) for _ in range(40))
    return _points


def _rep(v, k):
    """v (a field element) in R' form plus k p."""
    return v * RP % P + k * P


def state(pt, rng, xk):
    """A random XYZZ representation of an affine point: random Z, X's representative plus xk p,
    the other coordinates plus 0 or p."""
    x, y = pt
    z = rng.randrange(1, P)
    zz, zzz = z * z % P, z * z * z % P
    return (_rep(x * zz % P, xk), _rep(y * zzz % P, rng.randrange(2)), _rep(zz, rng.randrange(2)),
            _rep(zzz, rng.randrange(2)))


def garbage_identity(rng, xmax):
    """ZZ == 0 and random nonzero other coordinates inside their bounds: still the identity."""
    return (rng.randrange(1, xmax * P), rng.randrange(1, 2 * P), 0, rng.randrange(1, 2 * P))


def to_affine(X, Y, ZZ, ZZZ):
    X, Y, ZZ, ZZZ = (v * RINV % P for v in (X, Y, ZZ, ZZZ))
    if ZZ == 0:
        return None
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def _pair(rng):
    a, b = rng.sample(points(), 2)
    return a, b


def madd_cases(neg):
    """state + (x2, neg ? -y2 : y2) for madd and for the loop's start / madd_live / dbl_start:
    (inputs, want, kind).  The state's X takes every representative up to x + 7p (below 8p)."""
    key = ("madd", neg)
    if key not in _cache:
        rng = _rng("f29 madd", neg)
        cases = []
        for kind in ("generic", "doubling", "cancel", "identity", "garbage-identity"):
            for n in range(N_KIND):
                a, b = _pair(rng)
                if kind == "doubling":
                    b = a
                elif kind == "cancel":
                    b = ob.g1_neg(a)
                if kind == "identity":
                    st, want = (0, 0, 0, 0), b
                elif kind == "garbage-identity":
                    st, want = garbage_identity(rng, 8), b
                else:
                    st, want = state(a, rng, n % 8), ob.g1_add(a, b)
                yv = ob.g1_neg(b)[1] if neg else b[1]  # the point handed over: -y2 is b's y under neg
                cases.append(((*st, _rep(b[0], rng.randrange(2)), _rep(yv, rng.randrange(2))), want, kind))
        _cache[key] = cases
    return _cache[key]


def xadd_cases():
    """r29::add and add_x8: both operands' X up to 8p - 1 (as k_accumulate hands chain states over)."""
    if "xadd" not in _cache:
        rng = _rng("f29 xadd")
        cases = []
        kinds = ("generic", "doubling", "doubling-same-rep", "cancel", "identity-a", "identity-b", "identity-both",
                 "garbage-a", "garbage-b", "garbage-both")
        for kind in kinds:
            for n in range(N_KIND):
                a, b = _pair(rng)
                if kind.startswith("doubling"):
                    b = a
                elif kind == "cancel":
                    b = ob.g1_neg(a)
                sa, sb = state(a, rng, n % 8), state(b, rng, (n // 8) % 8)
                if kind == "doubling-same-rep":
                    sb = sa
                zero = (0, 0, 0, 0)
                if kind in ("identity-a", "identity-both"):
                    sa, a = zero, None
                if kind in ("identity-b", "identity-both"):
                    sb, b = zero, None
                if kind in ("garbage-a", "garbage-both"):
                    sa, a = garbage_identity(rng, 8), None
                if kind in ("garbage-b", "garbage-both"):
                    sb, b = garbage_identity(rng, 8), None
                cases.append(((*sa, *sb), ob.g1_add(a, b), kind))
        _cache["xadd"] = cases
    return _cache["xadd"]


def curve_cases(name, neg):
    return xadd_cases() if name.startswith("xadd") else madd_cases(neg)


def curve_rows(name, neg):
    cases = curve_cases(name, neg)
    return [[x for v in ins for x in enc_limbs(v)] for ins, _, _ in cases], [neg] * len(cases)


def check_curve(name, neg, out_rows, out_flags):
    """out_rows: a row of 4 * 9 u32 per case (X, Y, ZZ, ZZZ).  Output bounds as curve29.hpp states
    them: X below 8p for the chain and add_x8, below 4p for add, the rest below 2p; an identity result has
    ZZ == 0 exactly (what every reader tests).  Returns how many cases it checked."""
    cases = curve_cases(name, neg)
    assert len(out_rows) == len(cases) == len(out_flags)
    xmax = 4 if name == "xadd" else 8
    kinds = {}
    for (ins, want, kind), row, fo in zip(cases, out_rows, out_flags):
        row = [int(x) for x in row]
        X, Y, ZZ, ZZZ = (dec_limbs(row[9 * c:9 * c + 9]) for c in range(4))
        ctx = "%s neg=%d %s: %s -> %s" % (name, neg, kind, [hex(v) for v in ins], [hex(v) for v in (X, Y, ZZ, ZZZ)])
        assert X < xmax * P and Y < 2 * P and ZZ < 2 * P and ZZZ < 2 * P, ctx
        got = to_affine(X, Y, ZZ, ZZZ)
        assert got == (None if want is None else tuple(want)), ctx
        if got is None:
            assert ZZ == 0, ctx
        if name.startswith("xadd") and kind in ("garbage-a", "identity-a", "garbage-b", "identity-b"):
            o = ins[4:] if kind.endswith("-a") else ins[:4]  # the other operand itself (add: X below 4p)
            assert (X, Y, ZZ, ZZZ) == (o[0] - 4 * P if name == "xadd" and o[0] >= 4 * P else o[0], *o[1:]), ctx
        if name == "maddl":  # madd_live's report, where it ran
            live = kind in ("generic", "doubling", "cancel")
            assert fo == ({"doubling": 2, "cancel": 1}.get(kind, 0) if live else 0), ctx
        kinds[kind] = kinds.get(kind, 0) + 1
    assert sum(kinds.values()) == len(cases) and all(v >= 200 for v in kinds.values()), kinds
    return len(cases)
