"""Case tables of the codec edge suite (not collected by pytest): tests/test_codec_cases.py checks
the tables against the oracle on the CPU, tests/test_gpu_codec_edges.py runs them through
csrc/codec.hip.  Nothing here imports the library.

Every expected value is the oracle's (oracle/bn254.py: g1_decompress, g1_evm_decode,
accumulator_from_limbs, fe_to_limbs, eip197_input); the Montgomery forms are Python integers
(`v * 2**256 % P` for a coordinate, `% R` for a limb).  Curve points are made from an x by one
square root (sqrt_fp), never by a scalar multiplication, so every table builds in well under a
second.  Deterministic: fixed seeds.

A decoder case is Case(name, data, want): the encoded bytes and the point (x, y), None for the
identity, or INVALID.  A limb case is LimbCase(name, kind, limbs, raw, want): 4 * n_limbs canonical
integers, the indices of the limbs that are written into the array as they stand in BOTH forms (a
raw word equal to r: no Fr element, so no Montgomery form of it exists), and (lhs, rhs) or INVALID.
"""
import random
from collections import namedtuple

from oracle import bn254 as b

P, R = b.P, b.R
INVALID = "INVALID"
CANONICAL, MONTGOMERY = 0, 1
MONT = 1 << 256

Case = namedtuple("Case", "name data want")
Layout = namedtuple("Layout", "name rows first_invalid")
LimbCase = namedtuple("LimbCase", "name kind limbs raw want")
Eip197Case = namedtuple("Eip197Case", "name records invalid first_fail arg_error")


def mont_p(v):
    return v * MONT % P


def mont_r(v):
    return v * MONT % R


def point_row(want, form):
    """The (x, y) integers of an output row: the identity and an invalid entry are (0, 0) in both
    forms."""
    if want is None or want == INVALID:
        return (0, 0)
    return (mont_p(want[0]), mont_p(want[1])) if form == MONTGOMERY else tuple(want)


def y_of(x):
    return b.sqrt_fp((x * x * x + b.B) % P)


def curve_points(k, seed, below=P):
    """k points (x, sqrt(x^3 + 3)) from random x; with below = R both coordinates are < r (y or
    p - y, whichever is)."""
    rng = random.Random(seed)
    out = []
    while len(out) < k:
        x = rng.randrange(1, below)
        y = y_of(x)
        if y is None:
            continue
        if y >= below:
            y = P - y
        out.append((x, y))
    return out


# ---------------------------------------------------------------- the two point decoders
N_GENERATED = 64
POINTS = curve_points(N_GENERATED, 0xC0DEC)
NON_RESIDUE_X = next(x for x in range(1, 100) if y_of(x) is None)   # the smallest x off the curve
_Y_PM1 = y_of(P - 1)                                                # (p - 1)^3 + 3 = 2


def _le(v, sign=0):
    raw = bytearray(int(v).to_bytes(32, "little"))
    raw[31] |= sign << 7
    return bytes(raw)


def _be(x, y):
    return int(x).to_bytes(32, "big") + int(y).to_bytes(32, "big")


def _valid_points():
    pts = []
    for i, p in enumerate(POINTS):
        pts += [(f"gen{i}", p), (f"gen{i}-neg", b.g1_neg(p))]
    pts += [("g1", (1, 2)), ("g1-neg", (1, P - 2))]
    for sign in (0, 1):   # x = p - 1 is on the curve: both signs decode, to y and to p - y
        y = _Y_PM1 if _Y_PM1 & 1 == sign else P - _Y_PM1
        pts.append((f"x=p-1,sign={sign}", (P - 1, y)))
    pts.append(("identity", None))
    return pts


VALID_POINTS = _valid_points()

COMPRESSED_VALID = [Case(name, b.g1_compress(p), p) for name, p in VALID_POINTS]
COMPRESSED_INVALID = [
    Case("x=0,sign=1", _le(0, 1), INVALID),                     # 3 is a non-residue
    Case("x=p", _le(P), INVALID),
    Case("x=p,sign=1", _le(P, 1), INVALID),
    Case("x=p+1", _le(P + 1), INVALID),
    Case("ff*31,7f", b"\xff" * 31 + b"\x7f", INVALID),          # the low 255 bits all ones, sign 0
    Case("ff*32", b"\xff" * 32, INVALID),
    Case("non-residue", _le(NON_RESIDUE_X), INVALID),
    Case("non-residue,sign=1", _le(NON_RESIDUE_X, 1), INVALID),
]

_EX, _EY = POINTS[0]
EVM_VALID = [Case(name, b.g1_evm_encode(p), p) for name, p in VALID_POINTS]
EVM_INVALID = [
    Case("(p,2)", _be(P, 2), INVALID),
    Case("(1,p)", _be(1, P), INVALID),
    Case("(x+p,y)", _be(_EX + P, _EY), INVALID),                # the same residues, not canonical
    Case("(x,y+p)", _be(_EX, _EY + P), INVALID),
    Case("(x,y^1)", _be(_EX, _EY ^ 1), INVALID),
    Case("(0,1)", _be(0, 1), INVALID),
    Case("(x,0)", _be(_EX, 0), INVALID),
    Case("ff*64", b"\xff" * 64, INVALID),
]

LAYOUT_SIZES = (1, 255, 256, 257, 769)   # one block of 256 less one, exact, plus one; three blocks plus one
MIXED_AT = (700, 256, 255)               # three invalid entries in three blocks: the lowest is reported


def layouts(valid, invalid):
    """Every size with no invalid entry, one at index 0 and one at the last index; at 769 also the
    three of MIXED_AT together.  The rows walk through `valid` and the invalid entries through
    `invalid`, so every case of both tables is in some layout (test_codec_cases.py asserts it)."""
    out, v, k = [], 0, 0
    for n in LAYOUT_SIZES:
        places = [("clean", ()), ("first", (0,))]
        if n > 1:
            places.append(("last", (n - 1,)))
        if n == 769:
            places.append(("mixed", MIXED_AT))
        for pname, bad in places:
            rows = [valid[(v + i) % len(valid)] for i in range(n)]
            v += n
            for i in bad:
                rows[i] = invalid[k % len(invalid)]
                k += 1
            out.append(Layout(f"{n}-{pname}", rows, min(bad) if bad else -1))
    return out


def device_layout(valid, invalid):
    """The 257-entry mixed layout of the device-entry runs: an invalid entry in each block."""
    rows = [valid[(11 + i) % len(valid)] for i in range(257)]
    rows[3], rows[100], rows[256] = invalid[4], invalid[0], invalid[6]
    return Layout("257-mixed-device", rows, 3)


COMPRESSED_LAYOUTS = layouts(COMPRESSED_VALID, COMPRESSED_INVALID)
EVM_LAYOUTS = layouts(EVM_VALID, EVM_INVALID)
COMPRESSED_DEVICE_LAYOUT = device_layout(COMPRESSED_VALID, COMPRESSED_INVALID)
EVM_DEVICE_LAYOUT = device_layout(EVM_VALID, EVM_INVALID)


# ---------------------------------------------------------------- accumulators from limbs
# (n_limbs, bits).  (4, 64): sb == 0 at sw = 2, 4, 6; (8, 32): sb == 0 at every sw; (9, 29): another
# sb for each limb; (2, 255): the largest shift the argument rule admits (sw = 7, sb = 31);
# (1, 256): one limb, which is an Fr element, so its points have coordinates < r; (256, 1): 256
# one-bit limbs, four random accumulators.
GEOMETRIES = [(3, 88), (4, 68), (4, 64), (8, 32), (2, 128), (9, 29), (2, 255), (1, 256), (256, 1)]
PLUS_2_256 = [(3, 88), (4, 64), (2, 255)]   # the geometries of the plus-2^256 cases
BAD_GEOMETRIES = [(0, 88), (3, 0), (1, 257), (3, 128), (2, 256)]
N_RANDOM = 40
LIMB_POOL = curve_points(2 * N_RANDOM, 0x11B5, below=R)   # every coordinate < r: usable in every geometry


def to_limbs(v, n_limbs, bits):
    """fe_to_limbs with everything above the last limb's position left in it (a sum >= 2^256 has
    to fit), or None where a limb would not be an Fr element."""
    ls = b.fe_to_limbs(v, n_limbs, bits)
    ls[-1] = v >> (bits * (n_limbs - 1))
    return ls if all(l < R for l in ls) else None


def _acc_limbs(coords, n_limbs, bits):
    """The 4 * n_limbs limbs of four coordinate values (each an integer or a ready limb list)."""
    out = []
    for c in coords:
        ls = c if isinstance(c, list) else to_limbs(c, n_limbs, bits)
        if ls is None:
            return None
        out += ls
    return out


def _coords(acc):
    (l, r) = acc
    l, r = l or (0, 0), r or (0, 0)
    return [l[0], l[1], r[0], r[1]]


def _raw_r_point(n_limbs, bits, rng):
    """A curve point whose x is r + (t << bits): its limbs (r, t, 0, ..) sum to a canonical on-curve
    x, so the only thing wrong with them is that the first is no Fr element.  None where too few
    such x lie below p (p - r is a little above 2^126)."""
    if n_limbs < 2 or bits > 120:
        return None
    while True:
        t = rng.randrange(1, 1 << (126 - bits))
        x = R + (t << bits)
        y = y_of(x)
        if y is not None and x < P:
            return [R, t] + [0] * (n_limbs - 2), (x, y)


def limb_cases(n_limbs, bits):
    """The cases of one geometry, in a fixed order: N_RANDOM random accumulators (four for 256
    limbs), (None, None), (G1, None), the overlapping-limb accumulators, then each invalid kind in
    lhs and in rhs."""
    rng = random.Random(1000 * n_limbs + bits)
    n_random = 4 if n_limbs == 256 else N_RANDOM
    accs = [(LIMB_POOL[2 * i], LIMB_POOL[2 * i + 1]) for i in range(n_random)]
    cases = [LimbCase(f"random{i}", "valid", _acc_limbs(_coords(a), n_limbs, bits), (), a) for i, a in enumerate(accs)]
    cases.append(LimbCase("(None,None)", "valid", [0] * (4 * n_limbs), (), (None, None)))
    cases.append(LimbCase("(G1,None)", "valid", _acc_limbs([1, 2, 0, 0], n_limbs, bits), (), (b.G1_GEN, None)))
    # overlapping limbs that carry across words: l1 = 2^k - 1 reaches far above its `bits`, l0 takes the rest
    if n_limbs >= 2:
        (x, y), rhs = accs[1]
        for k in (bits + 1, bits + 7, bits + 31, bits + 32, bits + 33, bits + 64, x.bit_length() - 1 - bits):
            if k <= bits:
                continue
            l1 = (1 << k) - 1
            l0 = x - (l1 << bits)
            if l1 < R and 0 <= l0 < R:
                cases.append(LimbCase(f"overlap-k{k}", "valid",
                                      _acc_limbs([[l0, l1] + [0] * (n_limbs - 2), y, rhs[0], rhs[1]], n_limbs, bits),
                                      (), accs[1]))
    good = accs[2]
    x, y = accs[3][0]
    bad_points = [("sum=p", (P, y)), ("sum=x+p", (x + P, y)), ("y=y+p", (x, y + P)), ("off-curve", (x, y ^ 1)),
                  ("(x,0)", (x, 0)), ("(0,y)", (0, y))]
    if (n_limbs, bits) in PLUS_2_256:   # the low 256 bits are the on-curve x: only words 8.. tell
        bad_points.append(("sum=x+2^256", (x + MONT, y)))
        bad_points.append(("y=y+2^256", (x, y + MONT)))
    for side in (0, 1):
        tag = "rhs" if side else "lhs"
        for name, pt_ in bad_points:
            coords = _coords(good)
            coords[2 * side], coords[2 * side + 1] = pt_
            limbs = _acc_limbs(coords, n_limbs, bits)
            if limbs is not None:   # None: a limb would be >= r, so the geometry cannot say it
                cases.append(LimbCase(f"{name}-{tag}", "invalid", limbs, (), INVALID))
        # a raw limb equal to r
        coords = _coords(good)
        trick = _raw_r_point(n_limbs, bits, rng)
        if trick is not None:
            coords[2 * side], coords[2 * side + 1] = trick[0], trick[1][1]
        limbs = _acc_limbs(coords, n_limbs, bits)
        at = 2 * side * n_limbs
        limbs[at] = R
        cases.append(LimbCase(f"raw-r-{tag}", "raw", limbs, (at,), INVALID))
    return cases


LIMB_CASES = {g: limb_cases(*g) for g in GEOMETRIES}

# batches of the (n_limbs, bits) != (256, 1) geometries: n accumulators, invalid ones at `bad`.
# 128 accumulators are 256 points, exactly one block; accumulator 128 is alone in a second block.
LIMB_BATCHES = [(1, ()), (1, (0,)), (128, ()), (128, (127, 64, 5)), (129, (128,)), (129, (128, 127, 40))]


def limb_batch(cases, n, bad, turn=0):
    """n accumulators walking through the valid cases, the invalid ones (walking through the invalid
    and raw cases from `turn`) at the indices `bad` -> (rows, first_invalid)."""
    valid = [c for c in cases if c.kind == "valid"]
    invalid = [c for c in cases if c.kind != "valid"]
    rows = [valid[(turn + i) % len(valid)] for i in range(n)]
    for j, i in enumerate(bad):
        rows[i] = invalid[(turn + j) % len(invalid)]
    return rows, (min(bad) if bad else -1)


# ---------------------------------------------------------------- EIP-197 records
REC = 0x180


def _case(golden, name):
    from conftest import pt, q2
    c = next(c for c in golden["cases"] if c["name"] == name)
    return q2(c["g2"]), q2(c["s_g2"]), [pt(v) for v in c["lhs"]], [pt(v) for v in c["rhs"]], c["first_fail"]


def _add_p(rec, word_at):
    """The 32-byte big-endian word at word_at plus p: the same residue, not canonical."""
    v = int.from_bytes(rec[word_at:word_at + 32], "big") + P
    assert v < MONT
    rec[word_at:word_at + 32] = v.to_bytes(32, "big")


def eip197_cases(golden):
    """Mutations of the golden decider cases (tests/golden/decider.json: key, accumulators and the
    known first_fail, so no pairing is computed here).  `invalid` lists the checks made invalid;
    first_fail is the lowest of the golden first_fail (if >= 0) and those."""
    out = []

    def add(name, base, edits=(), insert_identity_at=None, keep=None, g2_edit=None):
        g2, sg2, lhs, rhs, ff = _case(golden, base)
        lhs, rhs = list(lhs), list(rhs)
        if insert_identity_at is not None:
            assert ff < 0
            lhs.insert(insert_identity_at, None)
            rhs.insert(insert_identity_at, None)
        if keep is not None:
            lhs, rhs = lhs[:keep], rhs[:keep]
            ff = ff if ff < keep else -1
        recs = [bytearray(b.eip197_input(g2, sg2, l, r)) for l, r in zip(lhs, rhs)]
        assert 1 <= len(recs) <= 8
        for check, side, how in edits:
            at = 192 * side          # lhs at 0, rhs at 192: x then y
            if how == "off-curve":
                recs[check][at + 63] ^= 1
            elif how == "x+p":
                _add_p(recs[check], at)
            elif how == "y+p":
                _add_p(recs[check], at + 32)
            elif how == "y=0":
                recs[check][at + 32:at + 64] = bytes(32)
        if g2_edit is not None:       # in every record, so that only the range check can object
            for rec in recs:
                _add_p(rec, g2_edit)
        invalid = sorted({e[0] for e in edits})
        want = min([ff] * (ff >= 0) + invalid, default=-1)
        out.append(Eip197Case(name, b"".join(bytes(r) for r in recs), invalid, want, g2_edit is not None))

    add("lhs-off-curve-alone", "all_valid", [(1, 0, "off-curve")])
    add("rhs-off-curve-alone-last", "all_valid", [(3, 1, "off-curve")])
    add("lhs.x+p", "all_valid", [(2, 0, "x+p")])
    add("rhs.y+p", "all_valid", [(0, 1, "y+p")])
    add("lhs.y=0", "all_valid", [(3, 0, "y=0")])
    add("invalid-above-the-failing-check", "six_valid_one_bad_plus_identity", [(5, 1, "off-curve")])
    add("invalid-below-the-failing-check", "six_valid_one_bad_plus_identity", [(1, 0, "x+p")])
    add("invalid-at-the-failing-check", "six_valid_one_bad_plus_identity", [(3, 0, "off-curve")])
    add("invalid-lhs-2-rhs-1", "all_valid", [(2, 0, "off-curve"), (1, 1, "off-curve")])
    add("invalid-lhs-1-rhs-3", "all_valid", [(1, 0, "y+p"), (3, 1, "off-curve")])
    add("invalid-lhs-and-rhs-of-one-check", "all_valid", [(2, 0, "off-curve"), (2, 1, "x+p")])
    add("identity-record-inserted", "all_valid", insert_identity_at=2)
    add("identity-record-first", "all_valid", insert_identity_at=0)
    add("g2-word>=p", "all_valid", g2_edit=64)              # g2: x.c1
    add("g2-y-word>=p", "all_valid", g2_edit=64 + 96)       # g2: y.c0
    add("minus-s_g2-word>=p", "all_valid", g2_edit=256 + 32)  # -s_g2: x.c0
    add("one-check-passing", "all_valid", keep=1)
    add("one-check-failing", "first_bad", keep=1)
    add("one-check-invalid", "all_valid", [(0, 1, "off-curve")], keep=1)
    add("one-check-identity", "all_valid", insert_identity_at=0, keep=1)
    return out
