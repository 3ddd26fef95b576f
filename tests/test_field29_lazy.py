"""The bucket chain's redundant-limb differences (csrc/field29.hpp's sub_lazy) and the steps that
multiply them (csrc/curve29.hpp's madd_live / dbl_start), run on the host through
tests/native/field29lazy.cpp and checked with Python integers: limb ranges and exact values at the
stated bounds' edges, the fused product against an exact Montgomery reduction (also with every limb
at its maximum, the column accumulator's worst case), and the loop's step against the affine group
law.  The harness runs as built and again under ASan + UBSan.  CPU only."""
import os
import random
import subprocess

import pytest

from conftest import sanitizer_prefix
from oracle import bn254 as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc")
P = ob.P
RBIG = 1 << 261  # R'
RP = RBIG % P
RINV = pow(RP, -1, P)
NP29 = (-pow(P, -1, 1 << 29)) % (1 << 29)
RI29 = pow(1 << 29, -1, P)
M29 = (1 << 29) - 1
ALL = RBIG - 1  # every limb 2^29 - 1


@pytest.fixture(scope="module", params=["plain", "asan"])
def lazy(request):
    """The harness built with the host compiler, and again with AddressSanitizer + UBSan."""
    out = os.path.join(NATIVE, "build", "field29lazy" + ("_asan" if request.param == "asan" else ""))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
             if request.param == "asan" else ["-O2"])
    cmd = [os.environ.get("CXX", "g++"), *flags, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
           os.path.join(NATIVE, "field29lazy.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return (sanitizer_prefix() if request.param == "asan" else []) + [out]


def _run(lazy, mode, rows):
    inp = "".join(" ".join(("%x" % v if i or mode != "sublazy" else "%d" % v) for i, v in enumerate(r)) + "\n"
                  for r in rows)
    r = subprocess.run(lazy + [mode], input=inp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(rows)
    return out


def _raw(h):
    """9 raw limbs, least significant first."""
    assert len(h) == 72
    return [int(h[8 * (8 - i):8 * (8 - i) + 8], 16) for i in range(9)]


def _val(h):
    return sum(v << (29 * i) for i, v in enumerate(_raw(h)))


def _edge(rng, bound):
    """Values below `bound`: its edges, worst-limb patterns, random ones."""
    top = min(bound - 1, ALL)
    fixed = [0, 1, top, top - 1, bound // 2, top & ~M29, (top >> 29 << 29) - 1]
    # every lower limb at 2^29 - 1 / at zero under the largest top limb the bound allows
    t8 = (top >> 232) - 1
    fixed += [(t8 << 232) | ((1 << 232) - 1), t8 << 232]
    return [v for v in fixed if 0 <= v < bound] + [rng.randrange(bound) for _ in range(40)]


def test_sub_lazy_limbs_and_value(lazy):
    """a - b + K p exactly, every limb in its stated range, for b up to (K - 1/2) p - 1 and a up to
    every limb at 2^29 - 1; the two instances the chain uses (K = 8: Q - X3, K = 2: 0 - PPP)."""
    rng = random.Random(2901)
    rows = []
    for k in (2, 8):
        bs = _edge(rng, (2 * k - 1) * P // 2)
        for a in ([0] if k == 2 else []) + [ALL, 2 * P - 1, 0, 1] + [rng.randrange(2 * P) for _ in range(6)]:
            rows += [(k, a, b) for b in bs]
    for (k, a, b), line in zip(rows, _run(lazy, "sublazy", rows)):
        limbs = _raw(line)
        assert all(0 <= v < 3 << 29 for v in limbs[:8]), line
        assert limbs[8] < 1 << 30, line  # no wrap below zero: b's top limb stays below K p's
        if a == 0:
            assert all(v < 1 << 30 for v in limbs), line  # 2p - PPP: mul_sum2's b1 bound
        assert _val(line) == a - b + k * P, (k, a, b)
    assert len(rows) > 1000


def _redc(t):
    """field29.hpp's reduction, limb for limb: seven lazy steps (the low limb c leaves and
    c 2^-29 mod p enters one limb up), then two standard ones (m p clears the limb)."""
    v = t
    for k in range(9):
        c = (v >> (29 * k)) & M29
        if k < 7:
            v += (c * RI29 << (29 * (k + 1))) - (c << (29 * k))
        else:
            v += (c * NP29 & M29) * P << (29 * k)
    assert v % RBIG == 0 and v >> 261 < t // RBIG + P + (P >> 28) + 1  # below a b / R' + (1 + 2^-28) p
    return v >> 261


def test_mul_sum2_over_lazy_operands(lazy):
    """mul_sum2(a0, Q - X3 + 8p, a1, 2p - PPP) over redundant limbs equals the reduction's model
    over the same integer and the product over normalized differences, limb for limb; below
    2p inside the chain's bounds (a0 < 6p, Q < 2p, X3 < 7.5p, a1 < 2p, PPP < 1.5p).  Rows with every
    limb at its maximum (outside the value bounds) fill the 64-bit column accumulator as far as the
    limb ranges allow: a wrapped column would change the result."""
    rng = random.Random(2902)
    rows = [(ALL, ALL, 0, ALL, 0), (ALL, ALL, ALL, ALL, 0), (ALL, 2 * P - 1, 0, ALL, 3 * P // 2 - 1), (ALL, 0, 0, ALL, 0)]
    nfree = len(rows)
    e6, e2, ex, ep = _edge(rng, 6 * P), _edge(rng, 2 * P), _edge(rng, 15 * P // 2), _edge(rng, 3 * P // 2)
    rows += [(6 * P - 1, 2 * P - 1, 0, 2 * P - 1, 0), (6 * P - 1, 0, 15 * P // 2 - 1, 2 * P - 1, 3 * P // 2 - 1)]
    for _ in range(3000):
        rows.append(tuple(rng.choice(e) for e in (e6, e2, ex, e2, ep)))
    for n, ((a0, q, x3, a1, ppp), line) in enumerate(zip(rows, _run(lazy, "msum", rows))):
        got, ref = line.split()
        t = a0 * (q - x3 + 8 * P) + a1 * (2 * P - ppp)
        assert _val(got) == _redc(t), (a0, q, x3, a1, ppp)
        assert all(v <= M29 for v in _raw(got)[:8]), line
        if n >= nfree:
            assert _raw(got) == _raw(ref), line
            assert _val(got) < 2 * P and _val(got) % P == t * RINV % P, line


def test_products_match_the_reduction_model(lazy):
    """mul, sqr and the fused mul_sub over inputs up to 12p - 1 and with every limb at 2^29 - 1: the
    result is the model's, limb for limb, so it is a b / R' mod p and below a b / R' + (1 + 2^-28) p
    (_redc asserts that), which is below 2p inside the 12p input bound."""
    rng = random.Random(2904)
    e = _edge(rng, 12 * P)
    rows = [(ALL, ALL), (ALL, 0), (ALL, 1), (12 * P - 1, 12 * P - 1)] + [(rng.choice(e), rng.choice(e)) for _ in range(3000)]
    for n, ((x, y), line) in enumerate(zip(rows, _run(lazy, "prod", rows))):
        m, s, ms = line.split()
        assert _val(m) == _redc(x * y) and _val(s) == _redc(x * x), (x, y)
        if n >= 3:
            assert _val(m) < 2 * P and _val(s) < 2 * P and _val(m) % P == x * y * RINV % P, line
            assert _val(ms) == _val(m) + 8 * P, line  # the high columns' addend rides on the same reduction


def _state(pt, rng, kx, ky):
    """An XYZZ representation (R' form) of an affine point with X = x + kx p and Y = y + ky p."""
    z = rng.randrange(1, P)
    zz, zzz = z * z % P, z * z * z % P
    m = lambda v: v * RP % P  # noqa: E731
    return (m(pt[0] * zz % P) + kx * P, m(pt[1] * zzz % P) + ky * P, m(zz) + rng.randrange(2) * P,
            m(zzz) + rng.randrange(2) * P)


def _affine(X, Y, ZZ, ZZZ):
    X, Y, ZZ, ZZZ = (v * RINV % P for v in (X, Y, ZZ, ZZZ))
    return None if ZZ == 0 else (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def test_chain_step_group_law(lazy):
    """start / madd_live / dbl_start against the affine group law: both signs, doubling,
    cancellation, an empty chain, and states at the maxima X = x + 7p, Y = y + p (the bounds are
    those of the normalized form: X3 < 8p, the rest < 2p)."""
    rng = random.Random(2903)
    g = (1, 2)
    rows, want, kinds = [], [], []
    for n in range(240):
        a = ob.g1_mul(g, rng.randrange(1, ob.R))
        b = ob.g1_mul(g, rng.randrange(1, ob.R))
        kind, neg = n % 6, (n // 6) % 2
        if kind == 3:
            b = a
        elif kind == 4:
            b = ob.g1_neg(a)
        if kind == 5:
            st = (0, 0, 0, 0)
        else:
            st = _state(a, rng, 7 if kind != 1 else rng.randrange(8), 1 if kind != 1 else rng.randrange(2))
        given = ob.g1_neg(b) if neg else b  # the table's point; neg adds its negative, which is b
        rows.append((*st, given[0] * RP % P + (n % 2) * P, given[1] * RP % P + (n // 2 % 2) * P, neg))
        want.append(tuple(b) if kind == 5 else ob.g1_add(a, b))
        kinds.append(kind)
    for row, w, kind, line in zip(rows, want, kinds, _run(lazy, "step", rows)):
        f = line.split()
        X, Y, ZZ, ZZZ = (_val(v) for v in f[:4])
        assert all(v <= M29 for h in f[:4] for v in _raw(h)[:8]), line
        assert X < 8 * P and Y < 2 * P and ZZ < 2 * P and ZZZ < 2 * P, line
        assert int(f[4]) == {3: 2, 4: 1}.get(kind, 0), line
        assert _affine(X, Y, ZZ, ZZZ) == (None if w is None else tuple(w)), row
        if w is None:
            assert ZZ == 0, line
