"""Device paths of the fused field primitives (csrc/field.hpp fe_sqr_hp / fe_mul_sum<N>,
csrc/curve.hpp mul_diff) on edge operands, against Python big-int Montgomery arithmetic.

Their inline-asm device code differs from the host build (which falls back to a*a and separate
products) and the MSM / Poseidon parity tests only reach them with random operands; this hits
the boundary cases of the one-reduction bound: 0, 1, p-1, p-2, 2^k, all-ones low limbs, and
the N = 3 worst case near 1.75 p that needs the final conditional subtraction.  Harness:
tests/native/fieldcheck.hip (test-only, built by __graft_entry__.build()).

Also the 2p-domain helpers of csrc/field.hpp (fe_mul_lazy, fe_add2p, fe_sub2p, fe_neg2p,
fe_canon2p, fe_is_zero2p) on both representatives of 0, the top of [0, 2p) and sums of exactly 2p,
and the point operations built on them -- csrc/quad.hpp's add_2p / dbl_2p (DPP moves: no host
build) and xyzz_add_2p -- over a chosen mix of generic, doubling, cancelling and identity cases
inside each wave, against the oracle's affine group law.
"""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import ROOT
from oracle import bn254 as b

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tests", "native", "build", "libfieldcheck.so")
MODS = {0: b.P, 1: b.R}
OP_MUL, OP_SQR_HP, OP_SUM1, OP_SUM2, OP_SUM3, OP_MUL_DIFF = range(6)


def _edges(p):
    v = [0, 1, 2, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, (1 << 253), (1 << 253) - 1, p >> 1]
    v += [1 << k for k in range(0, 254, 17)]
    v += [(1 << (32 * k)) - 1 for k in range(1, 8)]             # all-ones low limbs
    v += [p - ((1 << (32 * k)) - 1) for k in range(1, 7)]       # just below p, ragged low limbs
    v += [(p - 1) ^ ((1 << 32) - 1)]
    rng = random.Random(0xF1E1D)
    v += [rng.randrange(p) for _ in range(24)]
    return [x % p for x in v]


def _arr(vals):
    out = np.zeros((len(vals), 8), np.uint32)
    for i, x in enumerate(vals):
        for k in range(8):
            out[i, k] = (x >> (32 * k)) & 0xFFFFFFFF
    return out


def _ints(a):
    return [sum(int(r[k]) << (32 * k) for k in range(8)) for r in a]


@pytest.fixture(scope="module")
def fc():
    assert os.path.exists(LIB), "tests/native/build/libfieldcheck.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(LIB)
    lib.fc_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    lib.fc_run.restype = ctypes.c_int
    lib.fc_points.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    lib.fc_points.restype = ctypes.c_int
    return lib


def _run(fc, op, field, A, B, C, D):
    arrs = [_arr(x) for x in (A, B, C, D)]
    out = np.zeros_like(arrs[0])
    rc = fc.fc_run(op, field, *[x.ctypes.data for x in arrs], out.ctypes.data, len(A))
    assert rc == 0, f"fc_run hip error {rc}"
    return _ints(out)


@pytest.mark.parametrize("field", [0, 1], ids=["Fq", "Fr"])
def test_fused_primitives_on_edges(gpu, fc, field):
    p = MODS[field]
    rinv = pow(1 << 256, -1, p)
    E = _edges(p)
    # all ordered pairs of edge values for the products; c, d shifted copies for the sums
    A = [x for x in E for _ in E]
    B = [y for _ in E for y in E]
    C = B[7:] + B[:7]
    D = A[13:] + A[:13]
    mont = lambda x, y: x * y * rinv % p  # noqa: E731
    assert _run(fc, OP_MUL, field, A, B, C, D) == [mont(x, y) for x, y in zip(A, B)]
    assert _run(fc, OP_SQR_HP, field, A, B, C, D) == [mont(x, x) for x in A]
    assert _run(fc, OP_SUM1, field, A, B, C, D) == [mont(x, y) for x, y in zip(A, B)]
    assert _run(fc, OP_SUM2, field, A, B, C, D) == [(x * y + z * w) * rinv % p for x, y, z, w in zip(A, B, C, D)]
    assert _run(fc, OP_SUM3, field, A, B, C, D) == [(x * y + z * w + y * z) * rinv % p
                                                    for x, y, z, w in zip(A, B, C, D)]
    if field == 0:
        assert _run(fc, OP_MUL_DIFF, field, A, B, C, D) == [(x * y - z * w) * rinv % p
                                                            for x, y, z, w in zip(A, B, C, D)]


@pytest.mark.parametrize("field", [0, 1], ids=["Fq", "Fr"])
def test_sum3_worst_case_needs_final_subtraction(gpu, fc, field):
    """Three products of (p-1)^2 scan to just under the 2p bound: the result must still be reduced."""
    p = MODS[field]
    rinv = pow(1 << 256, -1, p)
    top = [p - 1, p - 2, p - 1 - (1 << 200), p - ((1 << 64) - 1)]
    A = [x for x in top for _ in top]
    B = [y for _ in top for y in top]
    got = _run(fc, OP_SUM3, field, A, B, B, A)
    exp = [(x * y + y * x + y * y) * rinv % p for x, y in zip(A, B)]
    assert got == exp
    assert all(g < p for g in got)


# ---------------------------------------------------------------- the 2p domain (csrc/field.hpp)
OP_MUL_LAZY, OP_ADD2P, OP_SUB2P, OP_NEG2P, OP_CANON2P, OP_IS_ZERO2P = range(6, 12)


def _edges_2p(p):
    """Operands in [0, 2p): both representatives of 0 and their neighbours, the top of the range,
    powers of two, random values.  All ordered pairs hold the sums that are exactly 2p and 2p - 1
    (p + p, (p + 1) + (p - 1), (2p - 1) + 1; (2p - 1) + 0, p + (p - 1)), a - a, 0 - (2p - 1) and
    (2p - 1)^2."""
    v = [0, 1, 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1]
    v += [1 << k for k in range(3, 255, 11)] + [1 << 254]
    rng = random.Random(0x2F)
    v += [rng.randrange(2 * p) for _ in range(24)]
    assert all(0 <= x < 2 * p for x in v)
    return v


@pytest.mark.parametrize("field", [0, 1], ids=["Fq", "Fr"])
def test_2p_domain_helpers(gpu, fc, field):
    p = MODS[field]
    rinv = pow(1 << 256, -1, p)
    E = _edges_2p(p)
    A = [x for x in E for _ in E]
    B = [y for _ in E for y in E]
    got = _run(fc, OP_MUL_LAZY, field, A, B, A, B)
    assert all(g < 2 * p and g % p == x * y * rinv % p for g, x, y in zip(got, A, B))
    assert _run(fc, OP_ADD2P, field, A, B, A, B) == [x + y - (2 * p if x + y >= 2 * p else 0) for x, y in zip(A, B)]
    assert _run(fc, OP_SUB2P, field, A, B, A, B) == [x - y + (2 * p if x < y else 0) for x, y in zip(A, B)]
    U = E + [2 * p]  # fe_neg2p takes [0, 2p] and gives [0, 2p]
    assert _run(fc, OP_NEG2P, field, U, U, U, U) == [2 * p - x for x in U]
    assert _run(fc, OP_CANON2P, field, E, E, E, E) == [x % p for x in E]
    assert _run(fc, OP_IS_ZERO2P, field, E, E, E, E) == [1 if x % p == 0 else 0 for x in E]


# ---------------------------------------------------------------- point operations in the 2p domain
PT_QUAD_ADD, PT_QUAD_DBL, PT_XYZZ_ADD = range(3)
_OTHERS = ["generic", "cancel", "id-a", "id-b", "id-both"]


def _wave_plan():
    """The kind of case at each of the 16 quads of every wave: a wave without a doubling, waves where
    exactly one quad doubles (quad 0, quad 15, one in the middle) among the other kinds, and an
    all-doubling wave; the other kinds rotate, so each sits at different quads in different waves."""
    waves = []
    for r in range(6):
        mix = lambda shift: [_OTHERS[(i + r + shift) % 5] for i in range(16)]  # noqa: E731
        dbl = "dbl-same-rep" if r & 1 else "dbl"
        waves.append(mix(0))
        for n, at in enumerate((0, 15, 5 + r)):
            w = mix(n + 1)
            w[at] = dbl
            waves.append(w)
        waves.append(["dbl" if (i + r) & 1 else "dbl-same-rep" for i in range(16)])
    return waves


def _mont_rep(v, rng):
    return v * b.RP % b.P + rng.randrange(2) * b.P


def _xyzz_2p(pt, rng):
    """A random XYZZ representation in the 2p domain (x R form, each coordinate plus 0 or p)."""
    z = rng.randrange(1, b.P)
    zz, zzz = z * z % b.P, z * z * z % b.P
    return tuple(_mont_rep(v, rng) for v in (pt[0] * zz, pt[1] * zzz, zz, zzz))


def _identity_2p(rng, n):
    """ZZ = 0 exactly; the other coordinates zero, or anything in [0, 2p)."""
    if n & 1:
        return (0, 0, 0, 0)
    return (rng.randrange(2 * b.P), rng.randrange(2 * b.P), 0, rng.randrange(2 * b.P))


@pytest.fixture(scope="module")
def point_cases():
    """(a's coordinates, b's coordinates, a, b, kind) per quad, in wave order."""
    import f29_cases
    rng = random.Random(0x9AD)
    pts = f29_cases.points()
    cases = []
    for wave in _wave_plan():
        assert len(wave) == 16
        for kind in wave:
            pa, pb = rng.sample(pts, 2)
            if kind.startswith("dbl"):
                pb = pa
            elif kind == "cancel":
                pb = b.g1_neg(pa)
            sa, sb = _xyzz_2p(pa, rng), _xyzz_2p(pb, rng)
            if kind == "dbl-same-rep":
                sb = sa
            if kind in ("id-a", "id-both"):
                sa, pa = _identity_2p(rng, len(cases)), None
            if kind in ("id-b", "id-both"):
                sb, pb = _identity_2p(rng, len(cases) >> 1), None
            cases.append((sa, sb, pa, pb, kind))
    return cases


def _points(fc, op, SA, SB):
    a = np.stack([_arr(s) for s in SA])  # n x 4 x 8
    bb = np.stack([_arr(s) for s in SB])
    out = np.zeros_like(a)
    rc = fc.fc_points(op, a.ctypes.data, bb.ctypes.data, out.ctypes.data, len(SA))
    assert rc == 0, f"fc_points hip error {rc}"
    return [_ints(r) for r in out]


def _check_points(got, want, cases):
    rinv = pow(1 << 256, -1, b.P)
    for (X, Y, ZZ, ZZZ), w, c in zip(got, want, cases):
        assert max(X, Y, ZZ, ZZZ) < 2 * b.P, c
        x, y, zz, zzz = (v * rinv % b.P for v in (X, Y, ZZ, ZZZ))
        aff = None if zz == 0 else (x * pow(zz, -1, b.P) % b.P, y * pow(zzz, -1, b.P) % b.P)
        assert aff == (None if w is None else tuple(w)), c  # an identity result: ZZ = 0 mod p


@pytest.mark.parametrize("op", [PT_QUAD_ADD, PT_XYZZ_ADD], ids=["quad", "one-lane"])
def test_add_2p_chosen_mix_in_each_wave(gpu, fc, point_cases, op):
    """quad::add_2p (one point per quad of lanes: the wave-uniform doubling branch with its per-quad
    select, the per-quad exceptional flags) and xyzz_add_2p on the same inputs."""
    got = _points(fc, op, [c[0] for c in point_cases], [c[1] for c in point_cases])
    _check_points(got, [b.g1_add(c[2], c[3]) for c in point_cases], point_cases)


def test_quad_dbl_2p(gpu, fc, point_cases):
    """quad::dbl_2p of every first operand (the identity stays the identity)."""
    SA = [c[0] for c in point_cases]
    _check_points(_points(fc, PT_QUAD_DBL, SA, SA), [b.g1_add(c[2], c[2]) for c in point_cases], point_cases)


def test_fc_points_takes_whole_waves_only(gpu, fc):
    buf = np.zeros((17, 4, 8), np.uint32)
    assert fc.fc_points(PT_QUAD_ADD, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 17) != 0
