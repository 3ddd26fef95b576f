"""The extended-domain round trip on the device (sv_bn254_fr_coset_lde_device,
sv_bn254_fr_quotient_coeffs_device; csrc/ntt.hip, csrc/ext_plan.hpp) against Python-int arithmetic,
bit for bit.

Expected values.  An LDE is the Python FFT of test_gpu_ntt.py over the zero-padded coefficients (the
padding exists in Python only).  A quotient case draws h with 2^K generated coefficients (full
degree, so the truncation is real), feeds numer_j = h(g w_K^j) t(g w_K^j) with t(x) = x^n - 1 -- all
Python -- and expects h[:pieces n] back.  No expected value comes from the code under test.
References are computed once per (k, e, shift) and shared; no test modifies them.

Sizes.  T = kNttTileLog: K = k + e <= T is one launch, K in T + 1 .. 2 T two, K = 21 three.  (4, 8) is
two passes whose whole top digit is padding (blocks of pass 0 that hold no coefficient at all);
SVGPU_NTT_TILE_LOG in {1, 2, 3} runs e below, equal to and above the first digit and across several
digits at tiny sizes.  tests/COVERAGE_extended.md has the ledger."""
import functools

import numpy as np
import pytest

from oracle import bn254 as b
from stream_cases import environ
from test_gpu_kzg_open import _dev, _horner, _ints, _limb_bytes, _limbs
from test_gpu_ntt import CANONICAL, FORMS, G_GEN, MONTGOMERY, T, _fft, _forward, _gen, _root
from test_gpu_resident_bases import N as GEN_STRIDE, _UNREDUCED

pytestmark = pytest.mark.gpu

R = b.R
ZETA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
ZETA2 = ZETA * ZETA % R
LDE_SHIFTS = [None, ZETA, ZETA2, G_GEN]
QUOT_SHIFTS = [ZETA, ZETA2, G_GEN]
LDE_CASES = [(0, 0), (0, 3), (1, 1), (3, 2), (4, 8), (T - 2, 2), (T - 1, 2), (T, 1), (T, 2), (12, 3), (14, 2)]
QUOT_CASES = [(0, 0, 1), (0, 2, 3), (2, 2, 3), (3, 1, 2), (1, 3, 8), (1, 3, 5), (T - 1, 2, 3), (T, 2, 4), (13, 3, 7)]
CANARY = 0x0123456789ABCDEF


def test_the_constants():
    assert ZETA == pow(7, (R - 1) // 3, R) and ZETA != 1 and pow(ZETA, 3, R) == 1
    assert _fft([1, 2], R - 1) == [3, R - 1]


def _vals(n, skip=0):
    """n generated scalars: the edge-planted vector itself at 128 and more, else a slice of the
    256-vector (whose first entries would all be edge values)."""
    if n >= 128 and not skip:
        return list(_gen(n))
    flat = _gen(max(256, 2 * (n + skip)))
    return list(flat[3 + skip:3 + skip + n])


@functools.lru_cache(maxsize=None)
def _lde_pair(k, e, g, skip=0):
    """(a, the 2^(k + e) evaluations of a on g w_K^j)."""
    n = 1 << k
    a = _vals(n, skip)
    return tuple(a), tuple(_forward(a + [0] * ((n << e) - n), k + e, 1 if g is None else g))


def _t_values(k, e, g):
    """t(g w_K^j) for j < 2^e (it repeats with that period)."""
    gn, we = pow(g, 1 << k, R), _root(e)
    return [(gn * pow(we, j, R) - 1) % R for j in range(1 << e)]


@functools.lru_cache(maxsize=None)
def _quot_pair(k, e, g, skip=0):
    """(numer, h): h has 2^K generated coefficients, numer_j = h(g w_K^j) t(g w_K^j)."""
    K = k + e
    h = _vals(1 << K, skip)
    if K:
        h[-1] = h[-1] or 5                   # full degree
    t = _t_values(k, e, g)
    ev = _forward(h, K, g)
    return tuple(v * t[j & ((1 << e) - 1)] % R for j, v in enumerate(ev)), tuple(h)


def _same(t, values, form):
    return t.cpu().numpy().tobytes() == _limb_bytes(list(values), form)


def _lde(a, e, g, form, gpu, **kw):
    from svgpu import device as dv
    return dv.coset_lde_device(_dev(_limbs(list(a), form), gpu), e, shift=g, form=form, **kw)


# ---- LDE ----
@pytest.mark.parametrize("k,e", LDE_CASES)
def test_lde_dense(gpu, oracle_cpp, k, e):
    from svgpu import device as dv
    for g in LDE_SHIFTS:
        a, A = _lde_pair(k, e, g)
        for form in FORMS:
            src = _dev(_limbs(list(a), form), gpu)
            keep = src.clone()
            out = dv.coset_lde_device(src, e, shift=g, form=form)
            assert tuple(out.shape) == (1 << (k + e), 4)
            assert _same(out, A, form), (k, e, g, form)
            assert src.cpu().numpy().tobytes() == keep.cpu().numpy().tobytes()      # the input is only read
            if e == 0:
                assert out.cpu().numpy().tobytes() == dv.ntt_device(src, shift=g, form=form).cpu().numpy().tobytes()


@pytest.mark.parametrize("t", [1, 2, 3])
def test_lde_pass_structure_at_small_sizes(gpu, oracle_cpp, t):
    """SVGPU_NTT_TILE_LOG = t over every k <= 4, e <= 4: e below, equal to and above the first digit,
    and spanning several digits (t = 1: every digit one bit)."""
    with environ({"SVGPU_NTT_TILE_LOG": str(t)}):
        for k in range(5):
            for e in range(5):
                for g, form in ((G_GEN, CANONICAL), (G_GEN, MONTGOMERY), (None, MONTGOMERY), (ZETA, CANONICAL)):
                    a, A = _lde_pair(k, e, g)
                    assert _same(_lde(a, e, g, form, gpu), A, form), (t, k, e, g, form)


@pytest.mark.parametrize("count,k,e", [(5, 2, 1), (3, T - 1, 2)])
def test_lde_batches(gpu, oracle_cpp, count, k, e):
    """Polynomial t of the batch gives the Python result for slice t (the slices differ): at (2, 1) a
    block holds several polynomials, at (T - 1, 2) a polynomial spans several blocks.  The input is a
    buffer of exactly count n elements at the very end of its allocation; in a second run it lies
    between rows that are not below r, which a load past either end would bring into the result or
    the check."""
    import torch
    from svgpu import device as dv
    n, K = 1 << k, k + e
    flat = _vals(count * n, skip=11)
    want = [v for t in range(count) for v in _forward(flat[t * n:(t + 1) * n] + [0] * ((n << e) - n), K, G_GEN)]
    assert len({tuple(want[t << K:(t + 1) << K]) for t in range(count)}) == count
    for form in FORMS:
        rows = _dev(_limbs(flat, form), gpu)
        total = (count * n + 15) // 16 * 16                      # 512 B: the allocator's granule
        buf = torch.zeros((total, 4), dtype=torch.int64, device=gpu)
        tail = buf[total - count * n:]
        tail.copy_(rows)
        assert tail.data_ptr() + count * n * 32 == buf.data_ptr() + buf.numel() * 8
        out = dv.coset_lde_device(tail.reshape(count, n, 4), e, shift=G_GEN, form=form)
        assert tuple(out.shape) == (count, n << e, 4)
        assert _same(out, want, form), (count, k, e, form)
        fence = torch.from_numpy(np.tile(_UNREDUCED, (8 + count * n + 8, 1)).view(np.int64)).to(gpu)
        fence[8:8 + count * n] = rows
        out = dv.coset_lde_device(fence[8:8 + count * n].reshape(count, n, 4), e, shift=G_GEN, form=form)
        assert _same(out, want, form), ("fenced", count, k, e, form)


def _coset_samples(a, x0, s_log):
    """a(x0 w^s) for s < 2^s_log, w = root_of_unity(s_log), by Horner: a(x) = sum_r x^r A_r(x^S) with
    S = 2^s_log, and x^S = x0^S is the same at all S points -- S Horner runs of len(a) / S terms over
    the slices a[r::S], then one Horner run of S terms per point."""
    S = 1 << s_log
    y = pow(x0, S, R)
    A = [_horner(list(a[r::S]), y)[1] for r in range(S)]
    w = _root(s_log)
    return [_horner(A, x0 * pow(w, s, R) % R)[1] for s in range(S)]


def test_lde_three_pass_plan(gpu, oracle_cpp):
    """(19, 2): K = 21, three passes.  Generated input (on the device, the same scalars from the
    oracle).  The output is bit-equal to ntt_device on a zero-padded copy, and the 64 outputs
    j0 + s 2^15, s < 64, are checked against Horner in Python (they are the coset x0 w_6^s of one
    point x0 = g w_21^j0, so they share x^64 and the 64 Horner runs over a's residue classes)."""
    import torch
    from svgpu import device as dv
    k, e = 19, 2
    K, n = k + e, 1 << k
    a = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, n, start=11 * GEN_STRIDE))
    x = dv.gen_scalars(dv.empty_scalars(n, gpu), b.SEED_SCALARS, start=11 * GEN_STRIDE, form=MONTGOMERY)
    keep = x.clone()
    out = dv.coset_lde_device(x, e, shift=ZETA, form=MONTGOMERY)
    assert torch.equal(x, keep)
    padded = torch.zeros((1 << K, 4), dtype=torch.int64, device=gpu)
    padded[:n] = x
    assert torch.equal(out, dv.ntt_device(padded, shift=ZETA, form=MONTGOMERY))
    del padded
    j0 = 12345
    js = [j0 + (s << 15) for s in range(64)]
    got = _ints(out[js].cpu().numpy().view(np.uint64))
    minv = pow(1 << 256, R - 2, R)
    want = _coset_samples(a, ZETA * pow(_root(K), j0, R) % R, 6)
    assert [v * minv % R for v in got] == want


# ---- quotient ----
def _quot(numer, k, pieces, g, form, gpu, **kw):
    from svgpu import device as dv
    return dv.quotient_coeffs_device(_dev(_limbs(list(numer), form), gpu), k, pieces, g, form=form, **kw)


@pytest.mark.parametrize("k,e,pieces", QUOT_CASES)
def test_quotient(gpu, oracle_cpp, k, e, pieces):
    """Out of place with canary rows on both sides of d_out (nothing outside [0, pieces n) is
    written, and the input is only read), then in place (rows past pieces n are unspecified)."""
    import torch
    from svgpu import device as dv
    n, N = 1 << k, 1 << (k + e)
    keep = pieces * n
    for g in QUOT_SHIFTS:
        numer, h = _quot_pair(k, e, g)
        if keep < N:
            assert any(h[keep:])                                 # the truncation drops something
        for form in FORMS:
            src = _dev(_limbs(list(numer), form), gpu)
            before = src.cpu().numpy().tobytes()
            buf = torch.full((3 + keep + 5, 4), CANARY, dtype=torch.int64, device=gpu)
            out = dv.quotient_coeffs_device(src, k, pieces, g, form=form, out=buf[3:])
            assert out.data_ptr() == buf[3:].data_ptr() and tuple(out.shape) == (keep, 4)
            assert _same(out, h[:keep], form), (k, e, pieces, g, form)
            assert (torch.cat([buf[:3], buf[3 + keep:]]).cpu().numpy() == CANARY).all()
            assert src.cpu().numpy().tobytes() == before
            same = dv.quotient_coeffs_device(src, k, pieces, g, form=form, out=src)
            assert same.data_ptr() == src.data_ptr() and _same(same, h[:keep], form), ("in place", k, e, pieces, g, form)


@pytest.mark.parametrize("t", [1, 2, 3])
def test_quotient_pass_structure_at_small_sizes(gpu, oracle_cpp, t):
    """SVGPU_NTT_TILE_LOG = t: every k <= 3, e <= 3, pieces 1 .. 2^e; the table index is shared by a
    thread's elements (L_0 >= e) or not, and the cut falls inside, on and across the last digit."""
    import torch
    from svgpu import device as dv
    with environ({"SVGPU_NTT_TILE_LOG": str(t)}):
        for k in range(4):
            for e in range(4):
                g, form = (ZETA, CANONICAL) if (k + e) & 1 else (G_GEN, MONTGOMERY)
                numer, h = _quot_pair(k, e, g)
                src = _dev(_limbs(list(numer), form), gpu)
                for pieces in range(1, (1 << e) + 1):
                    keep = pieces << k
                    buf = torch.full((1 + keep + 2, 4), CANARY, dtype=torch.int64, device=gpu)
                    out = dv.quotient_coeffs_device(src, k, pieces, g, form=form, out=buf[1:])
                    assert _same(out, h[:keep], form), (t, k, e, pieces)
                    assert (torch.cat([buf[:1], buf[1 + keep:]]).cpu().numpy() == CANARY).all(), (t, k, e, pieces)


def test_quotient_shifts_on_and_next_to_the_domain(gpu, oracle_cpp):
    """g = 1, r - 1 and w_K^3 have g^(2^K) = 1 and stop at rule 5; w_(K+1) is one squaring outside
    and is a coset like any other."""
    import svgpu
    k, e = 3, 1
    K = k + e
    numer, h = _quot_pair(k, e, ZETA)
    for form in FORMS:
        for g in (1, R - 1, pow(_root(K), 3, R)):
            with pytest.raises(svgpu.ArgumentError, match="coset meets the domain"):
                _quot(numer, k, 1, g, form, gpu)
        g = _root(K + 1)
        numer2, h2 = _quot_pair(k, e, g)
        assert _same(_quot(numer2, k, 2, g, form, gpu), h2, form)
        assert _same(_quot(numer, k, 1, ZETA, form, gpu), h[:1 << k], form)


def test_unreduced_elements_are_rejected(gpu, oracle_cpp):
    """An element not below r at the first and at the last index, and in the last polynomial of a
    batch, is an ArgumentError for that call in both forms; the next call is exact."""
    import svgpu
    from svgpu import device as dv
    k, e = T - 1, 2
    n, N = 1 << k, 1 << (k + e)
    a, A = _lde_pair(k, e, G_GEN)
    numer, h = _quot_pair(k, e, G_GEN)
    for form in FORMS:
        good = _limbs(list(a), form)
        for idx in (0, n - 1):
            bad = good.copy()
            bad[idx] = _UNREDUCED
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                dv.coset_lde_device(_dev(bad, gpu), e, shift=G_GEN, form=form)
            assert _same(dv.coset_lde_device(_dev(good, gpu), e, shift=G_GEN, form=form), A, form), (form, idx)
        bad3 = np.stack([good, good, good])
        bad3[2, n - 3] = _UNREDUCED
        with pytest.raises(svgpu.ArgumentError, match="not reduced"):
            dv.coset_lde_device(_dev(bad3.reshape(-1, 4), gpu).reshape(3, n, 4), e, form=form)
        goodq = _limbs(list(numer), form)
        for idx in (0, N - 1):
            bad = goodq.copy()
            bad[idx] = _UNREDUCED
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                dv.quotient_coeffs_device(_dev(bad, gpu), k, 3, G_GEN, form=form)
            assert _same(dv.quotient_coeffs_device(_dev(goodq, gpu), k, 3, G_GEN, form=form), h[:3 * n], form)
    with pytest.raises(svgpu.ArgumentError, match="not reduced"):       # the shift, before any device work
        dv.coset_lde_device(_dev(good, gpu), e, shift=R)
    with pytest.raises(svgpu.ArgumentError, match="not reduced"):
        dv.quotient_coeffs_device(_dev(goodq, gpu), k, 1, R)


def test_wrappers_refuse_bad_shapes(gpu):
    import torch
    import svgpu
    from svgpu import device as dv
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=gpu)
    for rows in (3, 0, 6):
        with pytest.raises(svgpu.LengthError, match="power of two"):
            dv.coset_lde_device(z(rows, 4), 1)
        with pytest.raises(svgpu.LengthError, match="power of two"):
            dv.quotient_coeffs_device(z(rows, 4), 0, 1, ZETA)
    with pytest.raises(svgpu.LengthError):
        dv.coset_lde_device(z(4, 4), 9)
    with pytest.raises(svgpu.LengthError):
        dv.coset_lde_device(z(4, 4), 1, out=z(4, 4))
    with pytest.raises(svgpu.ArgumentError):
        dv.coset_lde_device(z(4, 5), 1)
    with pytest.raises(svgpu.LengthError):
        dv.quotient_coeffs_device(z(8, 4), 1, 5, ZETA)              # 4 pieces at most
    with pytest.raises(svgpu.LengthError):
        dv.quotient_coeffs_device(z(8, 4), 4, 1, ZETA)
    with pytest.raises(svgpu.LengthError):
        dv.quotient_coeffs_device(z(8, 4), 1, 2, ZETA, out=z(3, 4))
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        buf = z(16, 4)
        dv.coset_lde_device(buf[0:4], 1, out=buf[2:10])
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        buf = z(16, 4)
        dv.quotient_coeffs_device(buf[0:8], 1, 2, ZETA, out=buf[6:10])
    with pytest.raises(svgpu.ArgumentError, match="null"):
        dv.quotient_coeffs_device(z(8, 4), 1, 2, None)
    assert _same(svgpu.coset_lde_device(z(4, 4), 1, form=CANONICAL), [0] * 8, CANONICAL)
    assert _same(svgpu.quotient_coeffs_device(z(8, 4), 2, 1, ZETA, form=CANONICAL), [0] * 4, CANONICAL)


# ---- the two calls together ----
def test_round_trip_of_a_product_relation(gpu, oracle_cpp):
    """k = 4, e = 1: generated a and b; c = a o b on the domain (its coefficients by Python, degree <
    n); the LDE of all three in one batch; the numerator a b - c from the downloaded evaluations in
    Python; quotient_coeffs with pieces = 1; then a(x) b(x) - c(x) = h(x) (x^n - 1) at a generated x."""
    from svgpu import device as dv
    k, e = 4, 1
    n, K = 1 << k, k + e
    a, bb = _vals(n, skip=40), _vals(n, skip=80)
    ea, eb = _forward(a, k), _forward(bb, k)
    ec = [u * v % R for u, v in zip(ea, eb)]
    winv, ninv = pow(_root(k), R - 2, R), pow(n, R - 2, R)
    c = [v * ninv % R for v in _fft(ec, winv)]
    assert _forward(c, k) == ec
    for form in FORMS:
        cols = _dev(_limbs(a + bb + c, form), gpu).reshape(3, n, 4)
        ext = dv.coset_lde_device(cols, e, shift=ZETA, form=form)
        vals = _ints(ext.cpu().numpy().view(np.uint64))
        if form == MONTGOMERY:
            minv = pow(1 << 256, R - 2, R)
            vals = [v * minv % R for v in vals]
        A, B, C = vals[:1 << K], vals[1 << K:2 << K], vals[2 << K:]
        numer = [(u * v - w) % R for u, v, w in zip(A, B, C)]
        h = _ints(_quot(numer, k, 1, ZETA, form, gpu).cpu().numpy().view(np.uint64))
        if form == MONTGOMERY:
            h = [v * minv % R for v in h]
        x = b.gen_scalar(b.SEED_SCALARS, 31337)
        ev = lambda p: _horner(list(p), x)[1]
        assert (ev(a) * ev(bb) - ev(c)) % R == ev(h) * (pow(x, n, R) - 1) % R, form
        assert any(h)


def test_commit_pieces_on_a_resident_set(gpu, oracle_cpp):
    """n = 16, pieces = 3 of a (16, 2) quotient: each commitment against the C++ oracle's MSM of the
    piece's Python coefficients."""
    import svgpu
    from svgpu import encoding as enc
    k, e, pieces = 4, 2, 3
    n = 1 << k
    numer, h = _quot_pair(k, e, ZETA2)
    bases = oracle_cpp.gen_bases(b.SEED_BASES, n)
    with svgpu.ResidentBases(bases) as rs:
        for form in FORMS:
            hd = _quot(numer, k, pieces, ZETA2, form, gpu)
            got = svgpu.commit_pieces(rs, hd, n, form)
            assert len(got) == pieces
            for i, point in enumerate(got):
                want = oracle_cpp.msm_pippenger(bases, enc.scalars_array(list(h[i * n:(i + 1) * n])), 0)
                assert point == b.g1_from_bytes(want.tobytes()), (form, i)
            assert len(set(got)) == pieces
        with pytest.raises(svgpu.LengthError):
            svgpu.commit_pieces(rs, hd[:n + 1], n, form)
