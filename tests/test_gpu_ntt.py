"""Fr NTT on the device (sv_bn254_fr_ntt_device; csrc/ntt.hip, csrc/ntt_plan.hpp) against Python-int
arithmetic, bit for bit: out[j] = sum_i in[i] (g w^j)^i with w = root_of_unity(k), and its inverse.

Expected values.  A dense input goes through the recursive radix-2 FFT below (0.8 s at 2^16, never
run above that), a sparse one (up to three non-zero entries) through running powers, a sampled
output through Horner.  The inverse tests feed the Python forward output and expect the input back,
so no expected value comes from the code under test.  References are computed once per
(k, kind, shift) and shared; no test modifies them.

Sizes.  T = kNttTileLog (read from csrc/ntt.hpp): a transform takes ceil(k / T) launches, so k in
{0, 1, 2, 3, 4, T - 1, T, T + 1, T + 2, 16} covers the checked copy, the single pass with partly and
fully used blocks, and the two-pass plans with even and uneven widths; SVGPU_NTT_TILE_LOG in
{1, 2, 3} runs one to four and more passes at k <= 10; k = 2 T and 2 T + 1 run the default plan at
its large sizes once each.  tests/COVERAGE_ntt.md has the ledger."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import PKG
from oracle import bn254 as b
from stream_cases import environ
from test_gpu_kzg_open import _dev, _div_coeffs, _horner, _ints, _limb_bytes, _limbs
from test_gpu_resident_bases import N, _UNREDUCED

pytestmark = pytest.mark.gpu

T = int(re.search(r"constexpr uint32_t kNttTileLog = (\d+);", open(os.path.join(PKG, "csrc", "ntt.hpp")).read()).group(1))
R = b.R
ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c
CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
DENSE_K = sorted({0, 1, 2, 3, 4, T - 1, T, T + 1, T + 2, 16})  # 4: the widest tile with 128 columns to a block
KINDS = ["generated", "zero", "first", "last"]
G_GEN = b.gen_scalar(b.SEED_SCALARS, 555001)
SHIFTS = [1, R - 1, G_GEN]


def _root(k):
    return pow(ROOT_OF_UNITY, 1 << (28 - k), R)


def _fft(a, w):
    """w = the root for len(a); natural order in and out."""
    n = len(a)
    if n == 1:
        return a
    w2 = w * w % R
    e, o = _fft(a[0::2], w2), _fft(a[1::2], w2)
    out, x, h = [0] * n, 1, n // 2
    for i in range(h):
        t = x * o[i] % R
        out[i], out[i + h] = (e[i] + t) % R, (e[i] - t) % R
        x = x * w % R
    return out


def _forward(a, k, g=1):
    """out[j] = sum_i a[i] (g w^j)^i: running powers for a sparse a, else the FFT (k <= 16)."""
    n, w = 1 << k, _root(k)
    nz = [(i, c) for i, c in enumerate(a) if c]
    if len(nz) <= 3:
        terms = [(c * pow(g, i, R) % R, pow(w, i, R)) for i, c in nz]   # c g^i (w^i)^j
        out = []
        for _ in range(n):
            out.append(sum(c for c, _ in terms) % R)
            terms = [(c * s % R, s) for c, s in terms]
        return out
    assert k <= 16, "no full Python FFT above 2^16"
    x, p = list(a), 1
    if g != 1:
        for i in range(n):
            x[i] = x[i] * p % R
            p = p * g % R
    return _fft(x, w)


@functools.lru_cache(maxsize=None)
def _gen(n):
    """n generated scalars with the EDGE values planted (test_gpu_kzg_open._div_coeffs)."""
    from oracle import cpu_ref
    return tuple(_div_coeffs(cpu_ref, n, "generated"))


@functools.lru_cache(maxsize=None)
def _pair(k, kind, g=1):
    """(a, forward(a)) for one transform of 2^k points."""
    from oracle import cpu_ref
    a = list(_gen(1 << k)) if kind == "generated" else _div_coeffs(cpu_ref, 1 << k, kind)
    return tuple(a), tuple(_forward(a, k, g))


def _run(values, form, gpu, **kw):
    from svgpu import device as dv
    return dv.ntt_device(_dev(_limbs(list(values), form), gpu), form=form, **kw)


def _same(t, values, form):
    return t.cpu().numpy().tobytes() == _limb_bytes(list(values), form)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", DENSE_K)
def test_dense_forward_and_inverse(gpu, oracle_cpp, k, kind):
    a, A = _pair(k, kind)
    for form in FORMS:
        out = _run(a, form, gpu)
        assert tuple(out.shape) == (1 << k, 4)
        assert _same(out, A, form), ("forward", k, kind, form)
        assert _same(_run(A, form, gpu, inverse=True), a, form), ("inverse", k, kind, form)


@pytest.mark.parametrize("g", SHIFTS, ids=["one", "minus-one", "generated"])
@pytest.mark.parametrize("k", [3, T + 1])
def test_coset_forward_and_inverse(gpu, oracle_cpp, k, g):
    a, A = _pair(k, "generated", g)
    if g == 1:
        assert A == _pair(k, "generated")[1]
    else:
        assert A != _pair(k, "generated")[1]
    for form in FORMS:
        assert _same(_run(a, form, gpu, shift=g), A, form), ("forward", k, g, form)
        assert _same(_run(A, form, gpu, shift=g, inverse=True), a, form), ("inverse", k, g, form)


@pytest.mark.parametrize("count,k", [(5, 2), (3, T + 1), (2, 16)])
def test_batch_is_transform_by_transform(gpu, oracle_cpp, count, k):
    """Transform t of the batch equals the Python result for slice t (the slices differ); with a
    coset at the small sizes, where a block holds several transforms or a transform several blocks."""
    from svgpu import device as dv
    n = 1 << k
    g = G_GEN if k < 16 else 1
    flat = _gen(count * n)
    a = [flat[t * n:(t + 1) * n] for t in range(count)]
    A = [_forward(list(x), k, g) for x in a]
    assert len({tuple(x) for x in A}) == count
    for form in FORMS if k < 16 else (MONTGOMERY,):
        d = _dev(_limbs(list(flat), form), gpu).reshape(count, n, 4)
        out = dv.ntt_device(d, form=form, shift=g)
        assert tuple(out.shape) == (count, n, 4)
        assert _same(out, [v for x in A for v in x], form), ("forward", count, k, form)
        back = dv.ntt_device(out, form=form, shift=g, inverse=True, out=out)      # in place, batched
        assert back.data_ptr() == out.data_ptr() and _same(back, flat, form), ("inverse", count, k, form)


@pytest.mark.parametrize("k", [3, T + 1])
def test_placement(gpu, oracle_cpp, k):
    """Out of place leaves the input bytes untouched and the canary rows around d_out intact; in
    place gives the same bytes; `out=` and the input may be views at odd row offsets (32-B rows are
    always 16-B aligned)."""
    import torch
    from svgpu import device as dv
    n = 1 << k
    a, A = _pair(k, "generated", G_GEN)
    canary = 0x0123456789ABCDEF
    for form in FORMS:
        want, src = _limb_bytes(list(A), form), _limb_bytes(list(a), form)
        for inverse, x, y in ((False, src, want), (True, want, src)):
            buf = torch.full((n + 3 + n + 5, 4), canary, dtype=torch.int64, device=gpu)
            inp = torch.full((n + 2, 4), canary, dtype=torch.int64, device=gpu)
            inp[1:n + 1] = torch.from_numpy(np.frombuffer(x, np.int64).reshape(n, 4).copy()).to(gpu)
            before = inp.cpu().numpy().tobytes()
            out = dv.ntt_device(inp[1:n + 1], form=form, shift=G_GEN, inverse=inverse, out=buf[3:n + 3])
            assert out.data_ptr() == buf[3:].data_ptr()
            assert out.cpu().numpy().tobytes() == y, (k, form, inverse)
            assert inp.cpu().numpy().tobytes() == before                       # the input is only read
            rest = torch.cat([buf[:3], buf[n + 3:]]).cpu().numpy()
            assert (rest == canary).all()                                      # nothing outside d_out
            same = dv.ntt_device(inp[1:n + 1], form=form, shift=G_GEN, inverse=inverse, out=inp[1:n + 1])
            assert same.cpu().numpy().tobytes() == y, (k, form, inverse)       # in place
            edge = inp.cpu().numpy()
            assert (edge[0] == canary).all() and (edge[n + 1] == canary).all()


def _sweep_k(t):
    return list(range(1, 3 * t + 2))


@pytest.mark.parametrize("t", [1, 2, 3])
def test_pass_counts_at_small_sizes(gpu, oracle_cpp, t):
    """SVGPU_NTT_TILE_LOG = t: every k from 1 to 3 t + 1 (one to four passes -- and k passes at
    t = 1 --, even and uneven splits), forward and inverse in both forms, a coset at k = 3 t + 1 and
    a batch of three at k = 2 t + 1."""
    from svgpu import device as dv
    with environ({"SVGPU_NTT_TILE_LOG": str(t)}):
        for k in _sweep_k(t):
            a, A = _pair(k, "generated")
            for form in FORMS:
                assert _same(_run(a, form, gpu), A, form), ("forward", t, k, form)
                assert _same(_run(A, form, gpu, inverse=True), a, form), ("inverse", t, k, form)
        k = 3 * t + 1
        a, A = _pair(k, "generated", G_GEN)
        for form in FORMS:
            assert _same(_run(a, form, gpu, shift=G_GEN), A, form), ("coset forward", t, form)
            assert _same(_run(A, form, gpu, shift=G_GEN, inverse=True), a, form), ("coset inverse", t, form)
        k, count = 2 * t + 1, 3
        n = 1 << k
        flat = _gen(count * n)
        want = [v for c in range(count) for v in _forward(list(flat[c * n:(c + 1) * n]), k)]
        d = _dev(_limbs(list(flat), MONTGOMERY), gpu).reshape(count, n, 4)
        assert _same(dv.ntt_device(d, form=MONTGOMERY), want, MONTGOMERY), ("batch", t)


@pytest.mark.parametrize("value", ["0", str(T + 1), "-3", "2x", "", "999999999999999999999"])
def test_switch_out_of_range_runs_the_default_plan(gpu, oracle_cpp, value):
    k = T + 1
    a, A = _pair(k, "generated")
    with environ({"SVGPU_NTT_TILE_LOG": value}):
        assert _same(_run(a, MONTGOMERY, gpu), A, MONTGOMERY)
        assert _same(_run(A, CANONICAL, gpu, inverse=True), a, CANONICAL)


def _sparse(k, inverse):
    """Three monomials at 1, n / 2 + 3 and n - 1 with generated coefficients, and the whole transform
    of that vector in Montgomery form, built with running powers: forward sum_t c_t (w^e_t)^j; the
    inverse is the same sum over w^-1, times 1 / n (the sparse check transposed)."""
    n = 1 << k
    w = _root(k)
    if inverse:
        w = pow(w, R - 2, R)
    scale = pow(n, R - 2, R) if inverse else 1
    where = [1, n // 2 + 3, n - 1]
    coeff = [b.gen_scalar(b.SEED_SCALARS, 777000 + i) for i in range(3)]
    m = (1 << 256) % R
    (c0, s0), (c1, s1), (c2, s2) = [(c * scale * m % R, pow(w, e, R)) for c, e in zip(coeff, where)]
    out = bytearray(32 * n)
    for j in range(n):
        out[32 * j:32 * j + 32] = ((c0 + c1 + c2) % R).to_bytes(32, "little")
        c0, c1, c2 = c0 * s0 % R, c1 * s1 % R, c2 * s2 % R
    rows = np.zeros((n, 4), np.uint64)
    rows[where] = _limbs(coeff, MONTGOMERY)
    return rows, bytes(out)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("k", [2 * T, 2 * T + 1])
def test_default_plan_large_sparse(gpu, oracle_cpp, k, inverse):
    """The default plan at k = 2 T (two full tiles) and 2 T + 1 (three passes), Montgomery only: a
    sparse input of three monomials, the whole output compared."""
    from svgpu import device as dv
    rows, want = _sparse(k, inverse)
    out = dv.ntt_device(_dev(rows, gpu), form=MONTGOMERY, inverse=inverse)
    assert out.cpu().numpy().tobytes() == want


def test_default_plan_large_dense_samples(gpu, oracle_cpp):
    """k = 2 T, a dense generated input (generated on the device, the same scalars from the oracle):
    outputs j in {0, 1, n / 2 + 1, n - 1} against Python Horner at w^j.  The round trip
    inverse(forward(x)) == x is asserted too; it alone would prove nothing (any invertible map and
    its inverse pass it), the sampled outputs pin the map.  k = 2 T + 1 launches no instantiation or
    branch that smaller sizes do not (tests/COVERAGE_ntt.md), so it runs under the sparse check
    only."""
    import torch
    from svgpu import device as dv
    k = 2 * T
    n, w = 1 << k, _root(k)
    a = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, n, start=9 * N))
    x = dv.gen_scalars(dv.empty_scalars(n, gpu), b.SEED_SCALARS, start=9 * N, form=MONTGOMERY)
    keep = x.clone()
    out = dv.ntt_device(x, form=MONTGOMERY)
    got = _ints(out[[0, 1, n // 2 + 1, n - 1]].cpu().numpy().view(np.uint64))
    minv = pow(1 << 256, R - 2, R)
    for j, v in zip((0, 1, n // 2 + 1, n - 1), got):
        assert v * minv % R == _horner(a, pow(w, j, R))[1], j
    assert torch.equal(x, keep)
    back = dv.ntt_device(out, form=MONTGOMERY, inverse=True)
    assert torch.equal(back, keep)


def test_unreduced_elements_are_rejected(gpu, oracle_cpp):
    """k = T + 1: an element not below r at 0, in the middle of the second tile and at n - 1 is an
    ArgumentError for that call, in both forms and both directions; the next call is exact."""
    import svgpu
    from svgpu import device as dv
    k = T + 1
    n = 1 << k
    a, A = _pair(k, "generated")
    for form in FORMS:
        good = _limbs(list(a), form)
        for idx in (0, (1 << T) + (1 << (T - 1)), n - 1):
            bad = good.copy()
            bad[idx] = _UNREDUCED
            for inverse in (False, True):
                with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                    dv.ntt_device(_dev(bad, gpu), form=form, inverse=inverse)
            assert _same(dv.ntt_device(_dev(good, gpu), form=form), A, form), (form, idx)
    bad3 = np.stack([good, good, good])
    bad3[2, 5] = _UNREDUCED                                            # in the last transform of a batch
    with pytest.raises(svgpu.ArgumentError, match="not reduced"):
        dv.ntt_device(_dev(bad3.reshape(-1, 4), gpu).reshape(3, n, 4), form=MONTGOMERY)
    with pytest.raises(svgpu.ArgumentError, match="not reduced"):      # the shift, before any device work
        dv.ntt_device(_dev(good, gpu), shift=R)


def test_wrapper_refuses_bad_shapes(gpu):
    import torch
    import svgpu
    from svgpu import device as dv
    for rows in (3, 0, 6):
        with pytest.raises(svgpu.LengthError, match="power of two"):
            dv.ntt_device(torch.zeros((rows, 4), dtype=torch.int64, device=gpu))
    with pytest.raises(svgpu.LengthError):
        dv.ntt_device(torch.zeros((2, 3, 4), dtype=torch.int64, device=gpu))
    x = torch.zeros((4, 4), dtype=torch.int64, device=gpu)
    with pytest.raises(svgpu.LengthError):
        dv.ntt_device(x, out=torch.zeros((8, 4), dtype=torch.int64, device=gpu))
    with pytest.raises(svgpu.ArgumentError):
        dv.ntt_device(torch.zeros((4, 5), dtype=torch.int64, device=gpu))
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        buf = torch.zeros((12, 4), dtype=torch.int64, device=gpu)
        dv.ntt_device(buf[0:8], out=buf[1:9])
    assert _same(svgpu.ntt_device(x, form=CANONICAL), [0] * 4, CANONICAL)


def test_evaluations_to_opening_end_to_end(gpu, oracle_cpp):
    """A prover's column: the evaluations of a generated polynomial on the 2^11 domain (Python FFT) go
    through the device inverse NTT to coefficients in HBM, which open_device opens on a set s^i g; the
    commitment and the witness satisfy the decider, and poly_eval_points_device at w^j returns the
    original evaluations."""
    import svgpu
    from svgpu import device as dv
    k = 11
    n, w = 1 << k, _root(k)
    a, evals = _pair(k, "generated")
    s = b.gen_scalar(b.SEED_TRAPDOOR, 1)
    z = b.gen_scalar(b.SEED_SCALARS, 424299)
    from svgpu import encoding as enc
    gen = enc.bases_array([b.G1_GEN])
    srs, sp = np.zeros((n, 8), np.uint64), 1
    for i in range(n):
        srs[i] = oracle_cpp.msm_pippenger(gen, _limbs([sp], CANONICAL), 1).reshape(8)
        sp = sp * s % R
    coeffs = dv.ntt_device(_dev(_limbs(list(evals), MONTGOMERY), gpu), inverse=True)
    assert _same(coeffs, a, MONTGOMERY)
    with svgpu.ResidentBases(srs) as rs:
        C = rs.msm_device(coeffs)
        v, pi = rs.open_device(coeffs, z)
    assert v == _horner(list(a), z)[1]
    assert C == b.g1_mul(b.G1_GEN, _horner(list(a), s)[1])
    dk = svgpu.KzgDecidingKey(b.G1_GEN, b.G2_GEN, b.g2_mul(b.G2_GEN, s))
    lhs = b.g1_add(b.g1_add(C, b.g1_neg(b.g1_mul(b.G1_GEN, v))), b.g1_mul(pi, z))
    assert svgpu.KzgAs.first_failure(dk, [svgpu.KzgAccumulator(lhs, pi)]) == -1
    js = [1, n // 2 + 1, n - 1]
    got = dv.poly_eval_points_device([coeffs], [pow(w, j, R) for j in js])
    assert got == [[evals[j] for j in js]]
