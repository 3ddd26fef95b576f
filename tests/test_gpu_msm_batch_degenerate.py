"""Degenerate additions through every route of the batched small MSMs (the msm_batch.hip table of
tests/COVERAGE.md): the batch cases of tests/degenerate_cases.py -- bucket sums of a window all
equal or alternating (the suffix scan doubles or cancels at every step), window sums and single
bucket sums that are +-2^c times the one above (the Horners' addition after the c doublings meets
a == b and a == -b), a quad's partial sums equal or opposite -- and the 8 MSMs of
test_gpu_msm_batch.py::test_edge_suite_per_msm, whose own route is k_batch_uwin alone.
tests/test_degenerate_cases.py proves on the CPU which operand classes each case brings.

A batch pads the degenerate MSMs with random 3-term ones up to the count its route needs and puts
degenerate MSMs at index 0, 15, 16, 17 (a quad and a wave boundary of k_msm_batch_horner_q) and at the
last index, so a 16-quad wave holds degenerate and generic MSMs side by side.  Every output row is
compared: the closed form ((sum s_i m_i) mod r) P for a lattice MSM, the Python group law for an
edge MSM, the oracle's Pippenger for a padding row.
"""
import numpy as np
import pytest
import torch

import degenerate_cases as dc
from oracle import bn254 as b

pytestmark = pytest.mark.gpu

_CACHE = {}


def _slots(count, k):
    """k distinct batch positions: 0, 15, 16, 17, count - 1 first, the others spread over the batch."""
    out = [p for p in (0, 15, 16, 17, count - 1) if 0 <= p < count]
    out = list(dict.fromkeys(out))[:k]
    step = max(1, (count - 1) // max(1, k))
    for p in list(range(7 % count, count, step)) + list(range(count)):
        if len(out) == k:
            break
        if p not in out:
            out.append(p)
    return out


def _batch(oracle_cpp, c, count):
    """(bases, scalars, offsets, expected rows, table rows, row indices) of the batch at width c."""
    key = (c, count)
    if key in _CACHE:
        return _CACHE[key]
    from svgpu import encoding as enc
    lat = dc.lattice()
    special = []  # (base rows, scalar ints, expected point)
    for _, terms in dc.batch_msms(c):
        special.append((lat.rows_of([m for _, m in terms]), [s for s, _ in terms],
                        lat.point(sum(s * m for s, m in terms))))
    for pairs in dc.edge_msms():
        special.append((dc.point_rows([q for _, q in pairs]), [s for s, _ in pairs],
                        b.native_msm([s for s, _ in pairs], [q for _, q in pairs])))
    assert count >= len(special)
    where = dict(zip(_slots(count, len(special)), special))
    npad = count - len(special)
    PB = oracle_cpp.gen_bases(b.SEED_BASES, 3 * npad, start=31337)
    PS = oracle_cpp.gen_scalars(b.SEED_SCALARS, 3 * npad, start=31337)
    B, S, off, exp, k = [], [], [0], [], 0
    for i in range(count):
        if i in where:
            rows, sc, want = where[i]
            B.append(rows)
            S.append(enc.scalars_array(sc))
        else:
            B.append(PB[3 * k:3 * k + 3])
            S.append(PS[3 * k:3 * k + 3])
            want = b.g1_from_bytes(oracle_cpp.msm_pippenger(B[-1], S[-1], 1).tobytes())
            k += 1
        off.append(off[-1] + B[-1].shape[0])
        exp.append(want)
    B, S = np.ascontiguousarray(np.concatenate(B)), np.ascontiguousarray(np.concatenate(S))
    # the same batch over a table of its distinct rows (the indexed entry point)
    table, idx = np.unique(B, axis=0, return_inverse=True)
    _CACHE[key] = (B, S, off, exp, np.ascontiguousarray(table), idx.reshape(-1).astype(np.int32))
    return _CACHE[key]


def _rows_to_points(out, form):
    from svgpu import encoding as enc
    return [enc.g1_from_limbs(r, form) for r in out.cpu().numpy().view(np.uint64)]


def _device_batch(gpu, oracle_cpp, c, count, montgomery=False):
    import svgpu
    from svgpu import device as dv, encoding as enc
    B, S, off, exp, _, _ = _batch(oracle_cpp, c, count)
    form = svgpu.SV_CANONICAL
    if montgomery:
        form = svgpu.SV_MONTGOMERY
        key = ("mont", c, count)
        if key not in _CACHE:
            _CACHE[key] = (enc.bases_array([enc.g1_from_limbs(r) for r in B], form),
                           enc.scalars_array([enc.limbs_to_int(r) for r in S], form))
        B, S = _CACHE[key]
    out = dv.msm_batch(torch.from_numpy(B.view(np.int64)).to(gpu), torch.from_numpy(S.view(np.int64)).to(gpu),
                       torch.tensor(off, dtype=torch.int64, device=gpu), int(max(np.diff(off))), form)
    torch.cuda.synchronize()
    got = _rows_to_points(out, form)
    bad = [i for i in range(count) if got[i] != exp[i]]
    assert not bad, bad


def test_uwin_host_and_device_api(gpu, oracle_cpp):
    """k_batch_uwin + the host Horner: at most 64 MSMs of at most 256 terms, host arrays and device
    buffers (the host API keeps batches of more than 4 MSMs in one batch call)."""
    import svgpu
    B, S, off, exp, _, _ = _batch(oracle_cpp, 5, 24)
    assert svgpu.msm_batch_arrays(B, S, off) == exp
    _device_batch(gpu, oracle_cpp, 5, 24)
    _device_batch(gpu, oracle_cpp, 5, 24, montgomery=True)


@pytest.mark.parametrize("bw", ["1", "26"])
def test_fused(gpu, oracle_cpp, monkeypatch, bw):
    """k_batch_fused at 65 MSMs (bucket_sum_q's quad additions, horner_msm<true>'s bucket-wise Horner
    and its scan and tree), one and 26 bucket waves an MSM."""
    monkeypatch.setenv("SVGPU_BATCH_BW", bw)
    _device_batch(gpu, oracle_cpp, 5, 65)


@pytest.mark.parametrize("count,fuse", [(513, None), (65, "0")])
def test_buckets_then_horner(gpu, oracle_cpp, monkeypatch, count, fuse):
    """k_batch_buckets_q + k_batch_horner_b: above 512 MSMs, and under SVGPU_BATCH_FUSE=0."""
    if fuse is not None:
        monkeypatch.setenv("SVGPU_BATCH_FUSE", fuse)
    _device_batch(gpu, oracle_cpp, 5, count)


def test_windows_q_then_horner_q5(gpu, oracle_cpp, monkeypatch):
    """SVGPU_BATCH_BUCKETS=0: k_batch_windows_q (quad_madd_2p chains, the scan and tree per window) +
    k_msm_batch_horner_q<5> (16 MSMs a wave: degenerate and generic quads side by side)."""
    monkeypatch.setenv("SVGPU_BATCH_BUCKETS", "0")
    _device_batch(gpu, oracle_cpp, 5, 65)
    _device_batch(gpu, oracle_cpp, 5, 65, montgomery=True)


@pytest.mark.parametrize("c", [5, 8])
@pytest.mark.parametrize("quad", ["0", "1"])
def test_lane_windows_both_horners(gpu, oracle_cpp, monkeypatch, c, quad):
    """k_msm_batch_windows<5 / 8> (per-lane bucket chains, smul_small, the xor-shuffle fold) with
    k_msm_batch_horner<c> (par_add, par_dbl: SVGPU_BATCH_QUAD=0) and k_msm_batch_horner_q<c>; the
    window-8 batch holds the window-8 version of every case (T_w = +-256 T_(w+1)), both forms.
    (Window 5 with the quad path on is k_batch_fused again: covered above, so c = 5 runs it with
    more than 256 terms in one MSM instead, which keeps k_msm_batch_windows<5>.)"""
    monkeypatch.setenv("SVGPU_BATCH_WINDOW_BITS", str(c))
    monkeypatch.setenv("SVGPU_BATCH_QUAD", quad)
    if c == 5 and quad == "1":
        _long_msm_batch(gpu, oracle_cpp)
        return
    _device_batch(gpu, oracle_cpp, c, 65)
    _device_batch(gpu, oracle_cpp, c, 65, montgomery=True)


def _long_msm_batch(gpu, oracle_cpp):
    """65 MSMs, one of them 300 terms (300 copies of one lattice term: max_terms > 256 leaves the quad
    windows): k_msm_batch_windows<5> + k_msm_batch_horner_q<5>."""
    import svgpu
    from svgpu import device as dv
    lat = dc.lattice()
    B, S, off, exp, _, _ = _batch(oracle_cpp, 5, 64)
    s = 7 << 15
    B2 = np.concatenate([B, np.tile(lat.rows_of([1]), (300, 1))])
    S2 = np.concatenate([S, np.tile(dc.scalar_rows([7], [15]), (300, 1))])
    off2 = off + [off[-1] + 300]
    out = dv.msm_batch(torch.from_numpy(B2.view(np.int64)).to(gpu), torch.from_numpy(S2.view(np.int64)).to(gpu),
                       torch.tensor(off2, dtype=torch.int64, device=gpu), 300, svgpu.SV_CANONICAL)
    torch.cuda.synchronize()
    assert _rows_to_points(out, svgpu.SV_CANONICAL) == exp + [lat.point(300 * s)]


def test_indexed_device_entry(gpu, oracle_cpp):
    """sv_bn254_g1_msm_batch_indexed_device: the same 65 MSMs as rows of a table (k_batch_prep's
    lookup, then the fused route) and as 24 (no host route for an indexed batch: fused again)."""
    import svgpu
    from svgpu import device as dv
    for count in (65, 24):
        _, S, off, exp, table, idx = _batch(oracle_cpp, 5, count)
        out = dv.msm_batch_indexed(torch.from_numpy(table.view(np.int64)).to(gpu), torch.from_numpy(idx).to(gpu),
                                   torch.from_numpy(S.view(np.int64)).to(gpu),
                                   torch.tensor(off, dtype=torch.int64, device=gpu), int(max(np.diff(off))),
                                   svgpu.SV_CANONICAL, svgpu.SV_CANONICAL)
        torch.cuda.synchronize()
        assert _rows_to_points(out, svgpu.SV_CANONICAL) == exp


def test_fixed_table_host_and_device(gpu):
    """k_msm_batch_fixed over the rows {P, 2^8 P, 2^16 P, -(2^8 P), identity, Q}: Q_1(P) == Q_0(2^8 P)
    though no row repeats, so coinciding and opposite table points meet in one of the 128 buckets
    (the two threads of a bucket, the chain of one thread) and neighbouring S_b are equal or
    opposite in the 7-level scan."""
    import svgpu
    from svgpu import encoding as enc
    pts, mults = dc.fixed_table()
    lat = dc.lattice()
    msms = [terms for _, terms in dc.fixed_msms()]
    names = [name for name, _ in dc.fixed_msms()]
    exp = []
    for terms in msms:
        kp = sum(s * mults[r] for s, r in terms if mults[r] is not None)
        kq = sum(s for s, r in terms if mults[r] is None)
        exp.append(b.g1_add(lat.point(kp), b.g1_mul(pts[5], kq)))
    with svgpu.BaseTable(dc.point_rows(pts)) as tab:
        got = tab.batch_multi_scalar_multiplication(msms)
        assert [n for n, g, e in zip(names, got, exp) if g != e] == []
        idx = torch.tensor([r for t in msms for _, r in t], dtype=torch.int32, device=gpu)
        off = torch.tensor(np.cumsum([0] + [len(t) for t in msms]), dtype=torch.int64, device=gpu)
        for form in (svgpu.SV_CANONICAL, svgpu.SV_MONTGOMERY):
            S = torch.from_numpy(enc.scalars_array([s for t in msms for s, _ in t], form).view(np.int64)).to(gpu)
            out = tab.msm_batch_device(idx, S, off, form)
            torch.cuda.synchronize()
            got = _rows_to_points(out, form)
            assert [n for n, g, e in zip(names, got, exp) if g != e] == []
