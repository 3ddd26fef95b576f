"""Every branch of msm_batch_device's dispatch (csrc/msm_batch.hip) against the C++ oracle, one
MSM at a time and bit for bit:

  count <= 64 (kBatchHostMax)          window sums on the device, Horners on the host
  count <= 512 (kFuseMax), slot free   k_batch_fused
  count <= 4096, or the slot is held   k_batch_buckets_q + k_batch_horner_b
  count  > 4096                        k_batch_windows_q + k_msm_batch_horner_q<5>
  max_terms > 256 (kQMaxTerms)         k_msm_batch_windows<8> + k_msm_batch_horner_q<8>

and the documented fallbacks SVGPU_BATCH_FUSE=0, SVGPU_BATCH_BUCKETS=0, SVGPU_BATCH_QUAD=0 (the
one-wave Horner k_msm_batch_horner<5> / <8>) and SVGPU_BATCH_BW (bucket blocks per MSM of the fused
launch).  All these switches are read per call.

One master batch of 4097 MSMs serves every count: the batch of `count` MSMs is its prefix, so the
oracle runs once.  Almost all MSMs have 1-4 terms; every 257th, MSM 0 and MSM 4096 have 255 or 256."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import bn254 as b

pytestmark = pytest.mark.gpu

_CACHE = {}


def _limbs(x):
    return np.array([(x >> (64 * i)) & 0xffffffffffffffff for i in range(4)], np.uint64)


def _int(row):
    return sum(int(v) << (64 * i) for i, v in enumerate(row))


def _offsets(sizes):
    off = [0]
    for m in sizes:
        off.append(off[-1] + m)
    return off


def _oracle(oracle_cpp, B, S, off):
    return [b.g1_from_bytes(oracle_cpp.msm_pippenger(B[lo:hi], S[lo:hi], 1).tobytes())
            for lo, hi in zip(off[:-1], off[1:])]


def _batch(oracle_cpp, key, sizes, seed, edit=None):
    """(B, S, off, expected) in canonical limbs, computed once per key and never written again."""
    if key not in _CACHE:
        off = _offsets(sizes)
        B = oracle_cpp.gen_bases(b.SEED_BASES, off[-1], start=seed)
        S = oracle_cpp.gen_scalars(b.SEED_SCALARS, off[-1], start=seed)
        if edit:
            edit(B, S, off)
        exp = _oracle(oracle_cpp, B, S, off)
        for a in (B, S):
            a.setflags(write=False)
        _CACHE[key] = (B, S, off, exp)
    return _CACHE[key]


MASTER = 4097


def _master_sizes():
    sizes = [1 + k % 4 for k in range(MASTER)]
    for k in range(0, MASTER, 257):
        sizes[k] = 255 if (k // 257) % 2 else 256
    sizes[0] = sizes[MASTER - 1] = 256
    return sizes


def _master_edges(B, S, off):
    """The edge MSMs, each an MSM of its own, once near the front (inside every prefix of at least
    65 MSMs) and once past MSM 4000."""
    rm1 = _limbs(b.R - 1)
    for base in (4, 4000):
        k = base + 1                                     # 2 terms: P, -P with one scalar -> identity
        o = off[k]
        assert off[k + 1] - o == 2
        B[o + 1] = B[o]
        B[o + 1, 4:8] = _limbs(b.P - _int(B[o, 4:8]))
        S[o + 1] = S[o]
        k = base + 2                                     # 3 terms: one zero scalar
        S[off[k]] = 0
        k = base + 3                                     # 4 terms: an identity base
        B[off[k] + 1] = 0
        k = base + 5                                     # 2 terms: all scalars zero -> identity
        S[off[k]:off[k + 1]] = 0
        k = base + 7                                     # 4 terms: all-equal r - 1
        S[off[k]:off[k + 1]] = rm1
    S[off[257]:off[258]] = rm1                           # 255 terms: all-equal r - 1, every top digit
    S[off[MASTER - 1]:off[MASTER]] = rm1                 # the last MSM: 256 terms of r - 1


def _master(oracle_cpp):
    return _batch(oracle_cpp, "master", _master_sizes(), 31000, _master_edges)


def _to_form(B, S, form):
    import svgpu
    from svgpu import encoding as enc
    if form == svgpu.SV_CANONICAL:
        return B, S
    return (enc.bases_array([enc.g1_from_limbs(r) for r in B], form),
            enc.scalars_array([enc.limbs_to_int(r) for r in S], form))


def _run_device(gpu, B, S, off, max_terms, form):
    from svgpu import device as dv, encoding as enc
    Bf, Sf = _to_form(B, S, form)
    Bd = torch.from_numpy(np.array(Bf, dtype=np.uint64).view(np.int64)).to(gpu)  # a copy: the cache is read-only
    Sd = torch.from_numpy(np.array(Sf, dtype=np.uint64).view(np.int64)).to(gpu)
    od = torch.tensor(off, dtype=torch.int64, device=gpu)
    out = dv.msm_batch(Bd, Sd, od, max_terms, form)
    torch.cuda.synchronize()
    return [enc.g1_from_limbs(r, form) for r in out.cpu().numpy().view(np.uint64)]


def _run_host(B, S, off, form):
    import svgpu
    Bf, Sf = _to_form(B, S, form)
    return svgpu.msm_batch_arrays(Bf, Sf, off, form)


def _mismatches(got, exp):
    return [k for k, (g, e) in enumerate(zip(got, exp)) if g != e][:8], len(got), len(exp)


@pytest.mark.parametrize("form", ["canonical", "montgomery"])
@pytest.mark.parametrize("entry", ["device", "host"])
def test_more_than_4096_small_msms(gpu, oracle_cpp, entry, form):
    """A1: count = 4097 is past bucket_horner's limit: k_batch_windows_q + k_msm_batch_horner_q<5>,
    a pair of kernels no smaller batch reaches."""
    import svgpu
    f = svgpu.SV_MONTGOMERY if form == "montgomery" else svgpu.SV_CANONICAL
    B, S, off, exp = _master(oracle_cpp)
    assert len(exp) == MASTER and max(hi - lo for lo, hi in zip(off[:-1], off[1:])) == 256
    assert exp[5] is None and exp[9] is None and exp[4001] is None   # P - P and the all-zero MSMs
    got = _run_device(gpu, B, S, off, 256, f) if entry == "device" else _run_host(B, S, off, f)
    assert _mismatches(got, exp) == ([], MASTER, MASTER)


@pytest.mark.parametrize("count", [65, 512, 513, 4096])
def test_count_boundaries(gpu, oracle_cpp, count):
    """A2: the first count on the device side of kBatchHostMax (65), the last fused count (512), the
    first two-kernel count (513: k_batch_buckets_q + k_batch_horner_b from the dispatch itself, not
    from the redo after a timeout) and the last bucket-Horner count (4096)."""
    import svgpu
    B, S, off, exp = _master(oracle_cpp)
    n = off[count]
    got = _run_device(gpu, B[:n], S[:n], off[:count + 1], 256, svgpu.SV_CANONICAL)
    assert _mismatches(got, exp[:count]) == ([], count, count)


@pytest.mark.parametrize("longest", [256, 257])
def test_window_bits_boundary(gpu, oracle_cpp, longest):
    """A2: max_terms 256 is the last batch on the quad path (window 5), 257 the first on window 8."""
    import svgpu
    sizes = [longest, 1, 2, 3, 255] * 14
    B, S, off, exp = _batch(oracle_cpp, ("wb", longest), sizes, 47000 + longest)
    got = _run_device(gpu, B, S, off, longest, svgpu.SV_CANONICAL)
    assert _mismatches(got, exp) == ([], len(sizes), len(sizes))
    assert _run_host(B, S, off, svgpu.SV_CANONICAL) == exp


RAGGED = [1, 2, 3, 31, 32, 33, 64, 65, 255, 256] * 13          # 130 MSMs
RAGGED_W8 = [1, 2, 33, 65, 256, 257, 300, 600] * 5             # 40 MSMs, window 8


@pytest.mark.parametrize("env", [
    {"SVGPU_BATCH_FUSE": "0"},
    {"SVGPU_BATCH_BUCKETS": "0"},
    {"SVGPU_BATCH_QUAD": "0", "SVGPU_BATCH_WINDOW_BITS": "5"},
    {"SVGPU_BATCH_BW": "1"},
    {"SVGPU_BATCH_BW": "2"},
    {"SVGPU_BATCH_BW": "26"},
    {"SVGPU_BATCH_BW": "1000"},
], ids=lambda e: ",".join(f"{k[12:]}={v}" for k, v in e.items()))
def test_fallback_switches(gpu, oracle_cpp, monkeypatch, env):
    """A3: each documented fallback on one ragged 130-MSM batch.  SVGPU_BATCH_HOST_MAX=0 keeps the
    batch on the device whatever its count."""
    import svgpu
    B, S, off, exp = _batch(oracle_cpp, "ragged", RAGGED, 52000)
    monkeypatch.setenv("SVGPU_BATCH_HOST_MAX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert svgpu.msm_batch_arrays(B, S, off) == exp
    got = _run_device(gpu, B, S, off, 256, svgpu.SV_MONTGOMERY)
    assert _mismatches(got, exp) == ([], len(exp), len(exp))


def test_fallback_one_wave_horner_window_8(gpu, oracle_cpp, monkeypatch):
    """A3: SVGPU_BATCH_QUAD=0 at window 8: k_msm_batch_windows<8> + k_msm_batch_horner<8>."""
    import svgpu
    B, S, off, exp = _batch(oracle_cpp, "ragged8", RAGGED_W8, 53000)
    monkeypatch.setenv("SVGPU_BATCH_HOST_MAX", "0")
    monkeypatch.setenv("SVGPU_BATCH_QUAD", "0")
    monkeypatch.setenv("SVGPU_BATCH_WINDOW_BITS", "8")
    assert svgpu.msm_batch_arrays(B, S, off) == exp
    got = _run_device(gpu, B, S, off, 600, svgpu.SV_CANONICAL)
    assert _mismatches(got, exp) == ([], len(exp), len(exp))


def test_two_batches_contend_for_the_fused_slot(gpu, oracle_cpp):
    """A4: two threads issue a 128-MSM batch each on one device at once (ctypes releases the GIL
    around the call).  One fused launch per device is in flight, so whichever call finds the slot
    taken runs k_batch_buckets_q + k_batch_horner_b; the order is left to the scheduler and both
    must return the oracle's results."""
    import svgpu
    batches = [_batch(oracle_cpp, ("pair", j), [64] * 128 if j == 0 else [17, 200, 64, 255] * 32, 61000 + 9000 * j)
               for j in range(2)]

    def job(j):
        B, S, off, exp = batches[j % 2]
        return svgpu.msm_batch_arrays(B, S, off) == exp

    with ThreadPoolExecutor(max_workers=2) as ex:
        results = list(ex.map(job, range(8)))
    assert all(results), results
