"""The extended-domain round trip on the device (sv_bn254_fr_coset_lde_device,
sv_bn254_fr_quotient_coeffs_device), one GPU.

LDE, per (k, e, count) (default (16,2,1) (20,2,1) (20,2,8) (22,2,1)): the fused call against the
composition a caller had to write from the NTT alone -- zero a padded buffer of count 2^K elements,
copy the coefficients in, ntt_device(shift=g) at K = k + e -- with the composition's three steps also
timed apart.  Quotient, per (k, e, pieces) (default (20,2,3) (22,2,3)): the call against the inverse
coset ntt_device alone at K, which is a floor under any composition (the library has no Fr product
to divide with, and the floor neither divides nor truncates).

Each figure is the median (min .. max) of REPS calls after WARMUP, from HIP events on the call's
stream (a side stream made current, so the library and torch's fill and copy work on that stream and
the events bracket them, the flag read-back included) and, beside it, the wall time.  Before
anything is timed the fused LDE is compared with the composition bit for bit; the quotient's full
output h (all 2^e pieces) goes forward through the coset ntt_device, and h(g w^j) t(g w^j) is
compared with numer[j] at four rows in Python-int arithmetic; the cut call must equal h's head.

MODEL columns (computed from the plan, not measured; Montgomery form): Fr products per call / 130 G
products/s and HBM bytes / 8 TB/s, the figures DESIGN.md uses.  Per element of the 2^K image and
pass: (w - 1) / 2 products for the radix-2 stages, one (K <= 13) or two for the twiddle of every
pass but the last, two for a coset power.  The LDE's pass 0 skips, in stage i of its first
z = min(e, w_0), the 1 - 2^-(z - 1 - i) share of butterflies whose inputs are both padding, and puts
the two coset products on live elements only; the quotient adds one table product per element on
the way in to the coset inverse's two on the way out.

  python tools/extended_bench.py [--lde 16,2,1 20,2,1 ...] [--quotient 20,2,3 ...] [--reps 20] [--warmup 3]
"""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from svgpu import encoding as enc  # noqa: E402

SEED_S = 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY
R = enc.R
ZETA = pow(7, (R - 1) // 3, R)   # halo2's Fr::ZETA, the coset a halo2 prover uses
PRODUCTS_PER_S, HBM_BYTES_PER_S = 130e9, 8e12
T = int(re.search(r"constexpr uint32_t kNttTileLog = (\d+);",
                  open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "ntt.hpp")).read()).group(1))


def widths(k, t=T):
    p = -(-k // t)
    return [k // p + (1 if s < k % p else 0) for s in range(p)] if k else [0]


def model_lde(k, e, count):
    """(products, bytes) of the fused call and of the composition's transform."""
    K = k + e
    ws = widths(K)
    tw = 2 if K > 13 else 1
    N = count << K
    full = (sum((w - 1) / 2 for w in ws) + (len(ws) - 1) * tw + 2) * N
    z = min(e, ws[0])
    # pass 0: stage i of the top z runs 2^-(z - 1 - i) of its butterflies (half a product per element each)
    saved = sum(0.5 * (1 - 2.0 ** -(z - 1 - i)) for i in range(z) if ws[0] - 1 - i > 0) * N
    fused = full - saved - 2 * (N - (count << k))
    nbytes = len(ws) * 64 * N
    return (fused, nbytes - 32 * (N - (count << k))), (full, nbytes + 32 * N + 64 * (count << k))


def model_quot(k, e, pieces):
    K = k + e
    ws = widths(K)
    tw = 2 if K > 13 else 1
    N = 1 << K
    base = (sum((w - 1) / 2 for w in ws) + (len(ws) - 1) * tw + 2) * N
    nbytes = len(ws) * 64 * N
    return (base + N, nbytes - 32 * (N - (pieces << k))), (base, nbytes)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
    return out


def report(label, samples, model=None):
    ev = sorted(s[1] for s in samples)
    wall = statistics.median(s[0] for s in samples)
    tail = ""
    if model is not None:
        tail = (f" | MODEL products {model[0] / PRODUCTS_PER_S * 1e6:8.1f} us  "
                f"MODEL bytes {model[1] / HBM_BYTES_PER_S * 1e6:7.1f} us")
    print(f"{label:<52} events {statistics.median(ev) * 1e3:9.1f} us ({ev[0] * 1e3:.1f} .. {ev[-1] * 1e3:.1f})  "
          f"wall {wall * 1e3:9.1f} us{tail}", flush=True)
    return statistics.median(ev), ev[0], ev[-1]


def ratio(label, a, b):
    print(f"{label}: {a[0] / b[0]:.3f}  (medians {a[0] * 1e3:.1f} / {b[0] * 1e3:.1f} us; "
          f"spreads {a[1] * 1e3:.1f} .. {a[2] * 1e3:.1f} and {b[1] * 1e3:.1f} .. {b[2] * 1e3:.1f})", flush=True)


def to_int(row):
    return enc.limbs_to_int(list(row.cpu().numpy().view(np.uint64)))


def bench_lde(k, e, count, dev, reps, warmup):
    n, K = 1 << k, k + e
    N = 1 << K
    x = dv.gen_scalars(dv.empty_scalars(count * n, dev), SEED_S, 0, FORM).reshape(count, n, 4)
    y = torch.empty((count, N, 4), dtype=torch.int64, device=dev)
    padded = torch.empty((count, N, 4), dtype=torch.int64, device=dev)
    y2 = torch.empty_like(y)

    def compose():
        padded.zero_()
        padded[:, :n].copy_(x)
        dv.ntt_device(padded, form=FORM, shift=ZETA, out=y2)

    dv.coset_lde_device(x, e, shift=ZETA, form=FORM, out=y)
    compose()
    assert torch.equal(y, y2), f"({k},{e},{count}): the fused call differs from the composition"
    tag = f"LDE ({k},{e},{count}) [{'+'.join(map(str, widths(K)))}]"
    mf, mc = model_lde(k, e, count)
    f = report(f"{tag} fused", timed(lambda: dv.coset_lde_device(x, e, shift=ZETA, form=FORM, out=y), reps, warmup), mf)
    c = report(f"{tag} zero + copy + ntt_device", timed(compose, reps, warmup), mc)
    report(f"{tag}   zero alone", timed(lambda: padded.zero_(), reps, warmup))
    report(f"{tag}   copy alone", timed(lambda: padded[:, :n].copy_(x), reps, warmup))
    report(f"{tag}   ntt_device alone", timed(lambda: dv.ntt_device(padded, form=FORM, shift=ZETA, out=y2), reps, warmup))
    ratio(f"{tag} fused / composition", f, c)


def bench_quotient(k, e, pieces, dev, reps, warmup):
    n, K = 1 << k, k + e
    N = 1 << K
    numer = dv.gen_scalars(dv.empty_scalars(N, dev), SEED_S, 7, FORM)
    out = torch.empty((pieces * n, 4), dtype=torch.int64, device=dev)
    y = torch.empty_like(numer)
    # correctness first: h = the call's output (all 2^e pieces) must evaluate, on the coset, to
    # numer / t at sampled points: LDE-free, through the forward coset NTT of the full h
    h = dv.quotient_coeffs_device(numer, k, 1 << e, ZETA, form=FORM)
    ev = dv.ntt_device(h, form=FORM, shift=ZETA)
    gn, we = pow(ZETA, n, R), svgpu.root_of_unity(e)
    for j in (0, 1, N // 2 + 3, N - 1):
        t = (gn * pow(we, j % (1 << e), R) - 1) % R
        assert to_int(ev[j]) * t % R == to_int(numer[j]), f"({k},{e}): h(g w^{j}) t != numer[{j}]"
    dv.quotient_coeffs_device(numer, k, pieces, ZETA, form=FORM, out=out)
    assert torch.equal(out, h[:pieces * n]), f"({k},{e},{pieces}): the cut differs from the full quotient"
    del h, ev
    tag = f"quotient ({k},{e},{pieces}) [{'+'.join(map(str, widths(K)))}]"
    mq, mf = model_quot(k, e, pieces)
    q = report(f"{tag} quotient_coeffs",
               timed(lambda: dv.quotient_coeffs_device(numer, k, pieces, ZETA, form=FORM, out=out), reps, warmup), mq)
    f = report(f"{tag} floor: inverse coset ntt_device",
               timed(lambda: dv.ntt_device(numer, form=FORM, shift=ZETA, inverse=True, out=y), reps, warmup), mf)
    ratio(f"{tag} quotient / floor", q, f)


def triples(values):
    return [tuple(int(v) for v in s.split(",")) for s in values]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lde", nargs="*", default=["16,2,1", "20,2,1", "20,2,8", "22,2,1"])
    ap.add_argument("--quotient", nargs="*", default=["20,2,3", "22,2,3"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery shift=ZETA tile log {T} reps={args.reps} warmup={args.warmup}")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    for k, e, count in triples(args.lde):
        bench_lde(k, e, count, dev, args.reps, args.warmup)
        torch.cuda.empty_cache()
    for k, e, pieces in triples(args.quotient):
        bench_quotient(k, e, pieces, dev, args.reps, args.warmup)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
