"""SHPLONK (bdfg21) opening on a resident base set, and the multi-point pass under it (one GPU).

Part 1, per size n = 2^k (default 16, 18, 20), m (default 4, 16) and K (default 1, 2, 3, 4), PASSES
interleaved passes of
  (p)  one sv_bn254_fr_poly_eval_points_device call: m polynomials at K points, each read once
  (s)  K evaluate-only sv_bn254_fr_poly_combine_eval_device calls, one per point: what a caller had
       before (that entry point and its kernel are as they were)
Part 2, at n = 2^LOG (default 20) with 16 polynomials in three sets of 1, 2 and 3 points (8 + 5 + 3
polynomials, 27 queries over three shifts):
  (o)  the whole opening: Bdfg21Opening (the evaluations), quotient (W), witness (W')
  (e) (q) (w)  its three steps alone
  (g)  svgpu.gwc19_open over the same queries: another protocol for the same job, three MSMs
  (2m) the two witness MSMs alone over scalars of the same lengths: the floor of (o)
  (c1) the three combinations c_i alone, (dv) the divisions by 1, 2 and 3 roots alone
each the median of REPS calls after WARMUP; the spread of every column over the passes is printed.
Before anything is timed the multi-point evaluations are compared with the single-point passes', and
the opening's evaluations with those.

  python tools/shplonk_open_bench.py [--log-n 16 18 20] [--m 4 16] [--k 1 2 3 4] [--open-log-n 20]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from svgpu import encoding as enc  # noqa: E402
from svgpu import loader  # noqa: E402

SEED_B, SEED_S = 0x5EEDBA5E5, 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY
Z = 0x1D0F5A17C3B2A49587766554433221100FFEEDDCCBBAA998877665544332211 % enc.R
CH = [pow(Z, e, enc.R) for e in (3, 5, 7, 11, 13)]  # mu, gamma, z', and two shifts


def med_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall)


def table(tag, run, passes, reps, warmup):
    cols = {k: [] for k in run}
    for ps in range(passes):
        for k in run:
            cols[k].append(med_ms(run[k], reps, warmup))
        print(f"{tag} pass {ps} wall ms: " + "  ".join(f"({k}) {cols[k][-1]:.3f}" for k in run))
    med = {k: statistics.median(cols[k]) for k in run}
    print(f"{tag} spread over the passes (max - min, ms): "
          + "  ".join(f"({k}) {max(cols[k]) - min(cols[k]):.3f}" for k in run))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 18, 20])
    ap.add_argument("--m", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 3, 4])
    ap.add_argument("--open-log-n", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery passes={args.passes} reps={args.reps} warmup={args.warmup}")
    points = [Z] + [Z * c % enc.R for c in CH]

    for lg in args.log_n:
        n = 1 << lg
        every = [dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, (j + 1) * n, FORM) for j in range(max(args.m))]
        torch.cuda.synchronize()
        for m in args.m:
            polys = every[:m]
            for K in args.k:
                xs = points[:K]
                single = [dv.poly_combine_eval_device(polys, x, 1, form=FORM, combined=False)[0] for x in xs]
                assert dv.poly_eval_points_device(polys, xs, form=FORM) == [list(c) for c in zip(*single)], \
                    f"2^{lg} m={m} K={K}: the multi-point pass disagrees with the single-point passes"
                run = {
                    "p": lambda: dv.poly_eval_points_device(polys, xs, form=FORM),
                    "s": lambda: [dv.poly_combine_eval_device(polys, x, 1, form=FORM, combined=False) for x in xs],
                }
                med = table(f"2^{lg} m={m} K={K}", run, args.passes, args.reps, args.warmup)
                print(f"2^{lg} m={m} K={K}: (p) {med['p']:.3f} ms; (s) {med['s']:.3f} ms = {med['s'] / K:.3f} per point; "
                      f"(s)/(p) = {med['s'] / med['p']:.2f}")
        del every

    lg = args.open_log_n
    n = 1 << lg
    dB = dv.gen_bases(dv.empty_bases(n, dev), SEED_B, 0, FORM)
    rset = loader.ResidentBases.from_device(dB, FORM)
    del dB
    polys = [dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, (j + 1) * n, FORM) for j in range(16)]
    w1, w2 = CH[3], CH[4]
    groups = [(range(0, 8), [1]), (range(8, 13), [1, w1]), (range(13, 16), [1, w1, w2])]
    queries = [(p, s) for members, shifts in groups for p in members for s in shifts]
    mu, gamma, zp = CH[:3]
    op = svgpu.Bdfg21Opening(rset, polys, queries, Z, form=FORM)
    want = [dv.poly_combine_eval_device([polys[p]], s * Z % enc.R, 1, form=FORM, combined=False)[0][0] for p, s in queries]
    assert op.evals == want, "the opening's evaluations disagree with the single-point passes"
    assert svgpu.gwc19_open(rset, polys, queries, Z, mu, form=FORM)[0] == want
    first = (op.quotient(mu, gamma), op.witness(zp))
    assert first == svgpu.bdfg21_open(rset, polys, queries, Z, (mu, gamma, zp), form=FORM)[1:]
    scal = polys[0]
    dC = torch.empty((n, 4), dtype=torch.int64, device=dev)
    dQ = torch.empty((n, 4), dtype=torch.int64, device=dev)
    run = {
        "o": lambda: svgpu.bdfg21_open(rset, polys, queries, Z, (mu, gamma, zp), form=FORM),
        "e": lambda: svgpu.Bdfg21Opening(rset, polys, queries, Z, form=FORM),
        "q": lambda: op.quotient(mu, gamma),
        "w": lambda: op.witness(zp),
        "g": lambda: svgpu.gwc19_open(rset, polys, queries, Z, mu, form=FORM),
        "2m": lambda: (rset.msm_device(scal[:n - 1], 0, FORM), rset.msm_device(scal[1:], 0, FORM)),
        "c1": lambda: [dv.poly_combine_eval_device([polys[p] for p in members], 0, mu, form=FORM, out=dC)
                       for members, _ in groups],
        "dv": lambda: [dv.poly_div_roots_device(scal, [s * Z % enc.R for s in shifts], form=FORM, out=dQ)
                       for _, shifts in groups],
    }
    med = table(f"2^{lg} open", run, args.passes, args.reps, args.warmup)
    print(f"2^{lg} open: (o) {med['o']:.3f} ms = (e) {med['e']:.3f} + (q) {med['q']:.3f} + (w) {med['w']:.3f}; "
          f"(g) {med['g']:.3f} ms, (g)/(o) = {med['g'] / med['o']:.2f}; (2m) {med['2m']:.3f} ms, "
          f"(o) - (2m) = {med['o'] - med['2m']:.3f} ms: evaluations {med['e']:.3f}, combinations {med['c1']:.3f}, "
          f"divisions {med['dv']:.3f}, the rest (h, L, its division) "
          f"{med['o'] - med['2m'] - med['e'] - med['c1'] - med['dv']:.3f}")
    rset.close()


if __name__ == "__main__":
    main()
