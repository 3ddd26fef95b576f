"""Batched KZG opening on a resident base set against m single openings (one GPU).

Per size n = 2^k (default 16, 18, 20) and batch m (default 1, 4, 16, 64), PASSES interleaved passes of
  (a)  m sequential sv_bn254_kzg_open_device calls, one per polynomial: what a caller with m
       polynomials in HBM had before (that entry point and its kernels are as they were, so this is
       the earlier figure, measured in the same run); the host-side fold of the m witnesses is not
       counted
  (b)  one sv_bn254_kzg_open_batch_device call over the same m polynomials
  (c)  the witness MSM alone: sv_bn254_g1_msm_bases_device over the n - 1 quotient scalars in HBM
  (d)  sv_bn254_fr_poly_combine_eval_device alone, with d_combined (d comb) and without (d eval): HIP
       events on the stream around the call (table copy + the two kernels + the read-back)
  copy a plain elementwise kernel over n x 32 B (one read, one write), HIP events: the bandwidth the
       pass's traffic floor is taken at -- m x 32 B read and 32 B written per coefficient
each the median of REPS calls after WARMUP.  Printed at the end per (n, m): (b) against (a), (b) - (c),
(d) against its floor and against the product count, and the spread of every column over the passes.
Before anything is timed the inputs are checked: the first and the last polynomial's evaluation against
a Python-int Horner, sampled rows of the combination against Python ints, every evaluation of the batch
against the single openings', and the batch's witness against the MSM over the quotient of (d)'s
combination.

  python tools/kzg_open_batch_bench.py [--log-n 16 18 20] [--m 1 4 16 64] [--passes 3] [--reps 15]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from svgpu import encoding as enc  # noqa: E402
from svgpu import loader  # noqa: E402

SEED_B, SEED_S = 0x5EEDBA5E5, 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY  # halo2curves' in-memory layout: what the Rust shim passes
Z = 0x1D0F5A17C3B2A49587766554433221100FFEEDDCCBBAA998877665544332211 % enc.R
V = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % enc.R
RINV = pow(1 << 256, -1, enc.R)
# field products per coefficient of the pass: the Horner step, the tree's share, the combination
PRODUCTS_EVAL, PRODUCTS_COMBINE = 1.25, 2.25


def med_ms(fn, reps, warmup):
    """(median wall ms, median HIP-event ms on the current stream) of fn, which synchronises."""
    for _ in range(warmup):
        fn()
    wall, evs = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        evs.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(evs)


def mont_ints(limbs):
    """Montgomery limbs (k, 4) u64 -> canonical Python ints."""
    raw = np.ascontiguousarray(limbs).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * RINV % enc.R for i in range(0, len(raw), 32)]


def horner_eval(limbs_mont, z):
    raw = limbs_mont.tobytes()
    h = 0
    for i in range(len(raw) - 32, -1, -32):
        h = (int.from_bytes(raw[i:i + 32], "little") + z * h) % enc.R
    return h * RINV % enc.R  # the coefficients carry one factor 2^256


def check(rset, polys, n, lg, m):
    """The inputs and every path that is timed, against Python ints and against each other."""
    singles = [rset.open_device(p, Z, 0, FORM) for p in polys]
    for j in sorted({0, m - 1}):
        assert singles[j][0] == horner_eval(polys[j].cpu().numpy().view(np.uint64), Z), \
            f"2^{lg} m={m}: p_{j}(z) disagrees with the Python Horner"
    evals, C = dv.poly_combine_eval_device(polys, Z, V, form=FORM)
    assert evals == [s[0] for s in singles], f"2^{lg} m={m}: evaluations disagree with the single openings"
    assert dv.poly_combine_eval_device(polys, Z, V, form=FORM, combined=False)[0] == evals
    rows = sorted({0, 1, n // 3, n // 2 + 1, n - 2, n - 1})
    idx = torch.tensor(rows, device=C.device)
    got = mont_ints(C[idx].cpu().numpy().view(np.uint64))
    cols = [mont_ints(p[idx].cpu().numpy().view(np.uint64)) for p in polys]
    for r, row in enumerate(rows):
        want, vp = 0, 1
        for col in cols:
            want = (want + vp * col[r]) % enc.R
            vp = vp * V % enc.R
        assert got[r] == want, f"2^{lg} m={m}: row {row} of the combination disagrees with Python ints"
    _, Q = dv.poly_div_linear_device(C, Z, FORM)
    ref = (evals, rset.msm_device(Q, 0, FORM))
    assert rset.open_batch_device(polys, Z, V, 0, FORM) == ref, f"2^{lg} m={m}: the batched opening disagrees"
    return Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--m", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery passes={args.passes} reps={args.reps} warmup={args.warmup}")
    # a stream of its own: the library then works on this stream (not on one from its pool), so the
    # events below bracket its kernels
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    for lg in args.log_n:
        n = 1 << lg
        dB = dv.gen_bases(dv.empty_bases(n, dev), SEED_B, 0, FORM)
        rset = loader.ResidentBases.from_device(dB, FORM)
        del dB
        src = dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, 0, FORM)
        dst = torch.empty_like(src)
        mmax = max(args.m)
        every = [dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, (j + 1) * n, FORM) for j in range(mmax)]
        torch.cuda.synchronize()

        def copy_kernel():
            torch.add(src, 1, out=dst)
            torch.cuda.synchronize()

        for m in args.m:
            polys = every[:m]
            dQ = check(rset, polys, n, lg, m)
            dC = torch.empty((n, 4), dtype=torch.int64, device=dev)
            run = {
                "a": lambda: [rset.open_device(p, Z, 0, FORM) for p in polys],
                "b": lambda: rset.open_batch_device(polys, Z, V, 0, FORM),
                "c": lambda: rset.msm_device(dQ, 0, FORM),
                "d comb": lambda: dv.poly_combine_eval_device(polys, Z, V, form=FORM, out=dC),
                "d eval": lambda: dv.poly_combine_eval_device(polys, Z, V, form=FORM, combined=False),
                "copy": copy_kernel,
            }
            cols = {k: [] for k in run}
            for ps in range(args.passes):
                for k in run:
                    cols[k].append(med_ms(run[k], args.reps, args.warmup))
                print(f"2^{lg} m={m} pass {ps} wall ms: " + "  ".join(f"({k}) {cols[k][-1][0]:.3f}" for k in run))
                print(f"2^{lg} m={m} pass {ps} event ms: " + "  ".join(f"({k}) {cols[k][-1][1]:.3f}" for k in run))
            wall = {k: statistics.median(v[0] for v in cols[k]) for k in run}
            evt = {k: statistics.median(v[1] for v in cols[k]) for k in run}
            spread = {k: max(v[0] for v in cols[k]) - min(v[0] for v in cols[k]) for k in run}
            bw = 2 * n * 32 / (evt["copy"] * 1e-3)  # bytes per second of the copy kernel
            floor = (m + 1) * 32 * n / bw * 1e3
            tag = f"2^{lg} m={m}:"
            print(f"{tag} spread over the passes (max - min, wall ms): "
                  + "  ".join(f"({k}) {spread[k]:.3f}" for k in run))
            print(f"{tag} (a) {wall['a']:.3f} ms = {wall['a'] / m:.3f} per opening; (b) {wall['b']:.3f} ms; "
                  f"(a)/(b) = {wall['a'] / wall['b']:.2f}; (b) - (c) = {wall['b'] - wall['c']:+.3f} ms "
                  f"((c) {wall['c']:.3f})")
            print(f"{tag} copy kernel {evt['copy'] * 1e3:.1f} us = {bw / 1e12:.2f} TB/s; pass floor "
                  f"({(m + 1) * 32} B per coefficient) {floor * 1e3:.1f} us")
            for k, per in (("d comb", PRODUCTS_COMBINE), ("d eval", PRODUCTS_EVAL)):
                f = floor if k == "d comb" else m * 32 * n / bw * 1e3
                print(f"{tag} ({k}) {evt[k] * 1e3:.1f} us events ({wall[k] * 1e3:.1f} us wall) = {evt[k] / f:.2f} x "
                      f"floor; {per} products per coefficient -> {per * m * n / (evt[k] * 1e-3) / 1e9:.1f} G products/s")
            del dQ, dC
        rset.close()
        del every, src, dst


if __name__ == "__main__":
    main()
