"""Resident base sets against the entry points that ship or prepare bases per call (one GPU).

Per size 2^k (default 16, 18, 20), PASSES interleaved passes of
  (a) sv_bn254_g1_msm               host bases + host scalars (96 B per term over PCIe)
  (b) sv_bn254_g1_msm_bases         resident set, host scalars (32 B per term)
  (c) sv_bn254_g1_msm_device        bases + scalars in HBM (per-call base check / conversion / table)
  (d) sv_bn254_g1_msm_bases_device  resident set, scalars in HBM
each the median wall ms of REPS calls after WARMUP, plus the set's create time (host rows and rows
in HBM) and (b) as a multiple of (c).  --sweep adds (b) under other piece schedules (--splits, each an
SVGPU_H2D_SPLIT weight list; "1" is one piece) at the sizes of --sweep-log-n (default: the largest),
interleaved the same way, next to the library's default schedule.  Results of (a)-(d) are checked
to agree before anything is timed.

  python tools/resident_bench.py [--log-n 16 18 20] [--passes 3] [--reps 15] [--sweep [--splits 1 1,1 ...]]
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
from svgpu import loader  # noqa: E402

SEED_B, SEED_S = 0x5EEDBA5E5, 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY  # halo2curves' in-memory layout: what the Rust shim passes


def med_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="piece schedules of (b)")
    ap.add_argument("--splits", nargs="+", default=["1", "1,1", "1,1,1,1", "5,4,4,3", "1,3"])
    ap.add_argument("--sweep-log-n", type=int, nargs="+", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery passes={args.passes} reps={args.reps} warmup={args.warmup}")
    for lg in args.log_n:
        n = 1 << lg
        dB = dv.gen_bases(dv.empty_bases(n, dev), SEED_B, 0, FORM)
        dS = dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, 0, FORM)
        torch.cuda.synchronize()
        hB = dB.cpu().numpy().view(np.uint64)
        hS = dS.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        rset = loader.ResidentBases(hB, form=FORM)
        create_host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        rdev = loader.ResidentBases.from_device(dB, FORM)
        create_dev = (time.perf_counter() - t0) * 1e3
        rdev.close()
        run = {
            "a": lambda: loader.msm_arrays(hB, hS, FORM, 1),
            "b": lambda: rset.msm_arrays(hS, 0, FORM),
            "c": lambda: dv.msm(dB, dS, FORM),
            "d": lambda: rset.msm_device(dS, 0, FORM),
        }
        ref = run["a"]()
        for k in "bcd":
            assert run[k]() == ref, f"2^{lg}: ({k}) disagrees with (a)"
        print(f"2^{lg}: create host rows {create_host:.3f} ms, rows in HBM {create_dev:.3f} ms, "
              f"{rset.device_bytes} B on the device")
        cols = {k: [] for k in "abcd"}
        for ps in range(args.passes):
            for k in "abcd":
                cols[k].append(med_ms(run[k], args.reps, args.warmup))
            print(f"2^{lg} pass {ps}: " + "  ".join(f"({k}) {cols[k][-1]:.3f}" for k in "abcd") + "  ms")
        for k in "abcd":
            print(f"2^{lg} ({k}): min {min(cols[k]):.3f} med {statistics.median(cols[k]):.3f} max {max(cols[k]):.3f} ms")
        print(f"2^{lg}: (b)/(c) = {statistics.median(cols['b']) / statistics.median(cols['c']):.3f}  "
              f"(a)/(c) = {statistics.median(cols['a']) / statistics.median(cols['c']):.3f}  "
              f"(a)/(b) = {statistics.median(cols['a']) / statistics.median(cols['b']):.3f}  "
              f"(c)/(d) = {statistics.median(cols['c']) / statistics.median(cols['d']):.3f}")
        if args.sweep and lg in (args.sweep_log_n or [max(args.log_n)]):
            scheds = [("default", {})] + [(w, {"SVGPU_H2D_SPLIT": w}) for w in args.splits]
            res = {name: [] for name, _ in scheds}
            for ps in range(args.passes):
                for name, env in scheds:
                    res[name].append(with_env(env, lambda: med_ms(run["b"], args.reps, args.warmup)))
            for name, _ in scheds:
                print(f"2^{lg} (b) pieces {name}: " + " ".join(f"{v:.3f}" for v in res[name]) + "  ms per pass")
        rset.close()


if __name__ == "__main__":
    main()
