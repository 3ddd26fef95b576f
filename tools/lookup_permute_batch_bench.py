"""The batched lookup permutation (sv_bn254_fr_lookup_permute_batch_device) against the same lookups
through the single call, one GPU, Montgomery form.

Per size n = 2^k and batch count L, three shapes:
  (a) range     one 2^16-entry range table (repeated to n rows) shared by all, inputs = random values of it
  (b) wide      one full-width table (generated scalars) shared by all, inputs = random draws from it
  (c) distinct  L full-width tables, one per lookup
and three ways of getting the L results:
  batch         one batch call
  presorted     one batch call with SV_LOOKUP_TABLES_SORTED on tables sorted beforehand (the one-off
                sort_device calls are timed on their own line)
  singles       L calls of sv_bn254_fr_lookup_permute_device in sequence: the baseline
Every time is the median (min .. max) of REPS calls after WARMUP, from HIP events around the whole
synchronous call or sequence of calls, read-back included, on a side stream made current.  The three
ways are taken interleaved -- batch, presorted, singles, batch, .. is one pass -- and there are two
passes; the spread is the difference between the baseline's two medians.  Before anything is timed
the three ways' outputs are compared byte for byte, and the first lookup's against the relations the
verifier checks (whole columns at 2^16, sampled rows above).

  python tools/lookup_permute_batch_bench.py [--log-n 16 20] [--counts 1 2 4 8 16] [--extra 22:4]
                                             [--reps 20] [--warmup 3] [--only range:16:8]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from svgpu import encoding as enc  # noqa: E402

from lookup_permute_bench import check_permute  # noqa: E402

SEED_S = 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY
R = enc.R
SHAPES = ("range", "wide", "distinct")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def interleaved(ways, reps, warmup):
    """{name: [event ms]}: every way once per round, reps rounds after warmup rounds."""
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    out = {name: [] for name in ways}
    for _ in range(reps):
        for name, fn in ways.items():
            out[name].append(event_ms(fn)[0])
    return out


def build(shape, n, count, dev, table16):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * count + n.bit_length())
    inputs, tables = [], []
    if shape == "range":
        table = table16[torch.arange(n, device=dev) & 0xFFFF].contiguous()
        for _ in range(count):
            inputs.append(table16[torch.randint(0, 1 << 16, (n,), device=dev, generator=gen)].contiguous())
            tables.append(table)
    else:
        for j in range(count):
            if shape == "distinct" or j == 0:
                table = dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S + j, 0, FORM)
            inputs.append(table[torch.randint(0, n, (n,), device=dev, generator=gen)].contiguous())
            tables.append(table)
    return inputs, tables


def run(shape, lg, count, dev, table16, reps, warmup):
    n = 1 << lg
    inputs, tables = build(shape, n, count, dev, table16)
    distinct = {t.data_ptr(): t for t in tables}
    out = {w: [(dv.empty_scalars(n, dev), dv.empty_scalars(n, dev)) for _ in range(count)] for w in ("batch", "presorted", "singles")}
    sort_ms = []
    for _ in range(3):                                                     # the one-off sort, warm on its third run
        done = {}
        ms = 0.0
        for ptr, t in distinct.items():
            buf = dv.empty_scalars(n, dev)
            ms += event_ms(lambda: dv.sort_device(t, form=FORM, out=buf))[0]
            done[ptr] = buf
        sort_ms.append(ms)
    presorted = [done[t.data_ptr()] for t in tables]

    def singles():
        for a, s, o in zip(inputs, tables, out["singles"]):
            dv.lookup_permute_device(a, s, form=FORM, out=o)
    ways = {"batch": lambda: dv.lookup_permute_batch_device(inputs, tables, form=FORM, out=out["batch"]),
            "presorted": lambda: dv.lookup_permute_batch_device(inputs, presorted, form=FORM, tables_sorted=True,
                                                                out=out["presorted"]),
            "singles": singles}
    for fn in ways.values():
        fn()
    torch.cuda.synchronize()
    for j in range(count):
        for k in (0, 1):
            assert torch.equal(out["batch"][j][k], out["singles"][j][k]), ("batch != singles", shape, lg, count, j, k)
            assert torch.equal(out["presorted"][j][k], out["singles"][j][k]), ("presorted != singles", shape, lg, count, j, k)
    check_permute(inputs[0], tables[0], out["batch"][0][0], out["batch"][0][1], n)
    passes = [interleaved(ways, reps, warmup) for _ in range(2)]
    label = f"2^{lg} L={count:<2} {shape:<8}"
    med = {w: [statistics.median(p[w]) for p in passes] for w in ways}
    spread = abs(med["singles"][0] - med["singles"][1])
    base = min(med["singles"])
    for w in ways:
        allv = sorted(passes[0][w] + passes[1][w])
        print(f"{label} {w:<9} pass medians {med[w][0] * 1e3:9.1f} {med[w][1] * 1e3:9.1f} us  "
              f"({allv[0] * 1e3:.1f} .. {allv[-1] * 1e3:.1f})  singles / this {base / max(med[w]):5.2f}", flush=True)
    verdict = "below the baseline by more than its spread" if max(med["batch"]) < base - spread else "NOT below the baseline by more than its spread"
    order = "below the batch call" if max(med["presorted"]) < min(med["batch"]) else "NOT below the batch call"
    print(f"{label} baseline spread {spread * 1e3:.1f} us; batch {verdict}; presorted {order}; one-off sort of "
          f"{len(distinct)} table(s) {sort_ms[-1] * 1e3:.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--extra", nargs="*", default=["22:4"], help="further log_n:count points")
    ap.add_argument("--only", help="shape:log_n:count, one point (for a kernel trace)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery  reps={args.reps} warmup={args.warmup}  two interleaved passes", flush=True)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    mont16 = b"".join(((v << 256) % R).to_bytes(32, "little") for v in range(1 << 16))
    table16 = torch.from_numpy(np.frombuffer(mont16, np.int64).reshape(1 << 16, 4).copy()).to(dev)
    if args.only:
        shape, lg, count = args.only.split(":")
        points = [(shape, int(lg), int(count))]
    else:
        points = [(s, lg, c) for lg in args.log_n for s in SHAPES for c in args.counts]
        points += [(s, int(e.split(":")[0]), int(e.split(":")[1])) for e in args.extra for s in SHAPES]
    for shape, lg, count in points:
        run(shape, lg, count, dev, table16, args.reps, args.warmup)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
