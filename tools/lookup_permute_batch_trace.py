"""The workload and the summary of the batch call's kernel trace in profiles/lookup_permute_batch_ab.log.

  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/lookup_permute_batch_trace.py
      CALLS (default 12) batch calls of L = 8 lookups at 2^16 rows against one shared range table
      (shape (a) of tools/lookup_permute_batch_bench.py), Montgomery form, and nothing else that
      launches a kernel of csrc/lookup_permute.hip
  python tools/lookup_permute_batch_trace.py --summarise DIR/NAME_results.db
      per kernel of that file: dispatches, mean (min .. max) and sum of the durations in rocprofv3's
      database, and the dispatches and the kernel time per call

A traced dispatch's duration is taken with the profiler attached, which serialises the dispatches
and adds to each; the sum per call is therefore above what HIP events measure around the whole call
untraced, and only the counts and the proportions are meant to be read.
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

LOOKUPS, LOG_N = 8, 16


def summarise(path, calls):
    import sqlite3
    db = sqlite3.connect(path)
    rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start), sum(end - start) "
                      "from kernels group by name order by 6 desc").fetchall()
    total, count = 0, 0
    for name, c, mean, lo, hi, s in rows:
        m = re.search(r"(k_lpb?_\w+?)(<[^>]*>)?(\(|$)", name)
        if not m:
            continue
        short = m.group(1) + (m.group(2) or "")
        print(f"{short:<28} {c:5d} dispatches  mean {mean / 1e3:7.1f} us (min {lo / 1e3:.1f} .. max {hi / 1e3:.1f})  "
              f"sum {s / 1e3:9.1f} us")
        total, count = total + s, count + c
    print(f"all kernels of lookup_permute.hip: {count} dispatches, {total / 1e3:.1f} us over {calls} batch calls = "
          f"{count / calls:.1f} kernels and {total / calls / 1e3:.1f} us per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--summarise", metavar="DB")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.calls)
        return
    import numpy as np
    import torch
    import svgpu
    from svgpu import device as dv
    import lookup_permute_batch_bench as bb
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    mont16 = b"".join(((v << 256) % bb.R).to_bytes(32, "little") for v in range(1 << 16))
    table16 = torch.from_numpy(np.frombuffer(mont16, np.int64).reshape(1 << 16, 4).copy()).to(dev)
    inputs, tables = bb.build("range", 1 << LOG_N, LOOKUPS, dev, table16)
    out = [(dv.empty_scalars(1 << LOG_N, dev), dv.empty_scalars(1 << LOG_N, dev)) for _ in range(LOOKUPS)]
    for _ in range(args.calls):
        dv.lookup_permute_batch_device(inputs, tables, form=bb.FORM, out=out)
    torch.cuda.synchronize()
    print(f"{args.calls} batch calls of L = {LOOKUPS} at 2^{LOG_N}, one range table")


if __name__ == "__main__":
    main()
