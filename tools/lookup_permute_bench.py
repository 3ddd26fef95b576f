"""The Fr sort and a lookup's permuted columns on the device (sv_bn254_fr_sort_device,
sv_bn254_fr_lookup_permute_device), one GPU.

Per size n = 2^k (default 16, 20, 24):
  sort, full-width keys                 generated scalars: all 32 digits live
  sort, 16-bit keys                     random values below 2^16: two live passes
  permutation, full-width table         S = generated scalars, A = n random draws from S
  permutation, 2^16-entry range table   S = 0 .. 2^16 - 1 repeated to n rows, A = n random values of it
the median (min .. max) of REPS calls after WARMUP, from HIP events on the call's stream (a side
stream made current, so the library works on that stream and the events bracket its launches, the
head's read-back included) and, beside it, the wall time of the synchronous call.  Before anything
is timed, every shape is checked: at 2^16 against sorted() and the relations the verifier checks on
the whole columns read back, above that on sampled rows.

Beside every measured time stands a MODEL column, computed from the shape and not measured: the
bytes a sort must move, (1 + 2 x live passes) x 32 B x n -- the first pass reads the column, every
live pass reads and writes an image -- over 8 TB/s (the HBM peak DESIGN.md uses); a permutation
counts its two sorts.  What the model leaves out: the images' first write and the conversion's
(64 B per row), a live pass's count launch (it reads one limb of every key: the same sectors again),
the permutation's own five launches, and the fixed cost of 3 x 32 launches per sort, live or not.

For context, the host path a caller had: one thread, std::sort on canonical limbs and halo2's map
walk (tools/ubench_host_lookup_permute, run when it has been built).

  python tools/lookup_permute_bench.py [--log-n 16 20 24] [--reps 20] [--warmup 3] [--no-host]
"""
import argparse
import os
import random
import re
import statistics
import subprocess
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
FORM = svgpu.SV_MONTGOMERY  # halo2curves' in-memory layout: what the Rust shim passes
R = enc.R
RINV = pow(1 << 256, -1, R)
HOST_BIN = os.path.join(ROOT, "tools", "ubench_host_lookup_permute")
HBM_BYTES_PER_S = 8e12
_HPP = open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "lookup_permute.hpp")).read()
TILE = int(re.search(r"constexpr uint32_t kLpTile = (\d+);", _HPP).group(1))
T = int(re.search(r"constexpr uint32_t kLpThreads = (\d+);", _HPP).group(1))


def model(n, live, sorts):
    return sorts * (1 + 2 * live) * 32 * n


def timed(fn, reps, warmup):
    """[(wall ms, event ms)] of fn, which synchronises."""
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


def report(label, nbytes, samples):
    ev = sorted(s[1] for s in samples)
    wall = statistics.median(s[0] for s in samples)
    mb = nbytes / HBM_BYTES_PER_S * 1e3
    med = statistics.median(ev)
    print(f"{label:<44} events {med * 1e3:9.1f} us ({ev[0] * 1e3:.1f} .. {ev[-1] * 1e3:.1f})  "
          f"wall {wall * 1e3:9.1f} us | MODEL bytes {mb * 1e3:8.1f} us  | model / measured {mb / med:.2f}", flush=True)
    return med


def ints(t):
    """Rows of a Montgomery column as canonical ints."""
    raw = t.cpu().numpy().view(np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * RINV % R for i in range(0, len(raw), 32)]


def sample(t, idx):
    return ints(t[torch.tensor(idx, device=t.device)])


def check_sort(keys, out, n):
    if n <= 1 << 16:
        assert ints(out) == sorted(ints(keys)), "sort"
        return
    rng = random.Random(n)
    idx = sorted(rng.randrange(n - 1) for _ in range(2000))
    lo, hi = sample(out, idx), sample(out, [i + 1 for i in idx])
    assert all(a <= b for a, b in zip(lo, hi)), "sort: sampled neighbours out of order"
    assert sample(out, [0])[0] <= lo[0]


def check_permute(a, s, ap, sp, n):
    if n <= 1 << 16:
        A, S, AP, SP = ints(a), ints(s), ints(ap), ints(sp)
        assert AP == sorted(A) and sorted(SP) == sorted(S), "permutation: not a permutation of the columns"
        assert AP[0] == SP[0] and all(AP[i] == SP[i] or AP[i] == AP[i - 1] for i in range(1, n)), "permutation: row rule"
        return
    rng = random.Random(n + 1)
    idx = sorted(rng.randrange(1, n) for _ in range(2000))
    AP, SP, prev = sample(ap, idx), sample(sp, idx), sample(ap, [i - 1 for i in idx])
    assert all(x == y or x == p for x, y, p in zip(AP, SP, prev)), "permutation: row rule on sampled rows"
    assert sample(ap, [0]) == sample(sp, [0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread host run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery tile {TILE} = {T} threads x {TILE // T} keys  reps={args.reps} "
          f"warmup={args.warmup}")
    if args.no_host:
        print("host, one thread: skipped (--no-host)")
    elif os.path.exists(HOST_BIN):
        out = subprocess.run([HOST_BIN] + [str(lg) for lg in args.log_n], capture_output=True, text=True,
                             timeout=900).stdout
        for line in out.splitlines():
            print("host, one thread: " + line)
    else:
        print("host, one thread: not measured (tools/ubench_host_lookup_permute is not built)")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    mont16 = b"".join(((v << 256) % R).to_bytes(32, "little") for v in range(1 << 16))
    table16 = torch.from_numpy(np.frombuffer(mont16, np.int64).reshape(1 << 16, 4).copy()).to(dev)
    for lg in args.log_n:
        n = 1 << lg
        gen = torch.Generator(device=dev)
        gen.manual_seed(lg)
        wide = dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, 0, FORM)
        narrow = table16[torch.randint(0, 1 << 16, (n,), device=dev, generator=gen)].contiguous()
        drawn = wide[torch.randint(0, n, (n,), device=dev, generator=gen)].contiguous()
        ranged = table16[torch.arange(n, device=dev) & 0xFFFF].contiguous()
        o1, o2 = dv.empty_scalars(n, dev), dv.empty_scalars(n, dev)
        torch.cuda.synchronize()
        for label, keys, live in (("sort, full-width keys", wide, 32), ("sort, 16-bit keys", narrow, 2)):
            dv.sort_device(keys, form=FORM, out=o1)
            check_sort(keys, o1, n)
            report(f"2^{lg} {label}", model(n, live, 1),
                   timed(lambda: dv.sort_device(keys, form=FORM, out=o1), args.reps, args.warmup))
        for label, a, s, live in (("permutation, full-width table", drawn, wide, 32),
                                  ("permutation, 2^16-entry range table", narrow, ranged, 2)):
            dv.lookup_permute_device(a, s, form=FORM, out=(o1, o2))
            check_permute(a, s, o1, o2, n)
            report(f"2^{lg} {label}", model(n, live, 2),
                   timed(lambda: dv.lookup_permute_device(a, s, form=FORM, out=(o1, o2)), args.reps, args.warmup))
        del wide, narrow, drawn, ranged, o1, o2, keys, a, s


if __name__ == "__main__":
    main()
