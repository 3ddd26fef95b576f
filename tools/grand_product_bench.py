"""Running products and batch inversion on the device (sv_bn254_fr_grand_product_device,
sv_bn254_fr_batch_invert_device), one GPU.

Per size n = 2^k (default 16, 20, 24) and shape -- the permutation argument with 4 columns (IDENTITY
numerators, COLUMN denominators: 8 columns read), a lookup (2 + 2 PLAIN factors: 4 columns) and batch
inversion (out of place and in place) -- the median (min .. max) of REPS calls after WARMUP, from
HIP events on the call's stream (a side stream made current, so the library works on that stream
and the events bracket its launches, the head's read-back included) and, beside it, the wall time of
the synchronous call.  Before anything is timed, every shape is checked at three rows against
Python-int arithmetic on the columns read back.

Beside every measured time stand two MODEL columns, computed from the shape and not measured:
  products  the call's Fr products / 130 G products/s (DESIGN.md's figure for the chip)
  bytes     the call's HBM bytes / 8 TB/s (the HBM peak DESIGN.md uses)
The counts (kept here, next to the benchmark; Montgomery form, P = kGpPer, L = log2 kGpThreads).
Forming a row's two products (k_gp_reduce only: it leaves them in scratch for k_gp_apply): per side
its factors - 1, plus one per COLUMN and per IDENTITY factor (s y, s omega^i), plus
(P - 1) / P + 13 / P for omega^i where a factor is IDENTITY (the step, and the power of the thread's
first row from 26 seeds, half of them set).  k_gp_reduce adds 2 (P - 1) / P (thread totals) + 2 / P
(the tree); k_gp_apply takes 2 (P - 1) / P + 2 L / P (the two scans) + (3 P - 1) / P (suffix walk,
prefix walk, z).  Batch inversion forms nothing and walks P - 1 suffix products.  Bytes: every column
once, the rows' two products written and read once (128 B), z once; batch inversion reads its
column twice and writes once.

For context, the host path a caller had: one thread over field.hpp's host build doing per-row
factors, Montgomery-trick inversion and the serial product (tools/ubench_host_grand_product, run
when it has been built).

  python tools/grand_product_bench.py [--log-n 16 20 24] [--reps 20] [--warmup 3] [--no-host]
"""
import argparse
import os
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
HOST_BIN = os.path.join(ROOT, "tools", "ubench_host_grand_product")
PRODUCTS_PER_S, HBM_BYTES_PER_S = 130e9, 8e12
_HPP = open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "grand_product.hpp")).read()
S = int(re.search(r"constexpr uint32_t kGpSpan = (\d+);", _HPP).group(1))
T = int(re.search(r"constexpr uint32_t kGpThreads = (\d+);", _HPP).group(1))
P, L = S // T, T.bit_length() - 1
BETA, GAMMA, DELTA = 0x1D0F5A17C3B2A495877665544332211 % R, 0x2B3C4D5E6F708192A3B4C5D6E7F8091 % R, 7
PLAIN, COLUMN, IDENTITY = 0, 1, 2


def model(num, den, n, invert=False):
    """(products, bytes) of one call in Montgomery form; num, den: lists of factor kinds."""
    if invert:
        form, walk, nbytes = 0.0, (3 * P - 2) / P, 3 * 32
    else:
        kinds = list(num) + list(den)
        form = sum(max(len(s) - 1, 0) for s in (num, den)) + sum(1 for k in kinds if k != PLAIN)
        if IDENTITY in kinds:
            form += (P - 1) / P + 13 / P
        cols = len(kinds) + sum(1 for k in kinds if k == COLUMN)
        walk, nbytes = (3 * P - 1) / P, (cols + 4 + 1) * 32
    reduce_ = form + 2 * (P - 1) / P + 2 / P
    apply_ = 2 * (P - 1) / P + 2 * L / P + walk
    return (reduce_ + apply_) * n, nbytes * n


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


def report(label, counts, samples):
    ev = sorted(s[1] for s in samples)
    wall = statistics.median(s[0] for s in samples)
    products, nbytes = counts
    mp, mb = products / PRODUCTS_PER_S * 1e3, nbytes / HBM_BYTES_PER_S * 1e3
    med = statistics.median(ev)
    print(f"{label:<44} events {med * 1e3:9.1f} us ({ev[0] * 1e3:.1f} .. {ev[-1] * 1e3:.1f})  "
          f"wall {wall * 1e3:9.1f} us | MODEL products {mp * 1e3:8.1f} us  MODEL bytes {mb * 1e3:7.1f} us  "
          f"| model / measured {max(mp, mb) / med:.2f}", flush=True)
    return med


def row(t, i):
    """Row i of a Montgomery column as a canonical int."""
    return enc.fr_from_struct(enc.fe_struct(enc.limbs_to_int(list(t[i].cpu().numpy().view(np.uint64)))), FORM)


def value(f, i, w):
    kind, x, y, s, c = f
    v = row(x, i) + c
    if kind == COLUMN:
        v += s * row(y, i)
    elif kind == IDENTITY:
        v += s * pow(w, i, R)
    return v % R


def check_product(num, den, n, w, z, total):
    """z[1] from row 0, a step in the middle, and the total from the last row."""
    def ratio(i):
        nv = dv_ = 1
        for f in num:
            nv = nv * value(f, i, w) % R
        for f in den:
            dv_ = dv_ * value(f, i, w) % R
        return nv * pow(dv_, -1, R) % R
    assert row(z, 0) == 1
    if n > 1:
        assert row(z, 1) == ratio(0), "z[1]"
        m = n // 2
        assert row(z, m + 1) == row(z, m) * ratio(m) % R, "a step in the middle"
    assert total == row(z, n - 1) * ratio(n - 1) % R, "the total"


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
    print(f"# {svgpu.version()}  form=montgomery span {S} = {T} threads x {P} rows  reps={args.reps} warmup={args.warmup}")
    if args.no_host:
        print("host, one thread: skipped (--no-host)")
    elif os.path.exists(HOST_BIN):
        out = subprocess.run([HOST_BIN] + [str(lg) for lg in args.log_n], capture_output=True, text=True,
                             timeout=900).stdout
        for line in out.splitlines():
            print("host, one thread: " + line)
    else:
        print("host, one thread: not measured (tools/ubench_host_grand_product is not built)")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    for lg in args.log_n:
        n = 1 << lg
        w = svgpu.root_of_unity(lg)
        cols = [dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, k * n, FORM) for k in range(8)]
        z = dv.empty_scalars(n, dev)
        torch.cuda.synchronize()
        perm_num = [(IDENTITY, cols[j], None, BETA * pow(DELTA, j, R) % R, GAMMA) for j in range(4)]
        perm_den = [(COLUMN, cols[j], cols[4 + j], BETA, GAMMA) for j in range(4)]
        look_num = [(PLAIN, cols[0], None, 0, BETA), (PLAIN, cols[1], None, 0, GAMMA)]
        look_den = [(PLAIN, cols[2], None, 0, BETA), (PLAIN, cols[3], None, 0, GAMMA)]
        shapes = [("permutation, 4 columns", perm_num, perm_den, w), ("lookup", look_num, look_den, None)]
        for label, num, den, om in shapes:
            _, total = dv.grand_product_device(num, den, omega=om, form=FORM, out=z)
            check_product(num, den, n, w, z, total)
            counts = model([f[0] for f in num], [f[0] for f in den], n)
            report(f"2^{lg} {label}", counts,
                   timed(lambda: dv.grand_product_device(num, den, omega=om, form=FORM, out=z), args.reps, args.warmup))
        x = cols[0]
        inv = dv.batch_invert_device(x, form=FORM, out=z)
        for i in (0, n // 2, n - 1):
            assert row(x, i) * row(inv, i) % R == 1, f"2^{lg}: inverse of row {i}"
        counts = model([], [], n, invert=True)
        report(f"2^{lg} batch inversion, out of place", counts,
               timed(lambda: dv.batch_invert_device(x, form=FORM, out=z), args.reps, args.warmup))
        work = x.clone()
        report(f"2^{lg} batch inversion, in place", counts,
               timed(lambda: dv.batch_invert_device(work, form=FORM, out=work), args.reps, args.warmup))
        del cols, z, x, inv, work, perm_num, perm_den, look_num, look_den, shapes, num, den


if __name__ == "__main__":
    main()
