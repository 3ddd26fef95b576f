"""The permutation and lookup terms of the quotient numerator on the device
(sv_bn254_fr_permutation_terms_device, sv_bn254_fr_lookup_terms_device), one GPU.

Per (k, e) (default (16,2) (20,2) (22,2)), with N = 2^(k + e) rows: the permutation terms of m = 6
columns in chunks of 3, and the lookup terms of 1 and of 4 lookups, each in place on a running
accumulator.  Three figures per shape:
  (a) the call;
  (b) the floor: a device-to-device copy that moves exactly the bytes the call must read and write
      (every input column once, d_out once: the copy's source and destination are half that each),
      timed in the same run;
  (c) one host thread doing the same fold over csrc/field.hpp's host build
      (tools/ubench_host_quotient_terms, run when it has been built; the only alternative a caller
      has without these calls).  It is measured up to 2^20 rows; it is linear in the rows.
and (a) / (b).  Beside them the coset_lde_device time of the columns the call consumes (measured on
as many columns as one LDE call takes, scaled to the call's column count), so a reader sees the
call's share of the quotient step.

Each figure is the median (min .. max) of REPS calls after WARMUP, from HIP events on the call's
stream (a side stream made current, so the library's work and torch's copy run on that stream and
the events bracket them, the flag read-back included), and beside it the wall time.  Before anything
is timed the output is compared at four rows with the constraint formulas in Python-int arithmetic.

MODEL columns (computed, not measured; Montgomery form): Fr products per call / 130 G products/s and
HBM bytes / 8 TB/s, the figures DESIGN.md uses.  Per row: permutation 4 m + 2 n_z + 8 products and
32 (2 m + n_z (1 + E / S) + (n_z - 1) + 5) bytes; lookups 11 n_lookups + 4 products and
32 (n_lookups (3 + 2 (1 + E / S)) + 5) bytes, with E = 2^e and S = kQtSpan rows per block.

  python tools/quotient_terms_bench.py [--shapes 16,2 20,2 22,2] [--reps 20] [--warmup 3] [--no-host]
                                       [--out profiles/quotient_terms_ab.log]
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
ZETA = pow(7, (R - 1) // 3, R)
HOST_BIN = os.path.join(ROOT, "tools", "ubench_host_quotient_terms")
PRODUCTS_PER_S, HBM_BYTES_PER_S = 130e9, 8e12
S = 256 * int(re.search(r"constexpr uint32_t kQtPer = (\d+);",
                        open(os.path.join(ROOT, "snark-verifier-axiom_amd", "csrc", "quotient_terms.hpp")).read()).group(1))
M, CHUNK, LAST = 6, 3, -6
BETA, GAMMA, Y, DELTA = 0x1234567, 0x89abcde, 0xfedcba9, 7
_LOG = []


def say(line):
    print(line, flush=True)
    _LOG.append(line)


def model_perm(N, e, m, nz):
    cols = 2 * m + nz * (1 + (1 << e) / S) + (nz - 1) + 5
    return (4 * m + 2 * nz + 8) * N, 32 * cols * N


def model_lookup(N, e, L):
    cols = L * (3 + 2 * (1 + (1 << e) / S)) + 5
    return (11 * L + 4) * N, 32 * cols * N


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
    say(f"{label:<58} events {statistics.median(ev) * 1e3:9.1f} us ({ev[0] * 1e3:.1f} .. {ev[-1] * 1e3:.1f})  "
        f"wall {wall * 1e3:9.1f} us{tail}")
    return statistics.median(ev), ev[0], ev[-1]


def ratio(label, a, b):
    say(f"{label}: {a[0] / b[0]:.3f}  (medians {a[0] * 1e3:.1f} / {b[0] * 1e3:.1f} us; "
        f"spreads {a[1] * 1e3:.1f} .. {a[2] * 1e3:.1f} and {b[1] * 1e3:.1f} .. {b[2] * 1e3:.1f})")


def to_int(row):
    return enc.limbs_to_int(list(row.cpu().numpy().view(np.uint64))) * pow(1 << 256, -1, R) % R


def columns(count, N, dev, start):
    return [dv.gen_scalars(dv.empty_scalars(N, dev), SEED_S, (start + c) * N, FORM) for c in range(count)]


def copy_floor(tag, total_bytes, dev, reps, warmup):
    """A device-to-device copy whose reads plus writes are total_bytes."""
    rows = total_bytes // 64
    src = torch.empty((rows, 4), dtype=torch.int64, device=dev).fill_(1)
    dst = torch.empty_like(src)
    out = report(f"{tag} floor: copy of {rows * 32 / 2**20:.0f} MiB", timed(lambda: dst.copy_(src), reps, warmup))
    del src, dst
    return out


def lde_share(tag, call, k, e, ncols, dev, reps, warmup):
    count = max(1, min(ncols, (1 << 28) >> (k + e)))
    coeffs = dv.gen_scalars(dv.empty_scalars(count << k, dev), SEED_S, 99, FORM).reshape(count, 1 << k, 4)
    out = torch.empty((count, 1 << (k + e), 4), dtype=torch.int64, device=dev)
    one = report(f"{tag} coset_lde_device of {count} columns",
                 timed(lambda: dv.coset_lde_device(coeffs, e, shift=ZETA, form=FORM, out=out), reps, warmup))
    say(f"{tag} call / coset LDE of its {ncols} columns: {call[0] / (one[0] * ncols / count):.3f}  "
        f"(LDE scaled from {count} to {ncols} columns: {one[0] * ncols / count * 1e3:.1f} us)")
    del coeffs, out


def bench_perm(k, e, dev, reps, warmup):
    K, E = k + e, 1 << e
    N, nz = 1 << K, -(-M // CHUNK)
    cols, sig, z = columns(M, N, dev, 0), columns(M, N, dev, 10), columns(nz, N, dev, 20)
    l, acc = columns(3, N, dev, 30), columns(1, N, dev, 40)[0]
    s = [BETA * pow(DELTA, j, R) % R for j in range(M)]
    out = dv.permutation_terms_device(cols, sig, s, CHUNK, z, *l, BETA, GAMMA, Y, k, LAST, shift=ZETA, form=FORM, acc=acc)
    w = svgpu.root_of_unity(K)
    for j in (0, 1, N // 2 + 3, N - 1):
        at = lambda c, r=0: to_int(c[(j + r * E) % N])  # noqa: E731
        x = ZETA * pow(w, j, R) % R
        cons = [at(l[0]) * (1 - at(z[0])), at(l[1]) * (at(z[-1]) ** 2 - at(z[-1]))]
        cons += [at(l[0]) * (at(z[i]) - at(z[i - 1], LAST)) for i in range(1, nz)]
        for i in range(nz):
            left, right = at(z[i], 1), at(z[i])
            for t in range(i * CHUNK, min((i + 1) * CHUNK, M)):
                left = left * (at(cols[t]) + BETA * at(sig[t]) + GAMMA) % R
                right = right * (at(cols[t]) + s[t] * x + GAMMA) % R
            cons.append(at(l[2]) * (left - right))
        want = at(acc)
        for c in cons:
            want = (want * Y + c) % R
        assert to_int(out[j]) == want, f"permutation ({k},{e}): row {j} differs from the Python fold"
    del out
    tag = f"permutation ({k},{e}) m={M} chunk={CHUNK}"
    call = report(f"{tag} call, in place",
                  timed(lambda: dv.permutation_terms_device(cols, sig, s, CHUNK, z, *l, BETA, GAMMA, Y, k, LAST, shift=ZETA,
                                                            form=FORM, acc=acc, out=acc), reps, warmup),
                  model_perm(N, e, M, nz))
    ncols = 2 * M + nz + 3
    floor = copy_floor(tag, 32 * N * (ncols + (nz - 1) + 2), dev, reps, warmup)
    ratio(f"{tag} call / floor", call, floor)
    del cols, sig, z, l, acc
    torch.cuda.empty_cache()
    lde_share(tag, call, k, e, ncols, dev, reps, warmup)


def bench_lookup(k, e, L, dev, reps, warmup):
    K, E = k + e, 1 << e
    N = 1 << K
    look = [columns(5, N, dev, 50 + 5 * i) for i in range(L)]
    l, acc = columns(3, N, dev, 30), columns(1, N, dev, 40)[0]
    out = dv.lookup_terms_device(look, *l, BETA, GAMMA, Y, k, form=FORM, acc=acc)
    for j in (0, 1, N // 2 + 3, N - 1):
        at = lambda c, r=0: to_int(c[(j + r * E) % N])  # noqa: E731
        want = at(acc)
        for zc, pa, ps, a, sc in look:
            d = at(pa) - at(ps)
            for c in (at(l[0]) * (1 - at(zc)), at(l[1]) * (at(zc) ** 2 - at(zc)),
                      at(l[2]) * (at(zc, 1) * (at(pa) + BETA) * (at(ps) + GAMMA) - at(zc) * (at(a) + BETA) * (at(sc) + GAMMA)),
                      at(l[0]) * d, at(l[2]) * d * (at(pa) - at(pa, -1))):
                want = (want * Y + c) % R
        assert to_int(out[j]) == want, f"lookups ({k},{e}) x{L}: row {j} differs from the Python fold"
    del out
    tag = f"lookups ({k},{e}) x{L}"
    call = report(f"{tag} call, in place",
                  timed(lambda: dv.lookup_terms_device(look, *l, BETA, GAMMA, Y, k, form=FORM, acc=acc, out=acc), reps, warmup),
                  model_lookup(N, e, L))
    ncols = 5 * L + 3
    floor = copy_floor(tag, 32 * N * (ncols + 2), dev, reps, warmup)
    ratio(f"{tag} call / floor", call, floor)
    del look, l, acc
    torch.cuda.empty_cache()
    lde_share(tag, call, k, e, ncols, dev, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["16,2", "20,2", "22,2"])
    ap.add_argument("--lookups", nargs="*", type=int, default=[1, 4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quotient_terms_ab.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes]
    say(f"# {svgpu.version()}  form=montgomery shift=ZETA rows per block {S} reps={args.reps} warmup={args.warmup}")
    if args.no_host:
        say("host, one thread: skipped (--no-host)")
    elif os.path.exists(HOST_BIN):
        logs = sorted({min(k + e, 20) for k, e in shapes})
        res = subprocess.run([HOST_BIN] + [str(lg) for lg in logs], capture_output=True, text=True, timeout=900).stdout
        for line in res.splitlines():
            say("host, one thread: " + line)
    else:
        say("host, one thread: not measured (tools/ubench_host_quotient_terms is not built)")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    for k, e in shapes:
        bench_perm(k, e, dev, args.reps, args.warmup)
        for L in args.lookups:
            bench_lookup(k, e, L, dev, args.reps, args.warmup)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(_LOG) + "\n")


if __name__ == "__main__":
    main()
