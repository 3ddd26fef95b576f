"""Expression programs on the device (sv_bn254_fr_expressions_device), one GPU, Montgomery form.

Workloads, with N = 2^(k + e) rows:
  (a) the five-monomial PLONK gate  q_l a + q_r b + q_m a b - c + q_c,  one FOLD, at (16,2) (20,2) (22,2);
  (b) halo2-base's single gate  q (a + b c - d)  read as rotations 0 .. 3 of one advice column, one
      FOLD, at the same shapes;
  (c) one lookup's five constraints as a program, against sv_bn254_fr_lookup_terms_device on the
      same columns in the same run: the price of interpretation, as a ratio;
  (d) the theta-compression of three columns into one by STORE, at (20,0).
The folds run in place on a running accumulator.  Per workload:
  the call;
  the floor: a device-to-device copy that moves exactly the bytes the call must move -- each
      distinct column once per distinct rotation, the accumulator, the outputs -- timed in the same run;
  MODEL products (computed, not measured): the program's MUL and FOLD count per row at the 130 G
      products/s DESIGN.md uses.

Each figure is the median (min .. max) of REPS calls after WARMUP, from HIP events on the call's
stream (a side stream made current, so the library's work and torch's copy run on that stream and
the events bracket them, the flag read-back included), and beside it the wall time.  Before anything
is timed the output is compared at four rows with the trees in Python-int arithmetic.

  python tools/expressions_bench.py [--shapes 16,2 20,2 22,2] [--reps 20] [--warmup 3]
                                    [--out profiles/expressions_ab.log]
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
from svgpu import _lib  # noqa: E402
from svgpu import device as dv  # noqa: E402
from svgpu import encoding as enc  # noqa: E402

SEED_S = 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY
R = enc.R
PRODUCTS_PER_S = 130e9
BETA, GAMMA, Y, THETA = 0x1234567, 0x89abcde, 0xfedcba9, 0x13579bdf
_LOG = []


def say(line):
    print(line, flush=True)
    _LOG.append(line)


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


def report(label, samples, products=None):
    ev = sorted(s[1] for s in samples)
    wall = statistics.median(s[0] for s in samples)
    tail = f" | MODEL products {products / PRODUCTS_PER_S * 1e6:8.1f} us" if products is not None else ""
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


def value(e, col):
    """A tree's value in Python ints; col(i, rot) reads a column."""
    kind = e[0]
    if kind == "col":
        return col(e[1], e[2])
    if kind == "const":
        return e[1] % R
    if kind == "neg":
        return -value(e[1], col) % R
    if kind == "scaled":
        return value(e[1], col) * e[2] % R
    if kind == "powers":
        vals, base = [value(x, col) for x in e[1]], value(e[2], col)
        acc = vals[0]
        for v in vals[1:]:
            acc = (acc * base + v) % R
        return acc
    a, c = value(e[1], col), value(e[2], col)
    return {"add": a + c, "sub": a - c, "mul": a * c}[kind] % R


def reads(ops):
    return len({(index, rot) for op, index, rot in ops if op == _lib.SV_EXPR_COLUMN})


def products(ops):
    return sum(1 for op, _, _ in ops if op in (_lib.SV_EXPR_MUL, _lib.SV_EXPR_FOLD))


def check(sinks, cols, acc, out, stores, k, e):
    N, E = 1 << (k + e), 1 << e
    for j in (0, 1, N // 2 + 3, N - 1):
        col = lambda i, rot: to_int(cols[i][(j + rot * E) % N])  # noqa: E731
        want = to_int(acc[j]) if acc is not None else 0
        for sink in sinks:
            if sink[0] == "fold":
                want = (want * Y + value(sink[1], col)) % R
            else:
                assert to_int(stores[sink[1]][j]) == value(sink[2], col), f"({k},{e}): store row {j} differs"
        if out is not None:
            assert to_int(out[j]) == want, f"({k},{e}): row {j} differs from the Python fold"


def bench_program(tag, sinks, n_cols, k, e, dev, reps, warmup, cols=None):
    """The program's call and its copy floor; returns (call, columns)."""
    N = 1 << (k + e)
    cols = columns(n_cols, N, dev, 100) if cols is None else cols
    ops, consts, depth = svgpu.compile_expressions(sinks)
    folds = any(s[0] == "fold" for s in sinks)
    n_stores = sum(1 for s in sinks if s[0] == "store")
    acc = columns(1, N, dev, 40)[0] if folds else None
    out, stores = svgpu.expressions_device(ops, cols, consts, stores=n_stores, y=Y if folds else None, acc=acc, log_n=k,
                                           form=FORM)
    check(sinks, cols, acc, out, stores, k, e)
    del out
    say(f"{tag}: {len(ops)} ops, depth {depth}, {reads(ops)} column reads, {products(ops)} products per row")
    call = report(f"{tag} call" + (", in place" if folds else ""),
                  timed(lambda: svgpu.expressions_device(ops, cols, consts, stores=stores, y=Y if folds else None, acc=acc,
                                                         out=acc, log_n=k, form=FORM), reps, warmup), products(ops) * N)
    floor = copy_floor(tag, 32 * N * (reads(ops) + n_stores + (2 if folds else 0)), dev, reps, warmup)
    ratio(f"{tag} call / floor", call, floor)
    return call, cols


def lookup_sinks():
    l0, ll, la, z, pa, ps, a, s = (("col", i, 0) for i in range(8))
    bt, gm, one = ("const", BETA), ("const", GAMMA), ("const", 1)
    return [("fold", ("mul", l0, ("sub", one, z))),
            ("fold", ("mul", ll, ("sub", ("mul", z, z), z))),
            ("fold", ("mul", la, ("sub", ("mul", ("mul", ("col", 3, 1), ("add", pa, bt)), ("add", ps, gm)),
                                  ("mul", ("mul", z, ("add", a, bt)), ("add", s, gm))))),
            ("fold", ("mul", l0, ("sub", pa, ps))),
            ("fold", ("mul", la, ("mul", ("sub", pa, ps), ("sub", pa, ("col", 4, -1)))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["16,2", "20,2", "22,2"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expressions_ab.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes]
    say(f"# {svgpu.version()}  form=montgomery reps={args.reps} warmup={args.warmup}")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    ql, qr, qm, qc, a, b, c = (("col", i, 0) for i in range(7))
    plonk = [("fold", ("sub", ("add", ("add", ("add", ("mul", ql, a), ("mul", qr, b)), ("mul", qm, ("mul", a, b))), qc), c))]
    base = [("fold", ("mul", ("col", 0, 0), ("sub", ("add", ("col", 1, 0), ("mul", ("col", 1, 1), ("col", 1, 2))),
                                             ("col", 1, 3))))]
    for k, e in shapes:
        bench_program(f"(a) PLONK gate ({k},{e})", plonk, 7, k, e, dev, args.reps, args.warmup)
        torch.cuda.empty_cache()
        bench_program(f"(b) halo2-base gate ({k},{e})", base, 2, k, e, dev, args.reps, args.warmup)
        torch.cuda.empty_cache()
        tag = f"(c) lookup constraints ({k},{e})"
        call, cols = bench_program(tag + " as a program", lookup_sinks(), 8, k, e, dev, args.reps, args.warmup)
        acc = columns(1, 1 << (k + e), dev, 40)[0]
        fixed = report(f"{tag} lookup_terms_device, in place",
                       timed(lambda: dv.lookup_terms_device([cols[3:8]], cols[0], cols[1], cols[2], BETA, GAMMA, Y, k,
                                                            form=FORM, acc=acc, out=acc), args.reps, args.warmup))
        ratio(f"{tag} program / fixed-function kernel", call, fixed)
        del cols, acc
        torch.cuda.empty_cache()
    theta = [("store", 0, svgpu.compress_expressions([("col", 0, 0), ("col", 1, 0), ("col", 2, 0)], THETA))]
    bench_program("(d) theta-compression of 3 columns (20,0)", theta, 3, 20, 0, dev, args.reps, args.warmup)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(_LOG) + "\n")


if __name__ == "__main__":
    main()
