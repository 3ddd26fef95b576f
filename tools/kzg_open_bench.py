"""KZG opening on a resident base set against the witness MSM alone (one GPU).

Per size n = 2^k (default 16, 18, 20), PASSES interleaved passes of
  (a)  sv_bn254_g1_msm_bases_device / sv_bn254_g1_msm_bases over n - 1 terms (the quotient as scalars):
       what an opening cost before, without its division -- the yardstick (this commit leaves both
       entry points and the MSM pipeline as they were)
  (b)  sv_bn254_kzg_open_device / sv_bn254_kzg_open: division + the same MSM in one call
  (c)  sv_bn254_fr_poly_div_linear_device alone, with and without the quotient (wall ms of the
       synchronous call, and HIP events on the stream around it: memset + kernels + the 64-B read-back)
  copy a plain elementwise kernel over the same n x 32 B (one read, one write), HIP events: the
       bandwidth the division's traffic floor is taken at -- 96 B per coefficient, the coefficients
       read twice and the quotient written once
  (d)  for context, the host path a caller had: a one-thread C++ Horner division
       (tools/ubench_host_horner, run when it has been built) in front of (a)
each the median of REPS calls after WARMUP.  Printed at the end per size: (b) - (a), (c) / (a) and
(c) / floor.  Before anything is timed the evaluation is checked against a Python-int Horner, the
two openings against each other and against the MSM over the division's own quotient.

  python tools/kzg_open_bench.py [--log-n 16 18 20] [--passes 3] [--reps 15]
"""
import argparse
import os
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
from svgpu import loader  # noqa: E402

SEED_B, SEED_S = 0x5EEDBA5E5, 0x5CA1A125
FORM = svgpu.SV_MONTGOMERY  # halo2curves' in-memory layout: what the Rust shim passes
Z = 0x1D0F5A17C3B2A49587766554433221100FFEEDDCCBBAA998877665544332211 % enc.R
HORNER_BIN = os.path.join(ROOT, "tools", "ubench_host_horner")


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


def horner_eval(limbs_mont, z):
    raw = limbs_mont.tobytes()
    rinv = pow(1 << 256, -1, enc.R)
    h = 0
    for i in range(len(raw) - 32, -1, -32):
        h = (int.from_bytes(raw[i:i + 32], "little") + z * h) % enc.R
    return h * rinv % enc.R  # the coefficients carry one factor 2^256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    svgpu.init(1)
    dev = torch.device("cuda:0")
    print(f"# {svgpu.version()}  form=montgomery passes={args.passes} reps={args.reps} warmup={args.warmup}")
    host = {}
    if os.path.exists(HORNER_BIN):
        out = subprocess.run([HORNER_BIN] + [str(lg) for lg in args.log_n], capture_output=True, text=True,
                             timeout=300).stdout
        for line in out.splitlines():
            print("(d) host Horner " + line)
            if line.startswith("2^"):
                host[int(line[2:line.index(":")])] = float(line.split()[1])
    else:
        print("(d) host Horner: not measured (tools/ubench_host_horner is not built)")
    # a stream of its own: the library then works on this stream (not on one from its pool), so the
    # events below bracket its kernels
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    for lg in args.log_n:
        n = 1 << lg
        dB = dv.gen_bases(dv.empty_bases(n, dev), SEED_B, 0, FORM)
        dA = dv.gen_scalars(dv.empty_scalars(n, dev), SEED_S, 0, FORM)
        torch.cuda.synchronize()
        hA = dA.cpu().numpy().view(np.uint64)
        rset = loader.ResidentBases.from_device(dB, FORM)
        del dB
        dQ = torch.empty((n - 1, 4), dtype=torch.int64, device=dev)
        ev, _ = dv.poly_div_linear_device(dA, Z, FORM, out=dQ)
        hQ = dQ.cpu().numpy().view(np.uint64)
        assert ev == horner_eval(hA, Z), f"2^{lg}: p(z) disagrees with the Python Horner"
        ref = (ev, rset.msm_device(dQ, 0, FORM))
        assert rset.open_device(dA, Z, 0, FORM) == ref, f"2^{lg}: open_device disagrees"
        assert rset.open_arrays(hA, Z, 0, FORM) == ref, f"2^{lg}: open (host coefficients) disagrees"
        assert dv.poly_div_linear_device(dA, Z, FORM, quotient=False)[0] == ev
        src = torch.empty((n, 4), dtype=torch.int64, device=dev).copy_(dA)
        dst = torch.empty_like(src)

        def copy_kernel():
            torch.add(src, 1, out=dst)
            torch.cuda.synchronize()

        run = {
            "a dev": lambda: rset.msm_device(dQ, 0, FORM),
            "a host": lambda: rset.msm_arrays(hQ, 0, FORM),
            "b dev": lambda: rset.open_device(dA, Z, 0, FORM),
            "b host": lambda: rset.open_arrays(hA, Z, 0, FORM),
            "c quot": lambda: dv.poly_div_linear_device(dA, Z, FORM, out=dQ),
            "c eval": lambda: dv.poly_div_linear_device(dA, Z, FORM, quotient=False),
            "copy": copy_kernel,
        }
        cols = {k: [] for k in run}
        for ps in range(args.passes):
            for k in run:
                cols[k].append(med_ms(run[k], args.reps, args.warmup))
            print(f"2^{lg} pass {ps} wall ms: " + "  ".join(f"({k}) {cols[k][-1][0]:.3f}" for k in run))
            print(f"2^{lg} pass {ps} event ms: " + "  ".join(f"({k}) {cols[k][-1][1]:.3f}" for k in run))
        wall = {k: statistics.median(v[0] for v in cols[k]) for k in run}
        evt = {k: statistics.median(v[1] for v in cols[k]) for k in run}
        bw = 2 * n * 32 / (evt["copy"] * 1e-3)  # bytes per second of the copy kernel
        floor = 96 * n / bw * 1e3
        print(f"2^{lg}: copy kernel {evt['copy'] * 1e3:.1f} us = {bw / 1e12:.2f} TB/s; division floor (96 B per "
              f"coefficient) {floor * 1e3:.1f} us")
        print(f"2^{lg}: (c) division with quotient {evt['c quot'] * 1e3:.1f} us events ({wall['c quot'] * 1e3:.1f} us "
              f"wall), evaluation only {evt['c eval'] * 1e3:.1f} us events; (c)/floor = {evt['c quot'] / floor:.2f}")
        print(f"2^{lg}: device coefficients (b) {wall['b dev']:.3f} - (a) {wall['a dev']:.3f} = "
              f"{wall['b dev'] - wall['a dev']:+.3f} ms; (c)/(a) = {evt['c quot'] / wall['a dev']:.3f}")
        print(f"2^{lg}: host coefficients   (b) {wall['b host']:.3f} - (a) {wall['a host']:.3f} = "
              f"{wall['b host'] - wall['a host']:+.3f} ms")
        if lg in host:
            print(f"2^{lg}: (d) host Horner {host[lg]:.3f} ms + (a host) {wall['a host']:.3f} = "
                  f"{host[lg] + wall['a host']:.3f} ms against (b host) {wall['b host']:.3f} ms")
        rset.close()


if __name__ == "__main__":
    main()
