"""Child process of tests/test_gpu_streams.py::test_cold_key_decide_on_a_side_stream (not collected
by pytest).

The decider uploads a key's prepared lines on the call's stream the first time it sees the key
(decider.hip decider_lines), so only a process that has not decided yet reaches that upload.  This
one makes its first decide under a side stream: the accumulators of tests/stream_cases.py's decider
case are uploaded under that stream and decided there, with verdicts and Gt.  It exits non-zero
unless first failure, verdicts and every Gt limb equal oracle_cpp.decide_all's.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from oracle import cpu_ref  # noqa: E402

import stream_cases as sc  # noqa: E402


def main():
    assert svgpu.init() >= 1
    gpu = torch.device("cuda:0")
    g2, sg2, L, R = sc.decider_case([2], 0)
    want = sc.decider_expected(cpu_ref, g2, sg2, L, R)
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(gpu).cuda_stream != 0
        ff, verdicts, gts = dv.decide(g2, sg2, sc.dev(L, gpu), sc.dev(R, gpu), svgpu.SV_CANONICAL, want_gt=True)
        drained = side.query()
    got = (ff, [bool(v) for v in verdicts], [[int(x) for x in g] for g in gts])
    bad = []
    if not drained:
        bad.append("the side stream had not drained on return")
    for name, g, w in zip(("first failure", "verdicts", "Gt"), got, want):
        if g != w:
            bad.append(f"{name}: {g if name != 'Gt' else '...'} != {w if name != 'Gt' else '...'}")
    if bad:
        print("MISMATCH " + "; ".join(bad), flush=True)
        return 1
    print("OK", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
