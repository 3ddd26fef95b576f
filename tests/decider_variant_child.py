"""Child process of tests/test_gpu_process_switches.py::test_decider_switches_read_once (not
collected by pytest).

decider.hip reads SVGPU_DECIDER_KC and SVGPU_DECIDER_PHASES into function-local statics on the
first decide of a process, so only a process started with the variable set runs the other side.
This one runs the 12-accumulator case of test_gpu_decider.py::test_decider_prologue_variants (bad
index 7, an identity pair, an rhs identity) under whatever SVGPU_DECIDER_* its environment holds
and exits non-zero unless verdicts, first failure and every Gt limb equal oracle_cpp.decide_all's.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from svgpu import encoding as enc  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import cpu_ref  # noqa: E402


def main():
    assert svgpu.init() >= 1
    dev = torch.device("cuda:0")
    n = 12
    g2, sg2, accs = b.gen_decider_case(n, seed=0xC0DE, bad=[7])
    accs[4] = (None, None)                                      # identity pair: passes
    accs[9] = (accs[9][0], None)                                # rhs identity: e(lhs, g2) != 1
    L, R = enc.bases_array([a[0] for a in accs]), enc.bases_array([a[1] for a in accs])
    ff, verdicts, gts = dv.decide(g2, sg2, torch.from_numpy(L.view(np.int64)).to(dev),
                                  torch.from_numpy(R.view(np.int64)).to(dev), svgpu.SV_CANONICAL, want_gt=True)
    eff, egt = cpu_ref.decide_all(np.frombuffer(b.g2_bytes(g2), np.uint64), np.frombuffer(b.g2_bytes(sg2), np.uint64),
                                  L, R, threads=0, want_gt=True)
    bad = []
    if not (ff == eff == 7):
        bad.append(f"first failure {ff}, oracle {eff}")
    one = [1] + [0] * 11                                        # Gt's identity: the verdict of the oracle's value
    for i in range(n):
        want = [enc.limbs_to_int(egt[i][4 * c:4 * c + 4]) for c in range(12)]
        if [int(x) for x in gts[i]] != want:
            bad.append(f"Gt of accumulator {i}")
        if bool(verdicts[i]) != (want == one):
            bad.append(f"verdict of accumulator {i}: {verdicts[i]}")
    if bad:
        print("MISMATCH " + "; ".join(bad), flush=True)
        return 1
    print("OK", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
