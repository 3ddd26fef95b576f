"""Child process of tests/test_gpu_process_switches.py::test_msm_switches_read_once (not collected
by pytest).

SVGPU_SORT_XCD and SVGPU_SORT_BM (msm_plan.hpp msm_tuning) and SVGPU_GATHER_AHEAD (api.cpp) are
read once per process, so only a process started with the variable set runs the other side.  This
one runs one MSM of n points under whatever SVGPU_* its environment holds -- over host arrays
(argument "arrays": sv_bn254_g1_msm, and the device entry point on the same data) or over shuffled
references (argument "refs": sv_bn254_g1_msm_refs) -- and exits non-zero unless the result equals
the C++ oracle's Pippenger.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "snark-verifier-axiom_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import svgpu  # noqa: E402
from svgpu import device as dv  # noqa: E402
from oracle import bn254 as b  # noqa: E402
from oracle import cpu_ref  # noqa: E402


def main():
    mode, n = sys.argv[1], int(sys.argv[2])
    assert svgpu.init() >= 1
    B = cpu_ref.gen_bases(b.SEED_BASES, n, start=7100)
    S = cpu_ref.gen_scalars(b.SEED_SCALARS, n, start=7100)
    exp = b.g1_from_bytes(cpu_ref.msm_pippenger(B, S, 0).tobytes())
    got = {}
    if mode == "arrays":
        got["host arrays"] = svgpu.msm_arrays(B, S)
        dev = torch.device("cuda:0")
        got["device"] = dv.msm(torch.from_numpy(B.view(np.int64)).to(dev), torch.from_numpy(S.view(np.int64)).to(dev),
                               svgpu.SV_CANONICAL)
    elif mode == "refs":
        perm = np.random.default_rng(23).permutation(n).astype(np.uint64)
        refs = svgpu.make_refs(S.ctypes.data + 32 * perm, B.ctypes.data + 64 * perm)
        got["references"] = svgpu.msm_refs(refs)
    else:
        print("usage: msm_variant_child.py arrays|refs n", flush=True)
        return 2
    bad = [k for k, v in got.items() if v != exp]
    if bad:
        print("MISMATCH " + ", ".join(bad), flush=True)
        return 1
    print("OK", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
