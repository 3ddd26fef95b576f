"""Per-call switches of the single-MSM host path (msm_plan.hpp msm_tuning) that no other test sets,
each on one 20 000-point MSM (GLV on, c = 11, 12 windows) against the C++ oracle's Pippenger, over
host arrays (host-fed) and over device buffers.  tests/COVERAGE.md lists what each one reaches."""
import numpy as np
import pytest
import torch

from oracle import bn254 as b

pytestmark = pytest.mark.gpu

N = 20000
_CACHE = {}


def _case(oracle_cpp):
    if not _CACHE:
        B = oracle_cpp.gen_bases(b.SEED_BASES, N, start=8800)
        S = oracle_cpp.gen_scalars(b.SEED_SCALARS, N, start=8800)
        S[100:1500] = S[99]  # 1400 points in one bucket per window: chunks that cross no bucket boundary
        exp = b.g1_from_bytes(oracle_cpp.msm_pippenger(B, S, 0).tobytes())
        for a in (B, S):
            a.setflags(write=False)
        _CACHE["case"] = (B, S, exp)
    return _CACHE["case"]


@pytest.mark.parametrize("glv", ["0", "1"])
def test_every_window_width(gpu, oracle_cpp, monkeypatch, glv):
    """k_bin_hist<C, GLV> and k_bin_scatter<C, GLV> are instantiated for C = 4 .. 16, with and
    without the GLV split; the sizes and overrides of the other tests leave some of the 26 out
    (C = 6 either way, for one).  All of them here, on the device buffers."""
    import svgpu
    from svgpu import device as dv
    B, S, exp = _case(oracle_cpp)
    Bd = torch.from_numpy(np.array(B).view(np.int64)).to(gpu)
    Sd = torch.from_numpy(np.array(S).view(np.int64)).to(gpu)
    monkeypatch.setenv("SVGPU_GLV", glv)
    for c in range(4, 17):
        monkeypatch.setenv("SVGPU_WINDOW_BITS", str(c))
        assert dv.msm(Bd, Sd, svgpu.SV_CANONICAL) == exp, c


@pytest.mark.parametrize("env", [
    {"SVGPU_SCAN_KEYS": "16"},                           # k_bin_scan_tiles<16>
    {"SVGPU_MSM_LEAN": "1"},                              # no sort / reduce events
    {"SVGPU_FED_PREP": "0", "SVGPU_H2D_PIECES": "3"},     # the pieces' preparation on the compute stream
    {"SVGPU_ACC_K": "8"},                                 # short accumulate chunks: most buckets cross chunks
    {"SVGPU_ACC_K": "64"},
    {"SVGPU_RED_LOG": "1"},                               # 512 running-sum segments per window (the tree)
    {"SVGPU_RED_LOG": "4"},                               # 64 segments: k_wsum + k_group_sum_q
    {"SVGPU_GROUP_TREE": "0", "SVGPU_GROUP_P": "1"},      # one k_group_sum_q block per group
    {"SVGPU_GROUP_TREE": "0", "SVGPU_GROUP_P": "4"},
    {"SVGPU_GROUP_TREE": "0", "SVGPU_GROUP_QUAD": "0", "SVGPU_GROUP_P": "4"},  # k_group_sum
    {"SVGPU_GLV_MAX_LOG": "13"},                          # no GLV at this size: 255-bit scalars, 24 windows
    {"SVGPU_ACC_R29": "0", "SVGPU_GLV": "0"},             # host-fed, 32-bit chain, no table: k_check_bases
], ids=lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_single_msm_switch(gpu, oracle_cpp, monkeypatch, env):
    import svgpu
    from svgpu import device as dv
    B, S, exp = _case(oracle_cpp)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert svgpu.msm_arrays(B, S) == exp
    Bd = torch.from_numpy(np.array(B).view(np.int64)).to(gpu)
    Sd = torch.from_numpy(np.array(S).view(np.int64)).to(gpu)
    assert dv.msm(Bd, Sd, svgpu.SV_CANONICAL) == exp
