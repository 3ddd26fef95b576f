"""Degenerate additions through every bucket reduction of the single-MSM pipeline: the lattice cases
of tests/degenerate_cases.py (bucket sums that are equal, opposite, cancelled or the identity at a
chosen level of the reduction; tests/test_degenerate_cases.py proves on the CPU which operand
classes each case brings to each level) against the closed form ((sum s_i m_i) mod r) P, or the
oracle's Pippenger where random rows are mixed in.

Every call runs the pipeline (SVGPU_SMALL_MSM=0) at a forced window width c and segment length, with
the GLV split off and on -- every scalar is below 2^125, so the split leaves it alone and the same
arrays fill the same buckets -- and asserts the window width and count from sv_msm_last_stats.  The
reduction that msm_plan (msm_plan.hpp) picks for that width:

  c = 11 with GLV (logL = 2), c = 12 without (logL = 3): 256 segments a window, one tree block:
          k_wsum_tree<true, R29> + k_group_fin; SVGPU_GROUP_TREE=0: k_wsum + k_group_sum(_q)
  c = 9,  SVGPU_GROUP_TREE=2: 256 buckets, k_wsum_tree<false>
  c = 13 with GLV / 14 without: 1024 segments, 4 blocks a window (k_group_fin's first two levels)
  c = 12 / 16, SVGPU_GROUP_TREE=2: 8 / 128 blocks a window; 128 is the only plan with more than 64
          members in k_group_fin (wave 1 into wave 0): the default tree stops at 64 blocks
"""
import numpy as np
import pytest
import torch

import degenerate_cases as dc
from oracle import bn254 as b

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def rand_rows(oracle_cpp):
    return oracle_cpp.gen_bases(b.SEED_BASES, 1 << 12, start=424242)


def _expected(case, oracle_cpp):
    key = ("exp", case.name)
    if key not in _CACHE:
        _CACHE[key] = dc.expected_point(case, oracle_cpp)
    return _CACHE[key]


def _assert_route(c, glv):
    """The pipeline ran, at window width c, with or without the split (as _last_route, test_gpu_msm.py)."""
    from svgpu import device as dv
    s = dv.last_msm_stats()
    assert (s["window_bits"], s["num_windows"]) == (c, -(-(128 if glv else 255) // c)), s


def _env(monkeypatch, c, red_log, glv, **more):
    monkeypatch.setenv("SVGPU_SMALL_MSM", "0")
    monkeypatch.setenv("SVGPU_WINDOW_BITS", str(c))
    monkeypatch.setenv("SVGPU_RED_LOG", str(red_log))
    monkeypatch.setenv("SVGPU_GLV", str(glv))
    for k, v in more.items():
        monkeypatch.setenv("SVGPU_" + k, str(v))


def _device(case, gpu):
    key = ("dev", case.name)
    if key not in _CACHE:
        _CACHE[key] = (torch.from_numpy(case.bases.view(np.int64)).to(gpu),
                       torch.from_numpy(case.scalars.view(np.int64)).to(gpu))
    return _CACHE[key]


def _run_device(case, gpu, oracle_cpp, c, glv):
    import svgpu
    from svgpu import device as dv
    Bd, Sd = _device(case, gpu)
    assert dv.msm(Bd, Sd, svgpu.SV_CANONICAL) == _expected(case, oracle_cpp), case.name
    _assert_route(c, glv)


# (GLV, c, logL) with 256 segments a window
PLANS = [(1, 11, 2), (0, 12, 3)]


@pytest.mark.parametrize("r29", ["1", "0"])
@pytest.mark.parametrize("glv,c,red_log", PLANS)
def test_default_tree(gpu, oracle_cpp, rand_rows, monkeypatch, glv, c, red_log, r29):
    """k_wsum_tree<true, true> (the 29-bit running sums: r29::add) and <true, false> (SVGPU_ACC_R29=0:
    xyzz_add_2p) + k_group_fin: doublings and cancellations in `run + cur`, `acc + run` and at every
    level of the in-block tree; a wave with doubling and generic quads side by side; the stored
    cancelled record; host_combine's a == b and a == -b."""
    _env(monkeypatch, c, red_log, glv, ACC_R29=r29)
    for case in (_case(("levels", c, red_log), lambda: dc.case_levels(c, red_log)),
                 _case(("mixed", c, red_log), lambda: dc.case_mixed(c, red_log, rand_rows))):
        _run_device(case, gpu, oracle_cpp, c, glv)


@pytest.mark.parametrize("glv", [0, 1])
def test_pure_tree(gpu, oracle_cpp, rand_rows, monkeypatch, glv):
    """SVGPU_GROUP_TREE=2 at c = 9: k_wsum_tree<false> over the 256 buckets of a window (levels 1
    and 2 as whole additions, the rest in quad form)."""
    _env(monkeypatch, 9, 0, glv, GROUP_TREE=2)
    for case in (_case(("levels", 9, 0), lambda: dc.case_levels(9, 0)),
                 _case(("mixed", 9, 0), lambda: dc.case_mixed(9, 0, rand_rows))):
        _run_device(case, gpu, oracle_cpp, 9, glv)


@pytest.mark.parametrize("glv,c,red_log,tree,levels", [
    (1, 13, 2, 1, (8, 9)), (0, 14, 3, 1, (8, 9)), (1, 12, 0, 2, (8, 9, 10)), (1, 16, 0, 2, (14,))])
def test_group_fin_blocks(gpu, oracle_cpp, monkeypatch, glv, c, red_log, tree, levels):
    """k_group_fin over 4, 8 and 128 blocks a window: equal and opposite block outputs in a quad's two
    additions, in the in-wave levels and (128 blocks) in wave 1 into wave 0.  Only the case's few
    windows are filled."""
    _env(monkeypatch, c, red_log, glv, GROUP_TREE=tree)
    case = _case(("blocks", c, red_log, levels), lambda: dc.case_blocks(c, red_log, levels))
    _run_device(case, gpu, oracle_cpp, c, glv)


@pytest.mark.parametrize("glv,c,red_log", PLANS)
@pytest.mark.parametrize("quad,parts", [("1", 1), ("1", 4), ("0", 1), ("0", 4)])
def test_wsum_and_group_sums(gpu, oracle_cpp, rand_rows, monkeypatch, glv, c, red_log, quad, parts):
    """SVGPU_GROUP_TREE=0: k_wsum + k_group_sum_q, and k_group_sum under SVGPU_GROUP_QUAD=0, with one
    and four blocks a group (at 4 the last block's fold of part[] adds equal and opposite slices)."""
    _env(monkeypatch, c, red_log, glv, GROUP_TREE=0, GROUP_QUAD=quad, GROUP_P=parts)
    for case in (_case(("levels", c, red_log), lambda: dc.case_levels(c, red_log)),
                 _case(("mixed", c, red_log), lambda: dc.case_mixed(c, red_log, rand_rows))):
        _run_device(case, gpu, oracle_cpp, c, glv)


@pytest.mark.parametrize("glv,c,red_log", PLANS)
@pytest.mark.parametrize("tree", [1, 0])
def test_three_pieces(gpu, oracle_cpp, monkeypatch, glv, c, red_log, tree):
    """The sections +mult, -mult, +mult host-fed in three pieces (k_accumulate<true, *>: piece 2 ends
    every bucket on the identity, piece 3 starts from those records; no bucket is empty by gst),
    device-resident in one piece (P, -P, P in every bucket) and through a ResidentBases set."""
    import svgpu
    size = 12288 if c == 11 else 20480
    case = _case(("pieces", c, red_log), lambda: dc.case_pieces(c, red_log, size))
    exp = _expected(case, oracle_cpp)
    assert exp is not None
    _env(monkeypatch, c, red_log, glv, GROUP_TREE=tree, H2D_PIECES=3)
    assert svgpu.msm_arrays(case.bases, case.scalars, svgpu.SV_CANONICAL, num_gpus=1) == exp
    _assert_route(c, glv)
    _run_device(case, gpu, oracle_cpp, c, glv)
    with svgpu.ResidentBases(case.bases) as rs:
        assert rs.msm_arrays(case.scalars) == exp
        _assert_route(c, glv)
        Sd = _device(case, gpu)[1]
        assert rs.msm_device(Sd, form=svgpu.SV_CANONICAL) == exp
        _assert_route(c, glv)


def test_fold_partials(gpu, oracle_cpp):
    """sv_bn254_g1_fold (host code; it sits here beside the partials it folds): Jacobian partials with
    Z != 1 out of msm_partial, and O with Z = 0 and non-zero X, Y."""
    import svgpu
    from svgpu import device as dv
    B = oracle_cpp.gen_bases(b.SEED_BASES, 300, start=5)
    S = oracle_cpp.gen_scalars(b.SEED_SCALARS, 300, start=5)
    p = dv.msm_partial(torch.from_numpy(B.view(np.int64)).to(gpu), torch.from_numpy(S.view(np.int64)).to(gpu),
                       svgpu.SV_CANONICAL)
    assert p[2] % b.P not in (0, 1)
    a = b.jac_to_affine(p)
    assert a == b.g1_from_bytes(oracle_cpp.msm_pippenger(B, S, 0).tobytes())
    n = (p[0], (-p[1]) % b.P, p[2])
    O = (p[0], p[1], 0)
    for parts, want in (([p, p], b.g1_add(a, a)), ([p, n], None), ([O, p], a), ([p, O], a), ([O, O], None),
                        ([p, p, n, n, p], a)):
        assert svgpu.fold_partials(parts) == want


@pytest.mark.parametrize("n", [8, 300])
def test_kzg_accumulate_equal_and_opposite(gpu, n):
    """sv_bn254_kzg_accumulate on the small route (k_batch_uwin) and above it (n = 300: the pipeline):
    every lhs the same point and rhs = -lhs, so every bucket sums copies of one point."""
    import svgpu
    r = 0x1234567890ABCDEF1234567890ABCDEF % b.R
    P = dc.lattice().P
    acc = svgpu.KzgAs.create_proof([svgpu.KzgAccumulator(P, b.g1_neg(P))] * n, r)
    k = sum(pow(r, i, b.R) for i in range(n)) % b.R
    want = b.g1_mul(P, k)
    assert (acc.lhs, acc.rhs) == (want, b.g1_neg(want))
