"""The multi-point pass (sv_bn254_fr_poly_eval_points_device; svgpu.device.poly_eval_points_device):
every p_j(x_k) of m polynomials in HBM at K points, each polynomial read once.

No expected value comes from the code under test: every evaluation is the Python-int Horner of
test_gpu_kzg_open.  Everything is arithmetic mod r, so every comparison is bit for bit.

Sizes.  The pass works in spans of kDivSpan coefficients (S) and takes kPointsPerLaunch points (KP)
per launch, both read from csrc/kzg_open.hpp: lengths 1, 2, S - 1, S, S + 1, 2 S + 1 and lengths
that differ inside one call (one shorter than K); K = 1, 2, KP (one full launch), KP + 1 (a second
launch of one point) and 16 (the limit: four full launches).  The only other size at which a loop
count changes is the fold's, 256 S + 1, where a thread folds two span totals.  Inside a launch the
K trees lie in one array, so what can go wrong is a pair taking another tree's weight: the points
of one call are therefore all different where the case allows it (and 0, 1, r - 1 are among them),
and one case repeats a point on purpose."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import PKG
from oracle import bn254 as b
from test_gpu_kzg_open import _dev, _horner, _ints, _limbs
from test_gpu_resident_bases import EDGE, N, _UNREDUCED

pytestmark = pytest.mark.gpu

_HPP = open(os.path.join(PKG, "csrc", "kzg_open.hpp")).read()
S = int(re.search(r"constexpr uint32_t kDivSpan = (\d+);", _HPP).group(1))
THREADS = int(re.search(r"constexpr uint32_t kDivThreads = (\d+);", _HPP).group(1))
KP = int(re.search(r"constexpr uint32_t kPointsPerLaunch = (\d+);", _HPP).group(1))
FOLD_STEP = THREADS * S + 1
CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
Z = [b.gen_scalar(b.SEED_SCALARS, 424200 + i) for i in range(16)]
# K points per K: 0, 1 and r - 1 among different generated values; the last list of K = KP + 1 repeats a point
POINTS = {
    1: [[0], [1], [b.R - 1], [Z[0]]],
    2: [[0, Z[0]], [b.R - 1, 1], [Z[1], Z[2]]],
    KP: [([0, 1, b.R - 1] + Z)[:KP], Z[:KP]],
    KP + 1: [(Z[:KP - 1] + [0, b.R - 1, 1])[:KP + 1], Z[:KP] + [Z[1]]],
    16: [Z[:5] + [0] + Z[5:9] + [1] + Z[9:12] + [b.R - 1, Z[3]]],
}
assert all(len(p) == k for k, ps in POINTS.items() for p in ps) and sorted(POINTS) == sorted({1, 2, KP, KP + 1, 16})

_POOL = {}


def _poly(oracle_cpp, j, n):
    """Polynomial j (of up to 2 S + 1 coefficients, the EDGE values among them), cut to n."""
    if j not in _POOL:
        a = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, 2 * S + 1, start=(50 + j) * N))
        e = EDGE[j % len(EDGE):] + EDGE[:j % len(EDGE)]
        for i, x in enumerate(e):  # spread over the whole length; the first two also lead every cut
            a[i * 2 * S // (len(e) - 1)] = x
        a[0], a[1] = e[0], e[1]
        _POOL[j] = a
    return _POOL[j][:n]


def _expected(polys, points):
    return [[_horner(a, x)[1] for x in points] for a in polys]


def _check(polys, gpu, ks=tuple(POINTS), forms=FORMS):
    from svgpu import device as dv
    for form in forms:
        A = [_dev(_limbs(a, form), gpu) for a in polys]
        for k in ks:
            for points in POINTS[k]:
                assert dv.poly_eval_points_device(A, points, form=form) == _expected(polys, points), (form, points)


@pytest.mark.parametrize("n", [1, 2, S - 1, S, S + 1, 2 * S + 1])
@pytest.mark.parametrize("m", [1, 3])
def test_eval_points_equal_lengths(gpu, oracle_cpp, m, n):
    _check([_poly(oracle_cpp, j, n) for j in range(m)], gpu)


@pytest.mark.parametrize("lens", [[2 * S + 1, 3, S, 1, S + 1], [1, 2 * S, 2, 2 * S + 1], [3, 1, 2]])
def test_eval_points_unequal_lengths(gpu, oracle_cpp, lens):
    """Polynomials shorter than K (1, 2, 3 coefficients at 5 and 16 points), ones that end inside a
    span, at a span's end, and whole spans before the longest."""
    _check([_poly(oracle_cpp, j, l) for j, l in enumerate(lens)], gpu, ks=(2, KP + 1, 16))


def test_eval_points_special_polynomials(gpu):
    """All zero, only the first coefficient, only the last: at S + 1 the last one is alone in its span."""
    n = S + 1
    polys = [[0] * n, [b.R - 2] + [0] * (n - 1), [0] * (n - 1) + [b.R - 3]]
    _check(polys, gpu, ks=(KP, KP + 1))


def test_eval_points_where_the_fold_takes_two_totals_per_thread(gpu, oracle_cpp):
    a = _ints(oracle_cpp.gen_scalars(b.SEED_SCALARS, FOLD_STEP, start=60 * N))
    a[-1] = b.R - 1
    polys = [a, a[1:]]
    points = [Z[0], b.R - 1]
    want = _expected(polys, points)
    from svgpu import device as dv
    for form in FORMS:
        A = [_dev(_limbs(p, form), gpu) for p in polys]
        assert dv.poly_eval_points_device(A, points, form=form) == want, form


def test_eval_points_equal_the_single_point_passes(gpu, oracle_cpp):
    """What a caller did before: one evaluate-only pass per point."""
    from svgpu import device as dv
    polys = [_poly(oracle_cpp, j, l) for j, l in enumerate([2 * S + 1, S + 1, 77])]
    A = [_dev(_limbs(a, MONTGOMERY), gpu) for a in polys]
    points = POINTS[KP + 1][0]
    per_point = [dv.poly_combine_eval_device(A, x, 1, form=MONTGOMERY, combined=False)[0] for x in points]
    assert dv.poly_eval_points_device(A, points, form=MONTGOMERY) == [list(col) for col in zip(*per_point)]


def test_the_same_tensor_twice_and_row_slices(gpu, oracle_cpp):
    import numpy as np
    from svgpu import device as dv
    a = _poly(oracle_cpp, 0, 2 * S + 1)
    A = _dev(_limbs(a, CANONICAL), gpu)
    points = POINTS[KP + 1][1]
    e = _expected([a], points)[0]
    assert dv.poly_eval_points_device([A, A, A], points, form=CANONICAL) == [e, e, e]
    # two polynomials as slices of one buffer from odd rows; the inputs are only read
    rows = np.zeros((2 * S + 8, 4), np.uint64)
    rows[1:1 + S + 1] = _limbs(a[:S + 1], CANONICAL)
    rows[S + 5:S + 5 + 300] = _limbs(a[:300], CANONICAL)
    buf = _dev(rows, gpu)
    got = dv.poly_eval_points_device([buf[1:S + 2], buf[S + 5:S + 305]], points, form=CANONICAL)
    assert got == _expected([a[:S + 1], a[:300]], points)
    assert buf.cpu().numpy().tobytes() == rows.tobytes()


def test_unreduced_coefficient_rejected_and_the_next_call_is_exact(gpu, oracle_cpp):
    import svgpu
    from svgpu import device as dv
    lens = [2 * S + 1, S + 1, 3]
    polys = [_poly(oracle_cpp, j, l) for j, l in enumerate(lens)]
    for form in FORMS:
        good = [_limbs(a, form) for a in polys]
        G = [_dev(a, gpu) for a in good]
        for k in (1, KP + 1):
            points = POINTS[k][-1]
            want = _expected(polys, points)
            for j in range(3):
                for idx in (0, lens[j] // 2, lens[j] - 1):
                    bad = good[j].copy()
                    bad[idx] = _UNREDUCED
                    with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                        dv.poly_eval_points_device(G[:j] + [_dev(bad, gpu)] + G[j + 1:], points, form=form)
                    assert dv.poly_eval_points_device(G, points, form=form) == want, (form, k, j, idx)
    with pytest.raises(svgpu.ArgumentError, match="point 1 not reduced"):
        dv.poly_eval_points_device(G, [5, b.R], form=CANONICAL)


def test_four_threads_at_once(gpu, oracle_cpp):
    """Calls are re-entrant (ctypes releases the GIL around every foreign call, so they overlap)."""
    from svgpu import device as dv
    jobs = [([2 * S + 1, 5], POINTS[16][0]), ([S, S + 1, 1], POINTS[KP][0]), ([3], POINTS[KP + 1][1]),
            ([S - 1, 2 * S], POINTS[2][1])]
    work = []
    for lens, points in jobs:
        polys = [_poly(oracle_cpp, j, l) for j, l in enumerate(lens)]
        work.append(([_dev(_limbs(a, CANONICAL), gpu) for a in polys], points, _expected(polys, points)))

    def run(k):
        A, points, want = work[k]
        return [dv.poly_eval_points_device(A, points, form=CANONICAL) == want for _ in range(3)]

    with ThreadPoolExecutor(max_workers=4) as ex:
        results = list(ex.map(run, range(4)))
    assert all(all(r) for r in results), results
