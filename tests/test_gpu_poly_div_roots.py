"""Division by several roots (sv_bn254_fr_poly_div_roots_device; svgpu.device.poly_div_roots_device):
the quotient of p by prod_k (X - x_k), remainder dropped.

The expected quotient is the Python-int synthetic division of test_gpu_kzg_open, once per root.
Everything is arithmetic mod r, so every comparison is bit for bit.

Sizes.  The call runs K three-launch divisions, each over the quotient before it (one coefficient
shorter each time, in Montgomery form in scratch, in two buffers by turns): n = K + 1 (one quotient
coefficient), S - 1, S, S + 1, S + K (the last run starts exactly at a span's end) and 2 S + 1 around
kDivSpan (S, read from csrc/kzg_open.hpp); K = 1 (no scratch buffer), 2 (one), 3 (both), 5 (each
reused)."""
import os
import re

import numpy as np
import pytest

from conftest import PKG
from oracle import bn254 as b
from test_gpu_kzg_open import _dev, _div_coeffs, _horner, _limb_bytes, _limbs
from test_gpu_resident_bases import _UNREDUCED

pytestmark = pytest.mark.gpu

S = int(re.search(r"constexpr uint32_t kDivSpan = (\d+);", open(os.path.join(PKG, "csrc", "kzg_open.hpp")).read()).group(1))
CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
X = [b.gen_scalar(b.SEED_SCALARS, 535300 + i) for i in range(5)]
ROOTS = {1: [[X[0]], [0], [b.R - 1]], 2: [[0, X[0]], [X[1], X[2]]], 3: [[1, b.R - 1, X[0]], X[:3]],
         5: [[X[0], 0, 1, b.R - 1, X[0]], X]}  # the first list of K = 5 repeats a root


def _div_roots(a, roots):
    for x in roots:
        a, _ = _horner(a, x)
    return a


@pytest.mark.parametrize("K", sorted(ROOTS))
@pytest.mark.parametrize("where", ["K + 1", "S - 1", "S", "S + 1", "S + K", "2 S + 1"])
def test_quotient_by_several_roots(gpu, oracle_cpp, where, K):
    from svgpu import device as dv
    n = {"K + 1": K + 1, "S - 1": S - 1, "S": S, "S + 1": S + 1, "S + K": S + K, "2 S + 1": 2 * S + 1}[where]
    a = _div_coeffs(oracle_cpp, n, "generated")
    for form in FORMS:
        A = _dev(_limbs(a, form), gpu)
        for roots in ROOTS[K]:
            q = _div_roots(a, roots)
            assert len(q) == n - K
            Q = dv.poly_div_roots_device(A, roots, form=form)
            assert tuple(Q.shape) == (n - K, 4)
            assert Q.cpu().numpy().tobytes() == _limb_bytes(q, form), (n, roots, form)


@pytest.mark.parametrize("n", [2, S, S + 1, 2 * S + 1])
def test_one_root_is_the_linear_division_bit_for_bit(gpu, oracle_cpp, n):
    from svgpu import device as dv
    a = _div_coeffs(oracle_cpp, n, "generated")
    for form in FORMS:
        A = _dev(_limbs(a, form), gpu)
        for x in (0, b.R - 1, X[0]):
            _, lin = dv.poly_div_linear_device(A, x, form=form)
            assert dv.poly_div_roots_device(A, [x], form=form).cpu().numpy().tobytes() == lin.cpu().numpy().tobytes()


def test_special_polynomials(gpu):
    """All zero; only the first coefficient (the quotient is zero); only the last (X^(n-1))."""
    from svgpu import device as dv
    n = S + 3
    for a in ([0] * n, [b.R - 2] + [0] * (n - 1), [0] * (n - 1) + [b.R - 3]):
        for roots in (ROOTS[3][0], ROOTS[5][1]):
            Q = dv.poly_div_roots_device(_dev(_limbs(a, CANONICAL), gpu), roots, form=CANONICAL)
            assert Q.cpu().numpy().tobytes() == _limb_bytes(_div_roots(a, roots), CANONICAL)


def test_rejections_and_the_next_call_is_exact(gpu, oracle_cpp):
    import svgpu
    from svgpu import device as dv
    n, roots = S + 1, ROOTS[3][1]
    a = _div_coeffs(oracle_cpp, n, "generated")
    want = _limb_bytes(_div_roots(a, roots), CANONICAL)
    good = _limbs(a, CANONICAL)
    G = _dev(good, gpu)
    for idx in (0, S - 1, n - 1):
        bad = good.copy()
        bad[idx] = _UNREDUCED
        with pytest.raises(svgpu.ArgumentError, match="not reduced"):
            dv.poly_div_roots_device(_dev(bad, gpu), roots, form=CANONICAL)
        assert dv.poly_div_roots_device(G, roots, form=CANONICAL).cpu().numpy().tobytes() == want
    with pytest.raises(svgpu.ArgumentError, match="no quotient"):
        dv.poly_div_roots_device(G[:3], roots, form=CANONICAL)
    # the quotient over the coefficients: rows [n, 2 n) hold them, the n - 3 quotient rows start at row s
    rows = np.zeros((3 * n, 4), np.uint64)
    rows[n:2 * n] = good
    buf = _dev(rows, gpu)
    for s in (4, n, 2 * n - 1):
        with pytest.raises(svgpu.ArgumentError, match="overlaps"):
            dv.poly_div_roots_device(buf[n:2 * n], roots, form=CANONICAL, out=buf[s:])
    with pytest.raises(svgpu.LengthError):
        dv.poly_div_roots_device(buf[n:2 * n], roots, form=CANONICAL, out=buf[:n - 4])
    assert buf.cpu().numpy().tobytes() == rows.tobytes()
    for s in (3, 2 * n):
        assert dv.poly_div_roots_device(buf[n:2 * n], roots, form=CANONICAL, out=buf[s:]).cpu().numpy().tobytes() == want
    assert buf[n:2 * n].cpu().numpy().tobytes() == rows[n:2 * n].tobytes()
