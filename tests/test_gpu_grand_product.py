"""Running products and batch inversion on the device (sv_bn254_fr_grand_product_device,
sv_bn254_fr_batch_invert_device; csrc/grand_product.hip) against Python-int arithmetic, bit for bit,
in both forms.

Expected values.  z[i] = z0 N_<i / D_<i with the rows' products formed in Python from the same
columns, a zero denominator product replaced by the ratio 0 / 1, and pow(D, -1, r) for the division;
the one large size is checked by cross-multiplication (z[i] D_<i = z0 N_<i: it pins z[i] because no
D_<i is zero after the replacement) and needs no Python inversion.  Nothing expected comes from the
code under test.  A case (columns, factor lists, per-row products) is built once per (shape, n) and
shared; no test modifies it.

Sizes.  P = kGpPer rows per thread, S = kGpSpan rows per block, T = kGpThreads (read from
csrc/grand_product.hpp): n in {1, 2, 3, P - 1, P, P + 1, S - 1, S, S + 1, 2 S + 1, 3 S - 1} covers
part of a thread, a thread, part of a block, a block, and two and three blocks with a one-row and an
all-but-one-row tail; n = T S + S + 1 gives the carries kernel two totals per thread.
tests/COVERAGE_grand_product.md has the ledger."""
import functools
import os
import random
import re

import numpy as np
import pytest

from conftest import PKG
from oracle import bn254 as b
from test_gpu_kzg_open import _dev, _ints, _limb_bytes, _limbs
from test_gpu_resident_bases import _UNREDUCED

pytestmark = pytest.mark.gpu

_HPP = open(os.path.join(PKG, "csrc", "grand_product.hpp")).read()
S = int(re.search(r"constexpr uint32_t kGpSpan = (\d+);", _HPP).group(1))
T = int(re.search(r"constexpr uint32_t kGpThreads = (\d+);", _HPP).group(1))
assert "kGpPer = kGpSpan / kGpThreads" in _HPP
P = S // T
R = b.R
ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c
CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
PLAIN, COLUMN, IDENTITY = 0, 1, 2
MAX = 16
SIZES = sorted({1, 2, 3, P - 1, P, P + 1, S - 1, S, S + 1, 2 * S + 1, 3 * S - 1})
LARGE = T * S + S + 1
SHAPES = ["num1", "den1", "lookup", "perm3"]
BETA, GAMMA, Z0_GEN, C1 = (b.gen_scalar(b.SEED_SCALARS, 919100 + i) for i in range(4))
DELTA = 7                                                   # 7^j is in no 2^k-th roots' coset for small j > 0
RINV = pow(1 << 256, -1, R)


def _omega(n):
    """The root of the smallest domain that holds n rows."""
    k = max(n - 1, 0).bit_length()
    return pow(ROOT_OF_UNITY, 1 << (28 - k), R)


@functools.lru_cache(maxsize=None)
def _column(n, tag):
    """n generated scalars with 0, 1 and r - 1 planted at the first, the middle and the last row; a
    column of fewer than 8 rows takes one of the three, chosen by the tag, so that the columns of a
    small case still differ."""
    from oracle import cpu_ref
    a = _ints(cpu_ref.gen_scalars(b.SEED_SCALARS, n, start=(40 + tag) << 22))
    if n < 8:
        a[tag % n] = (0, 1, R - 1)[tag % 3]
        return tuple(a)
    for i, e in zip((0, n // 2, n - 1), (0, 1, R - 1)):
        a[i] = e
    return tuple(a)


class Case:
    """Columns (name -> canonical ints), the two factor lists over their names, omega."""

    def __init__(self, n, cols, num, den, omega=None):
        self.n, self.cols, self.num, self.den, self.omega = n, cols, num, den, omega
        self._rows = None

    def rows(self):
        """[(numerator product, denominator product)] per row, the 0 / 1 rule applied."""
        if self._rows is None:
            out, w = [], 1
            for i in range(self.n):
                nv = dv = 1
                for side, fs in ((0, self.num), (1, self.den)):
                    for kind, x, y, s, c in fs:
                        f = self.cols[x][i] + c
                        if kind == COLUMN:
                            f += s * self.cols[y][i]
                        elif kind == IDENTITY:
                            f += s * w
                        if side:
                            dv = dv * f % R
                        else:
                            nv = nv * f % R
                if self.omega is not None:
                    w = w * self.omega % R
                out.append((0, 1) if dv == 0 else (nv, dv))
            self._rows = out
        return self._rows

    def expected(self, z0):
        """(z, total) by division."""
        z, cur = [], z0 % R
        for nv, dv in self.rows():
            z.append(cur)
            cur = cur * nv % R * pow(dv, -1, R) % R
        return z, cur

    def with_column(self, name, values):
        cols = dict(self.cols)
        cols[name] = tuple(values)
        return Case(self.n, cols, self.num, self.den, self.omega)


def _permutation_case(n):
    """Three columns over the cells (j, i) with labels delta^j omega^i: a real permutation of the
    cells in cycles of 1 .. 5, one value per cycle (the first three: 0, 1, r - 1), sigma_j[i] = the
    label of the cell after (j, i) in its cycle."""
    w = _omega(n)
    rng = random.Random(7700 + n)
    cells = [(j, i) for j in range(3) for i in range(n)]
    rng.shuffle(cells)
    wp = [1] * n
    for i in range(1, n):
        wp[i] = wp[i - 1] * w % R
    label = lambda j, i: pow(DELTA, j, R) * wp[i] % R  # noqa: E731
    values = [[0] * n for _ in range(3)]
    sigma = [[0] * n for _ in range(3)]
    at, cyc = 0, 0
    while at < len(cells):
        ln = min(rng.randint(1, 5), len(cells) - at)
        val = (0, 1, R - 1)[cyc] if cyc < 3 else b.gen_scalar(b.SEED_SCALARS, 929000 + cyc)
        for k in range(ln):
            j, i = cells[at + k]
            nj, ni = cells[at + (k + 1) % ln]
            values[j][i], sigma[j][i] = val, label(nj, ni)
        at, cyc = at + ln, cyc + 1
    cols = {f"v{j}": tuple(values[j]) for j in range(3)}
    cols.update({f"sigma{j}": tuple(sigma[j]) for j in range(3)})
    num = [(IDENTITY, f"v{j}", None, BETA * pow(DELTA, j, R) % R, GAMMA) for j in range(3)]
    den = [(COLUMN, f"v{j}", f"sigma{j}", BETA, GAMMA) for j in range(3)]
    return Case(n, cols, num, den, w)


@functools.lru_cache(maxsize=None)
def _case(shape, n):
    if shape == "num1":
        return Case(n, {"a": _column(n, 0)}, [(PLAIN, "a", None, 0, C1)], [])
    if shape == "den1":
        return Case(n, {"a": _column(n, 1)}, [], [(PLAIN, "a", None, 0, C1)])
    if shape == "lookup":
        cols = {name: _column(n, 2 + k) for k, name in enumerate(("a", "s", "ap", "sp"))}
        return Case(n, cols, [(PLAIN, "a", None, 0, BETA), (PLAIN, "s", None, 0, GAMMA)],
                    [(PLAIN, "ap", None, 0, BETA), (PLAIN, "sp", None, 0, GAMMA)])
    if shape == "perm3":
        return _permutation_case(n)
    assert shape == "max"
    cols = {name: _column(n, 6 + k) for k, name in enumerate("abcd")}
    sc = [b.gen_scalar(b.SEED_SCALARS, 939000 + i) for i in range(4 * MAX)]
    kinds, names = (PLAIN, COLUMN, IDENTITY), "abcd"
    num = [(kinds[j % 3], names[j % 4], names[(j + 1) % 4], sc[2 * j], sc[2 * j + 1]) for j in range(MAX)]
    den = [(kinds[(j + 1) % 3], names[(j + 2) % 4], names[(j + 3) % 4], sc[2 * MAX + 2 * j], sc[2 * MAX + 2 * j + 1])
           for j in range(MAX)]
    return Case(n, cols, num, den, _omega(n))


def _run(case, z0, form, gpu, out=None, override=None):
    """-> (z tensor, total).  override: name -> limb array to upload in place of the case's column."""
    from svgpu import device as dv
    override = override or {}
    cols = {name: _dev(override[name] if name in override else _limbs(list(v), form), gpu)
            for name, v in case.cols.items()}
    num = [dv.Factor(kind, cols[x], cols[y] if kind == COLUMN else None, s, c) for kind, x, y, s, c in case.num]
    den = [dv.Factor(kind, cols[x], cols[y] if kind == COLUMN else None, s, c) for kind, x, y, s, c in case.den]
    return dv.grand_product_device(num, den, z0=z0, omega=case.omega, form=form, out=out)


def _check(case, z0, gpu):
    want_z, want_total = case.expected(z0)
    for form in FORMS:
        z, total = _run(case, z0, form, gpu)
        assert tuple(z.shape) == (case.n, 4)
        assert total == want_total, ("total", form)
        assert z.cpu().numpy().tobytes() == _limb_bytes(want_z, form), ("z", form)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_sizes(gpu, oracle_cpp, shape, n):
    case = _case(shape, n)
    if shape == "perm3":
        _, total = case.expected(1)
        assert all(dv for _, dv in case.rows())
        if n & (n - 1) == 0:
            assert total == 1, "a real permutation with equal values along its cycles multiplies to 1"
    _check(case, Z0_GEN, gpu)


@pytest.mark.parametrize("z0", [1, 0], ids=["one", "zero"])
@pytest.mark.parametrize("shape", SHAPES)
def test_z0_one_and_zero(gpu, oracle_cpp, shape, z0):
    _check(_case(shape, S + 1), z0, gpu)


def test_most_factors_on_each_side(gpu, oracle_cpp):
    case = _case("max", S + 1)
    assert len(case.num) == len(case.den) == MAX
    _check(case, Z0_GEN, gpu)


@pytest.mark.parametrize("pos", ["0", "S-1", "S", "n-1"])
@pytest.mark.parametrize("shape", ["den1", "lookup", "perm3"])
def test_zero_denominator_zeroes_the_rest(gpu, oracle_cpp, shape, pos):
    n = 2 * S + 1
    at = {"0": 0, "S-1": S - 1, "S": S, "n-1": n - 1}[pos]
    base = _case(shape, n)
    kind, x, y, s, c = base.den[-1]
    col = list(base.cols[x])
    # the factor x + s y + c at row `at` becomes zero
    col[at] = -(c + (s * base.cols[y][at] if kind == COLUMN else 0)) % R
    case = base.with_column(x, col)
    assert case.rows()[at] == (0, 1)
    want_z, want_total = case.expected(Z0_GEN)
    assert want_total == 0 and not any(want_z[at + 1:]) and all(want_z[:at + 1])
    _check(case, Z0_GEN, gpu)


@pytest.mark.parametrize("shape", ["num1", "lookup"])
def test_zero_numerator(gpu, oracle_cpp, shape):
    n = 2 * S + 1
    base = _case(shape, n)
    kind, x, y, s, c = base.num[0]
    col = list(base.cols[x])
    col[S - 1] = -c % R
    case = base.with_column(x, col)
    want_z, want_total = case.expected(Z0_GEN)
    assert want_total == 0 and not any(want_z[S:]) and all(want_z[:S])
    _check(case, Z0_GEN, gpu)


def test_large_size_by_cross_multiplication(gpu, oracle_cpp):
    """n = T S + S + 1: the carries kernel folds two totals per thread.  z[i] D_<i = z0 N_<i."""
    case = _case("lookup", LARGE)
    rows = case.rows()
    assert all(dv for _, dv in rows)
    pn, pd, N, D = [], [], Z0_GEN, 1
    for nv, dv in rows:
        pn.append(N)
        pd.append(D)
        N, D = N * nv % R, D * dv % R
    for form in FORMS:
        z, total = _run(case, Z0_GEN, form, gpu)
        got = _ints(z.cpu().numpy().view(np.uint64))
        if form == MONTGOMERY:
            got = [v * RINV % R for v in got]
        assert len(got) == LARGE
        bad = [i for i in range(LARGE) if got[i] * pd[i] % R != pn[i]]
        assert not bad, (form, bad[:5])
        assert total * D % R == N, form


def test_unreduced_element_at_a_span_boundary(gpu, oracle_cpp):
    import svgpu
    n = 2 * S + 1
    for shape, name in (("lookup", "sp"), ("perm3", "sigma1"), ("num1", "a")):
        case = _case(shape, n)
        want_z, want_total = case.expected(Z0_GEN)
        for form in FORMS:
            for at in (S - 1, S):
                bad = _limbs(list(case.cols[name]), form)
                bad[at] = _UNREDUCED
                with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                    _run(case, Z0_GEN, form, gpu, override={name: bad})
                z, total = _run(case, Z0_GEN, form, gpu)          # the next call on the same pool
                assert total == want_total and z.cpu().numpy().tobytes() == _limb_bytes(want_z, form)


def test_wrapper_out_and_refusals(gpu, oracle_cpp):
    import torch
    import svgpu
    from svgpu import device as dv
    case = _case("lookup", S + 1)
    want_z, want_total = case.expected(1)
    out = torch.zeros((S + 1, 4), dtype=torch.int64, device=gpu)
    z, total = _run(case, 1, CANONICAL, gpu, out=out)
    assert z.data_ptr() == out.data_ptr() and total == want_total
    assert out.cpu().numpy().tobytes() == _limb_bytes(want_z, CANONICAL)
    a = _dev(_limbs(list(case.cols["a"]), CANONICAL), gpu)
    with pytest.raises(svgpu.LengthError):
        dv.grand_product_device([(PLAIN, a)], [], out=torch.zeros((S, 4), dtype=torch.int64, device=gpu))
    with pytest.raises(svgpu.LengthError):
        dv.grand_product_device([(PLAIN, a)], [(PLAIN, a[:S])])
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        dv.grand_product_device([(PLAIN, a)], [], out=a)
    with pytest.raises(svgpu.ArgumentError, match="omega"):
        dv.grand_product_device([(IDENTITY, a, None, 1, 0)], [])
    with pytest.raises(svgpu.EmptyError):
        dv.grand_product_device([], [])
    # a short tuple takes the defaults s = c = 0: the plain prefix product of the column
    z, total = svgpu.grand_product_device([(PLAIN, a)], [], form=CANONICAL)
    assert total == 0 and _ints(z[:2].cpu().numpy().view(np.uint64)) == [1, 0]      # a[0] is the planted 0


# ---- batch inversion ------------------------------------------------------------------------------

def _invert_column(n):
    """The generated column with zeros at rows 0, S - 1, S and n - 1 (those that exist)."""
    a = list(_column(n, 12))
    for at in (0, S - 1, S, n - 1):
        if at < n:
            a[at] = 0
    if n > 2:
        a[1] = 1
    if n > 3:
        a[2] = R - 1
    return a


def _check_inverses(a, got):
    assert len(got) == len(a)
    bad = [i for i, (x, y) in enumerate(zip(a, got)) if (y != 0 if x == 0 else x * y % R != 1) or y >= R]
    assert not bad, bad[:5]


@pytest.mark.parametrize("n", SIZES + [LARGE])
def test_batch_inversion(gpu, oracle_cpp, n):
    from svgpu import device as dv
    a = _invert_column(n)
    for form in FORMS:
        x = _dev(_limbs(a, form), gpu)
        keep = x.clone()
        out = dv.batch_invert_device(x, form=form)
        assert out.data_ptr() != x.data_ptr() and tuple(out.shape) == (n, 4)
        assert x.equal(keep), "out of place: the input is only read"
        got = _ints(out.cpu().numpy().view(np.uint64))
        if form == MONTGOMERY:
            got = [v * RINV % R for v in got]
        _check_inverses(a, got)
        same = dv.batch_invert_device(x, form=form, out=x)                        # in place
        assert same.data_ptr() == x.data_ptr() and x.equal(out)


def test_batch_inversion_refusals(gpu, oracle_cpp):
    import torch
    import svgpu
    from svgpu import device as dv
    n = 2 * S + 1
    a = _invert_column(n)
    for form in FORMS:
        good = _limbs(a, form)
        want = dv.batch_invert_device(_dev(good, gpu), form=form)
        for at in (S - 1, S):
            bad = good.copy()
            bad[at] = _UNREDUCED
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                dv.batch_invert_device(_dev(bad, gpu), form=form)
            assert dv.batch_invert_device(_dev(good, gpu), form=form).equal(want)
        got = _ints(want.cpu().numpy().view(np.uint64))
        _check_inverses(a, [v * RINV % R for v in got] if form == MONTGOMERY else got)
    buf = torch.zeros((12, 4), dtype=torch.int64, device=gpu)
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        dv.batch_invert_device(buf[0:8], out=buf[1:9])
    with pytest.raises(svgpu.LengthError):
        dv.batch_invert_device(buf[0:8], out=buf[0:4])
    with pytest.raises(svgpu.ArgumentError):
        dv.batch_invert_device(torch.zeros((4, 5), dtype=torch.int64, device=gpu))
    assert svgpu.batch_invert_device(buf[0:3], form=CANONICAL).equal(buf[0:3])   # zeros stay zero
