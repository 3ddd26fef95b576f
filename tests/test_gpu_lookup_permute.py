"""A lookup's permuted columns on the device (sv_bn254_fr_lookup_permute_device;
csrc/lookup_permute.hip) against the direct restatement of halo2's permute_expression_pair
(tests/lookup_permute_cases.permute_direct: a Counter and pop()), bit for bit, in both forms, and
the three relations the verifier checks on the device's output.  Nothing expected comes from the
code under test.  Sizes as in test_gpu_fr_sort.py (SIZES, and LARGE = T TILE + 1 where k_lp_carries
takes two totals per thread); a case is built once per (shape, n) and shared.
tests/COVERAGE_lookup_permute.md has the ledger."""
import ctypes
import functools
import random

import numpy as np
import pytest

import lookup_permute_cases as lp
from test_gpu_fr_sort import CANONICAL, FORMS, LARGE, MONTGOMERY, SIZES, TILE
from test_gpu_kzg_open import _dev, _ints, _limb_bytes, _limbs
from test_gpu_resident_bases import _UNREDUCED

pytestmark = pytest.mark.gpu

R = lp.R
RINV = pow(1 << 256, -1, R)
BETA, GAMMA, Z0 = 0x1234567 ** 9 % R, 0x89ABCDE ** 9 % R, 0xFEDCBA ** 9 % R


def _distinct(n, seed):
    out = set()
    rng = random.Random(seed)
    while len(out) < n:
        out.add(rng.randrange(R))
    out = list(out)
    rng.shuffle(out)
    return out


def _heavy_repeats(n):
    s = lp.plant(_distinct(n, 1000 + n))
    rng = random.Random(1100 + n)
    few = [s[0], s[n // 2], s[n - 1]] + [rng.choice(s) for _ in range(max(1, n // 16))]
    return [rng.choice(few) for _ in range(n)], s


def _permutation(n):
    s = lp.plant(_distinct(n, 1200 + n))
    a = list(s)
    random.Random(1300 + n).shuffle(a)
    return a, s


def _constant_input(n):
    s = lp.plant(_distinct(n, 1400 + n))
    return [s[n // 3]] * n, s


def _constant_both(n):
    return [R - 1] * n, [R - 1] * n


def _duplicated_table(n):
    """v twice and w three times in the table and both looked up: one copy of v and two of w are
    left over, among the other leftovers."""
    s = _distinct(n, 1500 + n)
    v, w = s[0], s[1]
    s[2], s[3], s[4] = v, w, w
    rng = random.Random(1600 + n)
    rng.shuffle(s)
    a = [v, w] + [rng.choice(s) for _ in range(n - 2)]
    rng.shuffle(a)
    return a, s


def _range_table(n):
    """A 16-bit range table (its n first values, shuffled) and random inputs from it: two live digits."""
    s = [i % 65536 for i in range(n)]
    rng = random.Random(1700 + n)
    rng.shuffle(s)
    return [rng.choice(s) for _ in range(n)], s


SHAPES = {"heavy-repeats": (_heavy_repeats, 1), "permutation": (_permutation, 1), "constant-input": (_constant_input, 1),
          "constant-both": (_constant_both, 1), "duplicated-table": (_duplicated_table, 5), "range-table": (_range_table, 1)}


@functools.lru_cache(maxsize=None)
def _case(shape, n):
    a, s = SHAPES[shape][0](n)
    ap, sp, row = lp.permute_direct(a, s)
    assert row is None
    return tuple(a), tuple(s), tuple(ap), tuple(sp)


def _run(a, s, form, gpu, **kw):
    from svgpu import device as dv
    return dv.lookup_permute_device(_dev(_limbs(list(a), form), gpu), _dev(_limbs(list(s), form), gpu), form=form, **kw)


def _decode(t, form):
    v = _ints(t.cpu().numpy().view(np.uint64))
    return [x * RINV % R for x in v] if form == MONTGOMERY else v


def _check(shape, n, gpu):
    a, s, ap, sp = _case(shape, n)
    for form in FORMS:
        gap, gsp = _run(a, s, form, gpu)
        assert gap.cpu().numpy().tobytes() == _limb_bytes(ap, form), (shape, n, form)
        assert gsp.cpu().numpy().tobytes() == _limb_bytes(sp, form), (shape, n, form)
        lp.check_relations(a, s, _decode(gap, form), _decode(gsp, form), BETA, GAMMA)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_permuted_columns_match_the_direct_restatement(gpu, shape):
    for n in SIZES:
        if n >= SHAPES[shape][1]:
            _check(shape, n, gpu)


def test_case_shapes_are_what_they_claim():
    n = TILE + 1
    a, s, ap, sp = _case("permutation", n)
    assert len(set(a)) == n and ap == sp                                   # no repeats, L empty
    a, s, ap, sp = _case("constant-input", n)
    assert sp[0] == ap[0] and list(sp[1:]) == sorted(set(s) - {ap[0]}, reverse=True)   # the leftover, reversed
    a, s, ap, sp = _case("duplicated-table", n)
    assert sorted(sp) == sorted(s) and max(s.count(v) for v in set(s)) == 3
    a, s, ap, sp = _case("range-table", 3 * TILE - 1)
    assert max(s) < 1 << 16 and len(set(a)) < len(a)


def test_carries_scan_takes_two_totals_per_thread(gpu):
    _check("heavy-repeats", LARGE, gpu)


def _missing_cases():
    """name -> (a, s, the row the case is built to fail at, or None where only the restatement says)."""
    n = TILE + 1
    s = sorted(_distinct(n, 2000))
    assert s[0] > 5 and s[-1] < R - 5
    rng = random.Random(2001)
    inner = s[n // 4: 3 * n // 4]
    base = [rng.choice(inner) for _ in range(n)]
    gap = next(v + 1 for v in inner[len(inner) // 2:] if v + 1 not in s)   # between two table values

    def with_values(*vals):
        a = list(base)
        for k, v in enumerate(vals):
            a[(k * 97 + 11) % n] = v
        return a
    leaders = lambda a: len(set(a))  # noqa: E731
    cases = {
        "first-leader-below-min": (with_values(s[0] - 1), s, 0),
        "first-leader": (with_values(s[2] + 1 if s[2] + 1 not in s else s[2] + 2), s, 0),
        "middle-leader": (with_values(gap), s, None),
        "last-leader": (with_values(s[-2] + 1 if s[-2] + 1 not in s else s[-2] + 2), s, n - 1),
        "last-leader-above-max": (with_values(s[-1] + 1), s, n - 1),
        "two-missing": (with_values(s[-1] + 1, gap), s, None),
        "repeated-missing": (with_values(gap, gap, gap), s, None),
        "n-1-missing": ([7], [8], 0),
        "n-3-above": ([1, 9, 1], [1, 5, 5], 2),
    }
    assert 0 < sorted(cases["middle-leader"][0]).index(gap) < n - 1 and leaders(cases["middle-leader"][0]) > 3
    return cases


@pytest.mark.parametrize("name", list(_missing_cases()))
def test_missing_value_reports_the_smallest_row(gpu, name):
    import svgpu
    a, s, built_row = _missing_cases()[name]
    ap, sp, row = lp.permute_direct(a, s)
    assert ap is None and row is not None and (built_row is None or row == built_row)
    assert lp.permute_sorted(a, s) == (None, None, row)
    for form in FORMS:
        with pytest.raises(svgpu.ArgumentError, match="not in table") as e:
            _run(a, s, form, gpu)
        assert e.value.row == row and f"row {row} " in str(e.value)
        # out_missing_row NULL: the same status and message; then a good call on the same pool sets UINT64_MAX
        A, S = _dev(_limbs(a, form), gpu), _dev(_limbs(s, form), gpu)
        import torch
        from svgpu import _lib
        o1, o2 = torch.empty_like(A), torch.empty_like(A)
        rc = _lib.lib.sv_bn254_fr_lookup_permute_device(A.data_ptr(), S.data_ptr(), len(a), form, o1.data_ptr(),
                                                        o2.data_ptr(), None, 0, None)
        assert rc == _lib.SV_ERR_ARG and "not in table" in _lib.last_error()
        got = ctypes.c_uint64(5)
        rc = _lib.lib.sv_bn254_fr_lookup_permute_device(S.data_ptr(), S.data_ptr(), len(a), form, o1.data_ptr(),
                                                        o2.data_ptr(), ctypes.byref(got), 0, None)
        assert rc == _lib.SV_OK and got.value == (1 << 64) - 1
        want = _limb_bytes(sorted(s), form)
        assert o1.cpu().numpy().tobytes() == want and (len(set(s)) < len(s) or o2.cpu().numpy().tobytes() == want)


def test_unreduced_in_either_column_wins_over_a_missing_value(gpu):
    import svgpu
    n = 2 * TILE + 1
    a, s, ap, sp = _case("heavy-repeats", n)
    miss = list(a)
    miss[5] = next(v for v in range(2, 100) if v not in s)                 # a missing value as well
    for form in FORMS:
        for column in (0, 1):
            for at in (TILE - 1, TILE):
                for inputs in (a, miss):
                    cols = [_limbs(list(inputs), form), _limbs(list(s), form)]
                    cols[column][at] = _UNREDUCED
                    from svgpu import device as dv
                    with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                        dv.lookup_permute_device(_dev(cols[0], gpu), _dev(cols[1], gpu), form=form)
                gap, gsp = _run(a, s, form, gpu)                            # the next call on the same pool
                assert gap.cpu().numpy().tobytes() == _limb_bytes(ap, form)
                assert gsp.cpu().numpy().tobytes() == _limb_bytes(sp, form)


def test_wrapper_out_inputs_unchanged_and_refusals(gpu):
    import torch
    import svgpu
    from svgpu import device as dv
    n = TILE + 1
    a, s, ap, sp = _case("duplicated-table", n)
    A, S = _dev(_limbs(list(a), CANONICAL), gpu), _dev(_limbs(list(s), CANONICAL), gpu)
    ka, ks = A.clone(), S.clone()
    out = (torch.zeros_like(A), torch.zeros_like(A))
    gap, gsp = dv.lookup_permute_device(A, S, form=CANONICAL, out=out)
    assert (gap.data_ptr(), gsp.data_ptr()) == (out[0].data_ptr(), out[1].data_ptr())
    assert gap.cpu().numpy().tobytes() == _limb_bytes(ap, CANONICAL) and gsp.cpu().numpy().tobytes() == _limb_bytes(sp, CANONICAL)
    assert A.equal(ka) and S.equal(ks)                                      # the inputs are only read
    buf = torch.zeros((4 * n + 2, 4), dtype=torch.int64, device=gpu)
    free1, free2 = buf[2 * n + 1:3 * n + 1], buf[3 * n + 1:4 * n + 1]
    for bad in ((A, free1), (free1, A), (S, free1), (free1, S), (free1, free1), (free1, buf[2 * n + 2:3 * n + 2])):
        with pytest.raises(svgpu.ArgumentError, match="overlaps"):
            dv.lookup_permute_device(A, S, form=CANONICAL, out=bad)
    Ab = buf[0:n]
    Ab.copy_(A)
    for bad in ((buf[1:n + 1], free2), (free2, buf[n - 1:2 * n - 1])):          # one element into / in front of an input
        with pytest.raises(svgpu.ArgumentError, match="overlaps"):
            dv.lookup_permute_device(Ab, S, form=CANONICAL, out=bad)
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_device(A, S[:n - 1])
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_device(A, S, out=(free1, free2[:n - 1]))
    with pytest.raises(svgpu.ArgumentError):
        dv.lookup_permute_device(A, torch.zeros((n, 5), dtype=torch.int64, device=gpu))
    # the two inputs may be one column: A looked up in itself
    gap, gsp = svgpu.lookup_permute_device(A, A, form=CANONICAL)
    want = lp.permute_direct(a, a)
    assert _decode(gap, CANONICAL) == want[0] and _decode(gsp, CANONICAL) == want[1]


def test_lookup_argument_end_to_end(gpu):
    """The permutation followed by the existing lookup_product: total == z0 for a lookup that holds,
    and z equal to Python-int arithmetic on the restatement's A', S'."""
    import svgpu
    n = TILE + 1
    a, s, ap, sp = _case("heavy-repeats", n)
    z, cur = [], Z0
    for x, y, xp, yp in zip(a, s, ap, sp):
        z.append(cur)
        cur = cur * (x + BETA) % R * (y + GAMMA) % R * pow((xp + BETA) * (yp + GAMMA) % R, -1, R) % R
    assert cur == Z0
    for form in FORMS:
        A, S = _dev(_limbs(list(a), form), gpu), _dev(_limbs(list(s), form), gpu)
        gap, gsp, gz, total = svgpu.lookup_argument(A, S, BETA, GAMMA, z0=Z0, form=form)
        assert total == Z0
        assert gap.cpu().numpy().tobytes() == _limb_bytes(ap, form) and gsp.cpu().numpy().tobytes() == _limb_bytes(sp, form)
        assert gz.cpu().numpy().tobytes() == _limb_bytes(z, form)
