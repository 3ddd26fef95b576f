"""The batched lookup permutation on the device (sv_bn254_fr_lookup_permute_batch_device;
csrc/lookup_permute.hip, csrc/lp_batch_plan.hpp) against the direct restatement of halo2's
permute_expression_pair (tests/lookup_permute_cases.permute_direct: a Counter and pop()), per lookup,
bit for bit, in both forms.  Nothing expected comes from the code under test.  Sizes are those of
test_gpu_fr_sort.py (SIZES, and LARGE = T TILE + 1 in one test, where k_lpb_carries takes two totals per
thread); a column and a lookup's expected pair are built once and shared.
tests/COVERAGE_lookup_permute_batch.md has the ledger."""
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
MAX = (1 << 64) - 1


def _distinct(n, seed):
    out = set()
    rng = random.Random(seed)
    while len(out) < n:
        out.add(rng.randrange(R))
    out = list(out)
    rng.shuffle(out)
    return out


# ---- tables, and inputs drawn from a given table -------------------------------------------------

@functools.lru_cache(maxsize=None)
def _table(kind, n, tag=0):
    if kind == "full-width":                     # distinct values, 0, 1 and r - 1 among them: 32 live digits
        return tuple(lp.plant(_distinct(n, 7000 + 31 * tag + n)))
    if kind == "range-table":                    # a 16-bit range table, shuffled: two live digits
        s = [i % 65536 for i in range(n)]
        random.Random(7100 + 31 * tag + n).shuffle(s)
        return tuple(s)
    if kind == "one-digit":                      # keys that differ in digit 13 only: one live digit
        return tuple(lp.one_digit(n, 13, 7200 + 31 * tag + n))
    if kind == "constant":                       # no live digit
        return (R - 1,) * n
    raise KeyError(kind)


def _input(shape, s, seed):
    """A column of len(s) values that are all in s."""
    n, rng = len(s), random.Random(seed)
    if shape == "heavy-repeats":
        few = [s[0], s[n // 2], s[n - 1]] + [rng.choice(s) for _ in range(max(1, n // 16))]
        return [rng.choice(few) for _ in range(n)]
    if shape == "permutation":
        a = list(s)
        rng.shuffle(a)
        return a
    if shape == "constant-input":
        return [s[n // 3]] * n
    if shape == "range-table":                   # uniform picks, as the range-table shape of the single call's tests
        return [rng.choice(s) for _ in range(n)]
    raise KeyError(shape)


INPUT_SHAPES = ("heavy-repeats", "permutation", "constant-input", "range-table")


@functools.lru_cache(maxsize=None)
def _shared_lookup(kind, n, j):
    """Lookup j against the one table of `kind`: its input shape goes round INPUT_SHAPES."""
    s = _table(kind, n)
    a = _input(INPUT_SHAPES[j % 4], s, 7300 + 17 * j + n)
    return tuple(a), s


@functools.lru_cache(maxsize=None)
def _expected(a, s):
    ap, sp, row = lp.permute_direct(list(a), list(s))
    assert row is None
    return tuple(ap), tuple(sp)


def _col(values, form, gpu):
    return _dev(_limbs(list(values), form), gpu)


def _decode(t, form):
    v = _ints(t.cpu().numpy().view(np.uint64))
    return [x * RINV % R for x in v] if form == MONTGOMERY else v


def _assert_pair(got, a, s, form, what):
    ap, sp = _expected(tuple(a), tuple(s))
    assert got[0].cpu().numpy().tobytes() == _limb_bytes(list(ap), form), ("permuted input", what, form)
    assert got[1].cpu().numpy().tobytes() == _limb_bytes(list(sp), form), ("permuted table", what, form)


def _run_and_check(lookups, form, gpu, share=True, **kw):
    """lookups: [(a, s)] as tuples of ints.  Tables that are the same tuple are one tensor when `share`."""
    from svgpu import device as dv
    tabs = {}
    A = [_col(a, form, gpu) for a, _ in lookups]
    S = []
    for _, s in lookups:
        if not share or id(s) not in tabs:
            tabs[id(s)] = _col(s, form, gpu)
        S.append(tabs[id(s)])
    got = dv.lookup_permute_batch_device(A, S, form=form, **kw)
    assert len(got) == len(lookups)
    for j, (a, s) in enumerate(lookups):
        _assert_pair(got[j], a, s, form, (j, len(a)))
    return A, S, got


# ---- 1. one table for every lookup ---------------------------------------------------------------

@pytest.mark.parametrize("kind", ["full-width", "range-table"])
@pytest.mark.parametrize("count", [1, 2, 3, 16])
def test_shared_table(gpu, count, kind):
    import svgpu
    for n in SIZES:
        lookups = [_shared_lookup(kind, n, j) for j in range(count)]
        for form in FORMS:
            A, S, _ = _run_and_check(lookups, form, gpu)
            assert len({t.data_ptr() for t in S}) == 1
            if count == 3 and n == TILE + 1:      # `tables` as one tensor means "shared by all"
                got = svgpu.lookup_permute_batch_device(A, S[0], form=form)
                for j, (a, s) in enumerate(lookups):
                    _assert_pair(got[j], a, s, form, j)


# ---- 2. columns of different liveness in one launch ----------------------------------------------

@functools.lru_cache(maxsize=None)
def _mixed(n):
    """Four lookups with distinct tables: 2, 1, 0 and 32 live digits."""
    out = []
    for tag, (kind, shape) in enumerate((("range-table", "range-table"), ("one-digit", "range-table"),
                                         ("constant", "constant-input"), ("full-width", "heavy-repeats"))):
        s = _table(kind, n, tag=1 + tag)
        out.append((tuple(_input(shape, s, 7400 + tag + n)), s))
    return tuple(out)


@pytest.mark.parametrize("rotation", range(4))
@pytest.mark.parametrize("n", [TILE + 1, 3 * TILE - 1])
def test_mixed_liveness_in_every_rotation(gpu, n, rotation):
    lookups = _mixed(n)
    assert max(lookups[0][1]) < 1 << 16 and len(set(lookups[2][0]) | set(lookups[2][1])) == 1
    differ = {v ^ lookups[1][1][0] for v in lookups[1][1]}
    assert len(differ) > 2 and all(d & ~(0xFF << (8 * 13)) == 0 for d in differ)   # one digit, several values
    order = lookups[rotation:] + lookups[:rotation]
    for form in FORMS:
        _run_and_check(list(order), form, gpu)


# ---- 3. which lookups share a table --------------------------------------------------------------

def test_tables_a_b_a(gpu):
    n = 2 * TILE + 1
    sa, sb = _table("full-width", n, tag=6), _table("range-table", n, tag=7)
    lookups = [(tuple(_input("heavy-repeats", sa, 1)), sa), (tuple(_input("range-table", sb, 2)), sb),
               (tuple(_input("permutation", sa, 3)), sa)]
    for form in FORMS:
        _, S, _ = _run_and_check(lookups, form, gpu)
        assert S[0].data_ptr() == S[2].data_ptr() != S[1].data_ptr()


def test_sixteen_distinct_tables_and_sixteen_copies_of_one(gpu):
    n = TILE + 1
    distinct = []
    for j in range(16):
        s = _table(("full-width", "range-table", "one-digit")[j % 3], n, tag=10 + j)
        distinct.append((tuple(_input(INPUT_SHAPES[j % 4], s, 7500 + j)), s))
    for form in FORMS:
        _, S, _ = _run_and_check(distinct, form, gpu)
        assert len({t.data_ptr() for t in S}) == 16
    # equal contents behind distinct pointers are distinct tables all the same
    same = [_shared_lookup("full-width", n, j) for j in range(16)]
    _, S, _ = _run_and_check(same, MONTGOMERY, gpu, share=False)
    assert len({t.data_ptr() for t in S}) == 16


def test_two_table_pointers_that_overlap(gpu):
    import torch
    from svgpu import device as dv
    n, shift = TILE + 1, 5
    long = _table("full-width", n + shift, tag=30)
    s0, s1 = long[:n], long[shift:]
    a0, a1 = _input("heavy-repeats", s0, 4), _input("heavy-repeats", s1, 5)
    for form in FORMS:
        buf = _col(long, form, gpu)
        T0, T1 = buf[:n], buf[shift:]
        assert T0.data_ptr() != T1.data_ptr() and T1.data_ptr() < T0.data_ptr() + 32 * n
        keep = buf.clone()
        got = dv.lookup_permute_batch_device([_col(a0, form, gpu), _col(a1, form, gpu)], [T0, T1], form=form)
        _assert_pair(got[0], a0, s0, form, 0)
        _assert_pair(got[1], a1, s1, form, 1)
        assert torch.equal(buf, keep)


def test_one_input_in_two_lookups_against_different_tables(gpu):
    from svgpu import device as dv
    n = 3 * TILE - 1
    common = _distinct(n // 2, 7600)
    s0 = tuple(common + _distinct(n - n // 2, 7601))
    s1 = tuple(_distinct(n - n // 2, 7602) + common)
    a = [random.Random(7603).choice(common) for _ in range(n)]
    for form in FORMS:
        A = _col(a, form, gpu)
        got = dv.lookup_permute_batch_device([A, A], [_col(s0, form, gpu), _col(s1, form, gpu)], form=form)
        _assert_pair(got[0], a, s0, form, 0)
        _assert_pair(got[1], a, s1, form, 1)
        assert got[0][0].cpu().numpy().tobytes() == got[1][0].cpu().numpy().tobytes()


# ---- 4. tables the caller has sorted -------------------------------------------------------------

def test_presorted_tables_give_the_same_bytes(gpu):
    from svgpu import device as dv
    for n in SIZES:
        sa, sb = _table("full-width", n, tag=40), _table("range-table", n, tag=41)   # the second has equal neighbours
        lookups = [(tuple(_input("heavy-repeats", sa, 6)), sa), (tuple(_input("range-table", sb, 7)), sb),
                   (tuple(_input("permutation", sa, 8)), sa)]
        for form in FORMS:
            TA, TB = dv.sort_device(_col(sa, form, gpu), form=form), dv.sort_device(_col(sb, form, gpu), form=form)
            assert TA.cpu().numpy().tobytes() == _limb_bytes(sorted(sa), form)
            got = dv.lookup_permute_batch_device([_col(a, form, gpu) for a, _ in lookups], [TA, TB, TA], form=form,
                                                 tables_sorted=True)
            for j, (a, s) in enumerate(lookups):
                _assert_pair(got[j], a, s, form, (j, n))


def test_equal_neighbours_are_sorted(gpu):
    from svgpu import device as dv
    n = TILE + 1
    s = sorted(_table("full-width", n, tag=42))
    s[TILE - 1] = s[TILE] = s[TILE - 2]                                   # three equal across the tile boundary
    s[1] = s[0]
    a = _input("heavy-repeats", s, 9)
    for form in FORMS:
        got = dv.lookup_permute_batch_device([_col(a, form, gpu)], [_col(s, form, gpu)], form=form, tables_sorted=True)
        _assert_pair(got[0], a, s, form, 0)
    got = dv.lookup_permute_batch_device([_col([R - 1] * n, CANONICAL, gpu)], [_col([R - 1] * n, CANONICAL, gpu)],
                                         form=CANONICAL, tables_sorted=True)
    _assert_pair(got[0], [R - 1] * n, [R - 1] * n, CANONICAL, "all equal")


@pytest.mark.parametrize("where", ["0/1", "TILE-1/TILE", "n-2/n-1"])
def test_a_swapped_pair_is_table_not_sorted(gpu, where):
    import svgpu
    from svgpu import device as dv
    n = 2 * TILE + 1
    at = {"0/1": 0, "TILE-1/TILE": TILE - 1, "n-2/n-1": n - 2}[where]
    good = sorted(_table("full-width", n, tag=43))
    bad = list(good)
    bad[at], bad[at + 1] = bad[at + 1], bad[at]
    a = _input("heavy-repeats", good, 10)
    miss = list(a)
    miss[7] = next(v for v in range(2, 100) if v not in good)               # "table not sorted" wins over "not in table"
    for form in FORMS:
        for inputs in (a, miss):
            with pytest.raises(svgpu.ArgumentError, match="table not sorted"):
                dv.lookup_permute_batch_device([_col(a, form, gpu), _col(inputs, form, gpu)],
                                               [_col(good, form, gpu), _col(bad, form, gpu)], form=form, tables_sorted=True)
        # without the flag the same columns are fine, and so is the next call with it
        got = dv.lookup_permute_batch_device([_col(a, form, gpu)], [_col(bad, form, gpu)], form=form)
        _assert_pair(got[0], a, bad, form, "unsorted, no flag")
        got = dv.lookup_permute_batch_device([_col(a, form, gpu)], [_col(good, form, gpu)], form=form, tables_sorted=True)
        _assert_pair(got[0], a, good, form, "sorted again")


# ---- 5. failures ---------------------------------------------------------------------------------

def _missing_batch():
    """Four lookups over n = TILE + 1 rows, the recipe of test_gpu_lookup_permute._missing_cases: lookups
    1 and 3 have a value that is not in the (shared) table, at different rows of their permuted inputs."""
    n = TILE + 1
    s = sorted(_distinct(n, 2000))
    assert s[0] > 5 and s[-1] < R - 5
    inner = s[n // 4: 3 * n // 4]
    gap = next(v + 1 for v in inner[len(inner) // 2:] if v + 1 not in s)   # between two table values

    def base(seed):
        rng = random.Random(seed)
        return [rng.choice(inner) for _ in range(n)]

    def with_values(a, *vals):
        for k, v in enumerate(vals):
            a[(k * 97 + 11) % n] = v
        return a
    lookups = [(base(2001), s), (with_values(base(2002), gap), s), (base(2003), s),
               (with_values(base(2004), s[-1] + 1, s[0] - 1), s)]
    rows = [lp.permute_direct(a, t)[2] for a, t in lookups]
    assert rows[0] is None and rows[2] is None and rows[3] == 0 and 0 < rows[1] < n - 1
    return lookups, rows


def test_missing_values_in_two_lookups_of_four(gpu):
    import ctypes
    import torch
    import svgpu
    from svgpu import _lib, device as dv
    lookups, rows = _missing_batch()
    n = len(lookups[0][0])
    for form in FORMS:
        S = _col(lookups[0][1], form, gpu)
        A = [_col(a, form, gpu) for a, _ in lookups]
        out = [(torch.zeros_like(S), torch.zeros_like(S)) for _ in lookups]
        with pytest.raises(svgpu.ArgumentError, match="not in table") as e:
            dv.lookup_permute_batch_device(A, S, form=form, out=out)
        assert e.value.lookup == 1 and e.value.rows == rows and f"row {rows[1]} " in str(e.value)
        for j in (0, 2):                                                    # the lookups that hold are exact
            _assert_pair(out[j], lookups[j][0], lookups[j][1], form, j)
        # the C ABI's own words: the rows as UINT64_MAX where fine; NULL outputs: the same status
        ptrs = ctypes.c_void_p * 4
        a_p, s_p = ptrs(*[t.data_ptr() for t in A]), ptrs(*[S.data_ptr()] * 4)
        oa, os_ = ptrs(*[p[0].data_ptr() for p in out]), ptrs(*[p[1].data_ptr() for p in out])
        got, failed = (ctypes.c_uint64 * 4)(5, 5, 5, 5), ctypes.c_uint64(5)
        call = _lib.lib.sv_bn254_fr_lookup_permute_batch_device
        assert call(a_p, s_p, 4, n, form, 0, oa, os_, got, ctypes.byref(failed), 0, None) == _lib.SV_ERR_ARG
        assert "not in table" in _lib.last_error()
        assert failed.value == 1 and list(got) == [MAX, rows[1], MAX, rows[3]]
        assert call(a_p, s_p, 4, n, form, 0, oa, os_, None, None, 0, None) == _lib.SV_ERR_ARG
        assert "not in table" in _lib.last_error()
        # the next call on the same pool is exact and says so
        a_p = ptrs(*[A[0].data_ptr(), A[2].data_ptr(), A[0].data_ptr(), A[2].data_ptr()])
        assert call(a_p, s_p, 4, n, form, 0, oa, os_, got, ctypes.byref(failed), 0, None) == _lib.SV_OK
        assert failed.value == MAX and list(got) == [MAX] * 4
        for j in range(4):
            _assert_pair(out[j], lookups[(0, 2)[j % 2]][0], lookups[0][1], form, j)


def test_unreduced_element_wins_and_the_next_call_is_exact(gpu):
    import svgpu
    from svgpu import device as dv
    lookups, rows = _missing_batch()
    good = [lookups[0], lookups[2], lookups[0]]
    for form in FORMS:
        for where in ("input", "shared table"):
            for at in (TILE - 1, TILE):
                for third in (lookups[0][0], lookups[1][0]):                # with and without a miss in another lookup
                    cols = [_limbs(list(lookups[0][0]), form), _limbs(list(lookups[2][0]), form), _limbs(list(third), form)]
                    table = _limbs(list(lookups[0][1]), form)
                    if where == "input":
                        cols[1][at] = _UNREDUCED
                    else:
                        table[at] = _UNREDUCED
                    for flag in (False, True):                              # the table is sorted: both ways of reading it
                        with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                            dv.lookup_permute_batch_device([_dev(c, gpu) for c in cols], _dev(table, gpu), form=form,
                                                           tables_sorted=flag)
            _run_and_check(good, form, gpu)                                 # the next call on the same pool


# ---- 6. the carries scan takes two totals per thread ---------------------------------------------

def test_large_two_lookups_one_table(gpu):
    lookups = [_shared_lookup("full-width", LARGE, 0), _shared_lookup("full-width", LARGE, 4)]
    assert INPUT_SHAPES[0] == INPUT_SHAPES[4 % 4] == "heavy-repeats" and lookups[0][0] != lookups[1][0]
    for form in FORMS:
        _run_and_check(lookups, form, gpu)


# ---- 7. the wrapper ------------------------------------------------------------------------------

def test_wrapper_out_inputs_unchanged_and_refusals(gpu):
    import torch
    import svgpu
    from svgpu import device as dv
    n = TILE + 1
    lookups = [_shared_lookup("full-width", n, 0), _shared_lookup("full-width", n, 1)]
    A = [_col(a, CANONICAL, gpu) for a, _ in lookups]
    S = _col(lookups[0][1], CANONICAL, gpu)
    keep = [t.clone() for t in A + [S]]
    out = [(torch.zeros_like(S), torch.zeros_like(S)) for _ in A]
    got = dv.lookup_permute_batch_device(A, S, form=CANONICAL, out=out)
    assert [(p[0].data_ptr(), p[1].data_ptr()) for p in got] == [(p[0].data_ptr(), p[1].data_ptr()) for p in out]
    for j, (a, s) in enumerate(lookups):
        _assert_pair(out[j], a, s, CANONICAL, j)
    assert all(t.equal(k) for t, k in zip(A + [S], keep))                   # inputs and tables are only read
    # every overlap among the 4 count pointers that is refused: an output on, one element into, and one
    # element in front of an input, a table and each other output
    buf = torch.zeros((6 * n + 4, 4), dtype=torch.int64, device=gpu)
    free = [buf[k * (n + 1):k * (n + 1) + n] for k in range(4)]
    others = A + [S] + free[1:]
    for slot in range(4):
        for other in others:
            bad = [list(p) for p in (free[0:2], free[2:4])]
            if other is bad[slot // 2][slot % 2]:
                continue
            bad[slot // 2][slot % 2] = other
            with pytest.raises(svgpu.ArgumentError, match="overlaps"):
                dv.lookup_permute_batch_device(A, S, form=CANONICAL, out=bad)
    Ab = buf[4 * (n + 1) + 1:4 * (n + 1) + 1 + n]
    Ab.copy_(A[0])
    for near in (buf[4 * (n + 1):4 * (n + 1) + n], buf[4 * (n + 1) + 2:4 * (n + 1) + 2 + n]):
        for slot in range(4):
            bad = [list(p) for p in (free[0:2], free[2:4])]
            bad[slot // 2][slot % 2] = near
            for cols, tab in (([Ab, A[1]], S), ([A[0], A[1]], [S, Ab])):    # near an input, near a table
                with pytest.raises(svgpu.ArgumentError, match="overlaps"):
                    dv.lookup_permute_batch_device(cols, tab, form=CANONICAL, out=bad)
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):                  # an output one element into another output
        dv.lookup_permute_batch_device(A, S, form=CANONICAL, out=[(free[0], buf[1:n + 1]), (free[2], free[3])])
    # counts, shapes, devices
    with pytest.raises(svgpu.EmptyError):
        dv.lookup_permute_batch_device([], [])
    with pytest.raises(svgpu.EmptyError):
        dv.lookup_permute_batch_device([], S)
    with pytest.raises(svgpu.LengthError, match="SV_LOOKUP_BATCH_MAX"):
        dv.lookup_permute_batch_device([A[0]] * 17, S)
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_batch_device(A, [S])
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_batch_device(A, S[:n - 1])
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_batch_device([A[0], A[1][:n - 1]], S)
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_batch_device(A, S, out=[(free[0], free[1])])
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_batch_device(A, S, out=[(free[0], free[1]), (free[2], free[3][:n - 1])])
    with pytest.raises(svgpu.ArgumentError):
        dv.lookup_permute_batch_device(A, torch.zeros((n, 5), dtype=torch.int64, device=gpu))
    with pytest.raises(svgpu.ArgumentError):
        dv.lookup_permute_batch_device([A[0], A[1].to(torch.int32)], S)
    with pytest.raises(svgpu.ArgumentError, match="one device"):
        dv.lookup_permute_batch_device(A, S.cpu())
    with pytest.raises(svgpu.ArgumentError, match="one device"):
        dv.lookup_permute_batch_device([A[0], A[1].cpu()], S)
    with pytest.raises(svgpu.LengthError):
        dv.lookup_permute_batch_device(A, S, out=[(free[0], free[1]), (free[2], free[3].cpu())])
    with pytest.raises(svgpu.ArgumentError, match="bad form"):
        dv.lookup_permute_batch_device(A, S, form=7)


# ---- 8. the lookup arguments of a circuit --------------------------------------------------------

def test_lookup_arguments_against_the_single_calls(gpu):
    import svgpu
    n = TILE + 1
    sa, sb = _table("full-width", n, tag=50), _table("range-table", n, tag=51)
    lookups = [(tuple(_input("heavy-repeats", sa, 11)), sa), (tuple(_input("range-table", sb, 12)), sb),
               (tuple(_input("constant-input", sa, 13)), sa)]
    for form in FORMS:
        TA, TB = _col(sa, form, gpu), _col(sb, form, gpu)
        A, S = [_col(a, form, gpu) for a, _ in lookups], [TA, TB, TA]
        got = svgpu.lookup_arguments(A, S, BETA, GAMMA, z0=Z0, form=form)
        assert len(got) == 3
        for j, (a, s) in enumerate(lookups):
            one = svgpu.lookup_argument(A[j], S[j], BETA, GAMMA, z0=Z0, form=form)
            assert got[j][3] == one[3] == Z0
            for x, y in zip(got[j][:3], one[:3]):
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
            _assert_pair(got[j][:2], a, s, form, j)
            lp.check_relations(list(a), list(s), _decode(got[j][0], form), _decode(got[j][1], form), BETA, GAMMA)
    # one tensor for every lookup, sorted by the caller
    TS = svgpu.sort_device(_col(sa, MONTGOMERY, gpu), form=MONTGOMERY)
    A = [_col(lookups[0][0], MONTGOMERY, gpu), _col(lookups[2][0], MONTGOMERY, gpu)]
    got = svgpu.lookup_arguments(A, TS, BETA, GAMMA, z0=Z0, form=MONTGOMERY, tables_sorted=True)
    for j, k in enumerate((0, 2)):
        _assert_pair(got[j][:2], lookups[k][0], sa, MONTGOMERY, j)
        assert got[j][3] == Z0
