"""The Fr sort on the device (sv_bn254_fr_sort_device; csrc/lookup_permute.hip) against sorted() on
Python ints, bit for bit, in both forms.  Nothing expected comes from the code under test.

Sizes.  W = 64 lanes per wave, TILE = kLpTile keys per block, T = kLpThreads (read from
csrc/lookup_permute.hpp): n in {1, 2, 3, W - 1, W, W + 1, TILE - 1, TILE, TILE + 1, 2 TILE + 1,
3 TILE - 1} covers part of a wave's run, a run, a block, and two and three blocks with a one-key and
an all-but-one-key tail; n = T TILE + 1 is the first size at which k_lp_offsets (and the
permutation's k_lp_carries) take two entries per thread, and at which a block of k_lp_first strides
to a second tile.

Key families (tests/lookup_permute_cases.py).  full-width keys: 32 live passes; all keys equal: no
live pass, the checked copy; keys that differ in one digit (0, a middle one, 31): one live pass, an
odd parity; keys that differ in two non-adjacent digits with three values each: two live passes, an
even parity, sorted only if the second pass is stable; three values; sorted and reverse sorted.
Every family also runs with 0, 1 and r - 1 planted at the first, the middle and the last row
(n >= 3), which adds live digits to the families that count them, so those run both ways.
tests/COVERAGE_lookup_permute.md has the ledger."""
import os
import re

import pytest

import lookup_permute_cases as lp
from conftest import PKG
from test_gpu_kzg_open import _dev, _limb_bytes, _limbs
from test_gpu_resident_bases import _UNREDUCED

pytestmark = pytest.mark.gpu

_HPP = open(os.path.join(PKG, "csrc", "lookup_permute.hpp")).read()
TILE = int(re.search(r"constexpr uint32_t kLpTile = (\d+);", _HPP).group(1))
T = int(re.search(r"constexpr uint32_t kLpThreads = (\d+);", _HPP).group(1))
W = 64
R = lp.R
CANONICAL, MONTGOMERY = 0, 1
FORMS = (CANONICAL, MONTGOMERY)
SIZES = sorted({1, 2, 3, W - 1, W, W + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE - 1})
LARGE = T * TILE + 1
assert LARGE <= 1 << 19, "the ledger lists a larger size as not launched"

FAMILIES = {
    "full-width": lambda n: lp.full_width(n, 100 + n),
    "all-equal": lambda n: [lp.BASE] * n,
    "digit-0": lambda n: lp.one_digit(n, 0, 200 + n),
    "digit-13": lambda n: lp.one_digit(n, 13, 300 + n),
    "digit-31": lambda n: lp.one_digit(n, 31, 400 + n),
    "digits-0-and-2": lambda n: lp.two_digits(n, 0, 2, 500 + n),
    "digits-7-and-31": lambda n: lp.two_digits(n, 7, 31, 600 + n),
    "three-values": lambda n: lp.few_values(n, 700 + n),
    "sorted": lambda n: sorted(lp.full_width(n, 800 + n)),
    "reverse-sorted": lambda n: sorted(lp.full_width(n, 900 + n), reverse=True),
}


def _sort(keys, form, gpu, **kw):
    from svgpu import device as dv
    return dv.sort_device(_dev(_limbs(keys, form), gpu), form=form, **kw)


def _check(keys, form, gpu):
    got = _sort(keys, form, gpu).cpu().numpy().tobytes()
    assert got == _limb_bytes(sorted(keys), form), (len(keys), form)


@pytest.mark.parametrize("planted", [False, True], ids=["plain", "planted"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_sort_matches_sorted_ints(gpu, family, planted):
    for n in SIZES:
        if planted and n < 3:
            continue
        keys = FAMILIES[family](n)
        if planted:
            keys = lp.plant(list(keys))
        for form in FORMS:
            _check(keys, form, gpu)


@pytest.mark.parametrize("family", ["full-width", "digits-7-and-31"])
def test_offsets_scan_takes_two_entries_per_thread(gpu, family):
    """n = T TILE + 1: 257 blocks, so a thread of k_lp_offsets sums and rewrites two counts."""
    keys = lp.plant(FAMILIES[family](LARGE))
    want = sorted(keys)
    for form in FORMS:
        assert _sort(keys, form, gpu).cpu().numpy().tobytes() == _limb_bytes(want, form)


def test_in_place_and_out_of_place(gpu):
    import torch
    from svgpu import device as dv
    n = 2 * TILE + 1
    keys = lp.plant(lp.full_width(n, 31))
    for form in FORMS:
        want = _limb_bytes(sorted(keys), form)
        src = _dev(_limbs(keys, form), gpu)
        keep = src.clone()
        out = torch.zeros_like(src)
        res = dv.sort_device(src, form=form, out=out)
        assert res.data_ptr() == out.data_ptr() and out.cpu().numpy().tobytes() == want
        assert src.equal(keep)                                   # the input is only read
        res = dv.sort_device(src, form=form, out=src)
        assert res.data_ptr() == src.data_ptr() and src.cpu().numpy().tobytes() == want


def test_unreduced_element_is_found_and_the_next_call_is_exact(gpu):
    import svgpu
    from svgpu import device as dv
    n = 2 * TILE + 1
    keys = lp.plant(lp.full_width(n, 32))
    for form in FORMS:
        good = _limbs(keys, form)
        for at in (TILE - 1, TILE):
            bad = good.copy()
            bad[at] = _UNREDUCED
            with pytest.raises(svgpu.ArgumentError, match="not reduced"):
                dv.sort_device(_dev(bad, gpu), form=form)
            assert dv.sort_device(_dev(good, gpu), form=form).cpu().numpy().tobytes() == _limb_bytes(sorted(keys), form)


def test_wrapper_refusals(gpu):
    import torch
    import svgpu
    from svgpu import device as dv
    buf = torch.zeros((12, 4), dtype=torch.int64, device=gpu)
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        dv.sort_device(buf[0:8], out=buf[1:9])
    with pytest.raises(svgpu.ArgumentError, match="overlaps"):
        dv.sort_device(buf[1:9], out=buf[0:8])
    with pytest.raises(svgpu.LengthError):
        dv.sort_device(buf[0:8], out=buf[0:4])
    with pytest.raises(svgpu.ArgumentError):
        dv.sort_device(torch.zeros((4, 5), dtype=torch.int64, device=gpu))
    assert svgpu.sort_device(buf[0:3], form=CANONICAL).equal(buf[0:3])
