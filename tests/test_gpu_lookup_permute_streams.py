"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for
sv_bn254_fr_sort_device and sv_bn254_fr_lookup_permute_device, under the pending-producer harness of
tests/stream_cases.py, imported and unchanged: read after write on an input column (the column is
produced behind a calibrated delay on the caller's stream), write after read on each output (an
earlier clone still reads it), at n = 3 and n = TILE + 1, on a side stream and on the NULL stream,
and the stream has drained when the call returns.  The harness wants a context with the cases built
and a delay sized from their warm times; the one below holds only these cases.  Expected values are
sorted() and the direct restatement (tests/lookup_permute_cases.py)."""
import random
import time

import pytest
import torch

import lookup_permute_cases as lp
import stream_cases as sc
from test_gpu_fr_sort import CANONICAL, MONTGOMERY, TILE
from test_gpu_kzg_open import _limb_bytes, _limbs

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]
SIZES = [3, TILE + 1]


def _keys(n, tag):
    """Generated keys; 0, 1 and r - 1 planted from 8 rows on (three planted rows would be all of n = 3,
    and the true and the stale column of a case must differ)."""
    keys = lp.full_width(n, 5000 + tag)
    return lp.plant(keys) if n >= 8 else keys


def _pair(n, tag):
    """(a, s) of a lookup that holds, with repeats."""
    rng = random.Random(5100 + tag)
    s = _keys(n, tag)
    return [rng.choice(s[:max(1, n // 2)]) for _ in range(n)], s


def _sort(n, in_place=False, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        true, stale = _keys(n, 1), _keys(n, 2)
        A = sc.dev(_limbs(stale, form), c.gpu)
        return dict(inputs=[(A, sc.dev(_limbs(true, form), c.gpu), sc.dev(_limbs(stale, form), c.gpu))],
                    call=lambda: dv.sort_device(A, form=form, out=A if in_place else None),
                    finish=lambda r: r.cpu().numpy().tobytes(), want=_limb_bytes(sorted(true), form),
                    stale=_limb_bytes(sorted(stale), form))
    return build


def _expected(a, s, form):
    ap, sp, row = lp.permute_direct(a, s)
    assert row is None
    return _limb_bytes(ap, form), _limb_bytes(sp, form)


def _permute(n, which, form=CANONICAL):
    """The column `which` (0: the input, 1: the table) is the one produced behind the delay; its
    stale content is another lookup's column that holds against the other one too."""
    def build(c):
        from svgpu import device as dv
        a, s = _pair(n, 3)
        if which == 0:
            a2, s2 = [random.Random(5200).choice(s) for _ in range(n)], s
        else:
            a2, s2 = a, list(s[:max(1, n // 2)]) + _keys(n, 4)[max(1, n // 2):]
        cols = [sc.dev(_limbs(a, form), c.gpu), sc.dev(_limbs(s, form), c.gpu)]
        true, stale = (a, s)[which], (a2, s2)[which]
        return dict(inputs=[(cols[which], sc.dev(_limbs(true, form), c.gpu), sc.dev(_limbs(stale, form), c.gpu))],
                    call=lambda: dv.lookup_permute_device(cols[0], cols[1], form=form),
                    finish=lambda r: (r[0].cpu().numpy().tobytes(), r[1].cpu().numpy().tobytes()),
                    want=_expected(a, s, form), stale=_expected(a2, s2, form))
    return build


def _war_sort(n):
    def build(c):
        from svgpu import device as dv
        a = _keys(n, 1)
        A, out = sc.dev(_limbs(a, CANONICAL), c.gpu), sc._pattern((n, 4), c.gpu)
        return dict(out=out, call=lambda: dv.sort_device(A, form=CANONICAL, out=out), want=_limb_bytes(sorted(a), CANONICAL))
    return build


def _war_permute(n, which):
    def build(c):
        from svgpu import device as dv
        a, s = _pair(n, 3)
        A, S = sc.dev(_limbs(a, CANONICAL), c.gpu), sc.dev(_limbs(s, CANONICAL), c.gpu)
        out, other = sc._pattern((n, 4), c.gpu), torch.empty((n, 4), dtype=torch.int64, device=c.gpu)
        pair = (out, other) if which == 0 else (other, out)
        return dict(out=out, call=lambda: dv.lookup_permute_device(A, S, form=CANONICAL, out=pair),
                    want=_expected(a, s, CANONICAL)[which])
    return build


CASES = [sc.Case(f"sort_device-n{n}", _sort(n)) for n in SIZES]
CASES += [sc.Case(f"sort_device-n{TILE + 1}-in-place-montgomery", _sort(TILE + 1, in_place=True, form=MONTGOMERY))]
CASES += [sc.Case(f"lookup_permute_device-input-n{n}", _permute(n, 0)) for n in SIZES]
CASES += [sc.Case(f"lookup_permute_device-table-n{n}", _permute(n, 1)) for n in SIZES]
CASES += [sc.Case(f"lookup_permute_device-table-n{TILE + 1}-montgomery", _permute(TILE + 1, 1, MONTGOMERY))]
WARS = [sc.War(f"sort_device-out-n{n}", _war_sort(n)) for n in SIZES]
WARS += [sc.War(f"lookup_permute_device-permuted-input-n{n}", _war_permute(n, 0)) for n in SIZES]
WARS += [sc.War(f"lookup_permute_device-permuted-table-n{n}", _war_permute(n, 1)) for n in SIZES]


class _Context:
    """What run_ordering and run_war read of stream_cases.Context: the device, every case built once,
    and the delay sized from the cases' warm wall times."""

    def __init__(self, gpu):
        self.gpu = gpu
        self.built = {}
        self.delay = sc.Delay()
        warm = {}
        for case in CASES + WARS:
            st = self.built[case.name] = case.build(self)
            torch.cuda.synchronize()
            for _ in range(2):               # the first call grows the pool; the second is the warm one
                t0 = time.perf_counter()
                st["call"]()
                torch.cuda.synchronize()
                warm[case.name] = (time.perf_counter() - t0) * 1e3
        self.delay.size(warm)


@pytest.fixture(scope="module")
def ctx(gpu, oracle_cpp):
    c = _Context(gpu)
    yield c
    torch.cuda.synchronize()
    c.built.clear()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_calls_are_ordered_after_the_callers_stream(ctx, case, mode):
    """Read after write on an input column; synchronous: the stream has drained on return
    (run_ordering asserts both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_outputs_written_after_earlier_readers(ctx, case, mode):
    """Write after read on the sort's out-of-place d_out and on each of the permutation's outputs."""
    sc.run_war(ctx, case, mode)
