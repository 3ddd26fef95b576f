"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for
sv_bn254_fr_lookup_permute_batch_device, under the pending-producer harness of tests/stream_cases.py,
imported and unchanged, in the manner of test_gpu_lookup_permute_streams.py: read after write on an
input column of the second lookup and on the shared table (the column is produced behind a calibrated
delay on the caller's stream), with the table sorted by the call and by the caller; write after read
on an output of either kind (an earlier clone still reads it); at n = 3 and n = TILE + 1, on a side
stream and on the NULL stream; and the stream has drained when the call returns.  Expected values are
the direct restatement (tests/lookup_permute_cases.py), per lookup."""
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


def _table(n, tag, ascending):
    keys = lp.full_width(n, 6000 + tag)
    keys = lp.plant(keys) if n >= 8 else keys
    return sorted(keys) if ascending else keys


def _inputs(n, s, tag):
    rng = random.Random(6100 + tag)
    return [rng.choice(s[:max(1, n // 2)]) for _ in range(n)]


def _expected(lookups, form):
    out = []
    for a, s in lookups:
        ap, sp, row = lp.permute_direct(a, s)
        assert row is None
        out += [_limb_bytes(ap, form), _limb_bytes(sp, form)]
    return tuple(out)


def _finish(r):
    return tuple(t.cpu().numpy().tobytes() for pair in r for t in pair)


def _batch(n, which, form=CANONICAL, tables_sorted=False):
    """Two lookups that share a table.  `which` = 0: the second lookup's input is the column produced
    behind the delay; 1: the table is.  The stale content is another column that holds as well."""
    def build(c):
        from svgpu import device as dv
        s = _table(n, 1, tables_sorted)
        a0, a1 = _inputs(n, s, 1), _inputs(n, s, 2)
        if which == 0:
            true, stale = a1, [s[(i + 1) % n] for i in range(n)]   # every value of the table once: no repeats
            want, old = [(a0, s), (true, s)], [(a0, s), (stale, s)]
        else:
            half = max(1, n // 2)
            s2 = list(s[:half]) + _table(n, 4, False)[half:]   # the inputs come from s[:half]: both tables hold them
            if tables_sorted:                                  # a stale table must be ascending too
                s2 = sorted(s2)
            true, stale = s, s2
            want, old = [(a0, s), (a1, s)], [(a0, s2), (a1, s2)]
        A0, A1, S = sc.dev(_limbs(a0, form), c.gpu), sc.dev(_limbs(a1, form), c.gpu), sc.dev(_limbs(s, form), c.gpu)
        col = A1 if which == 0 else S
        return dict(inputs=[(col, sc.dev(_limbs(true, form), c.gpu), sc.dev(_limbs(stale, form), c.gpu))],
                    call=lambda: dv.lookup_permute_batch_device([A0, A1], S, form=form, tables_sorted=tables_sorted),
                    finish=_finish, want=_expected(want, form), stale=_expected(old, form))
    return build


def _war(n, lookup, which):
    def build(c):
        from svgpu import device as dv
        s = _table(n, 1, False)
        a0, a1 = _inputs(n, s, 1), _inputs(n, s, 2)
        A0, A1, S = sc.dev(_limbs(a0, CANONICAL), c.gpu), sc.dev(_limbs(a1, CANONICAL), c.gpu), sc.dev(_limbs(s, CANONICAL), c.gpu)
        out = sc._pattern((n, 4), c.gpu)
        pairs = [[torch.empty((n, 4), dtype=torch.int64, device=c.gpu) for _ in range(2)] for _ in range(2)]
        pairs[lookup][which] = out
        return dict(out=out, call=lambda: dv.lookup_permute_batch_device([A0, A1], S, form=CANONICAL, out=pairs),
                    want=_expected([(a0, s), (a1, s)], CANONICAL)[2 * lookup + which])
    return build


CASES = [sc.Case(f"lookup_permute_batch-input-n{n}", _batch(n, 0)) for n in SIZES]
CASES += [sc.Case(f"lookup_permute_batch-table-n{n}", _batch(n, 1)) for n in SIZES]
CASES += [sc.Case(f"lookup_permute_batch-sorted-table-n{n}", _batch(n, 1, tables_sorted=True)) for n in SIZES]
CASES += [sc.Case(f"lookup_permute_batch-table-n{TILE + 1}-montgomery", _batch(TILE + 1, 1, MONTGOMERY))]
WARS = [sc.War(f"lookup_permute_batch-permuted-input-1-n{n}", _war(n, 1, 0)) for n in SIZES]
WARS += [sc.War(f"lookup_permute_batch-permuted-table-0-n{n}", _war(n, 0, 1)) for n in SIZES]


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
    """Read after write on an input column and on the shared table; synchronous: the stream has drained
    on return (run_ordering asserts both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_outputs_written_after_earlier_readers(ctx, case, mode):
    """Write after read on a permuted input and on a permuted table of the batch."""
    sc.run_war(ctx, case, mode)
