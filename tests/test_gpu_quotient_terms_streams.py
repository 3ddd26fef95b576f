"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for
sv_bn254_fr_permutation_terms_device and sv_bn254_fr_lookup_terms_device, under the pending-producer
harness of tests/stream_cases.py, imported and unchanged: read after write on an input (it is
produced behind a calibrated delay on the caller's stream: a z column, whose halo and far rotation
read other blocks' rows, the accumulator of an in-place call, and a lookup's a'), write after read on
an out-of-place output (an earlier clone still reads it), on a side stream and on the NULL stream,
and the stream has drained when the call returns.  The cases also cover each call's one small table
copy, which must run on the call's stream behind the caller's work like the launch."""
import time

import pytest
import torch

import stream_cases as sc
from test_gpu_extended import ZETA
from test_gpu_kzg_open import _limb_bytes, _limbs
from test_gpu_ntt import CANONICAL, MONTGOMERY
from test_gpu_quotient_terms import (BETA, GAMMA, Y, _fold, _lookup_constraints, _perm_constraints, _pool,
                                     _s_values)

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]
M, CHUNK, LAST = 3, 2, -3


def _perm_io(k, e, g, pending):
    """The columns of one permutation call and its results for the true and the stale `pending` column."""
    K, N = k + e, 1 << (k + e)
    pool = _pool(N)
    cols = dict(cols=list(pool[0:3]), sigmas=list(pool[3:6]), z=list(pool[6:8]), l=list(pool[8:11]), acc=[pool[11]])
    stale = pool[12]
    out = []
    for col in (None, stale):
        c = {key: list(v) for key, v in cols.items()}
        if col is not None:
            c[pending[0]][pending[1]] = col
        cons = _perm_constraints(c["cols"], c["sigmas"], _s_values(M), CHUNK, c["z"], *c["l"], BETA, GAMMA, g, K, 1 << e,
                                 LAST)
        out.append(_fold(cons, Y, c["acc"][0]))
    return cols, stale, out[0], out[1]


def _lookup_io(k, e, pending):
    N = 1 << (k + e)
    pool = _pool(N)
    cols = dict(look=list(pool[20:25]), l=list(pool[8:11]), acc=[pool[11]])
    stale = pool[12]
    out = []
    for col in (None, stale):
        c = {key: list(v) for key, v in cols.items()}
        if col is not None:
            c[pending[0]][pending[1]] = col
        out.append(_fold(_lookup_constraints([tuple(c["look"])], *c["l"], BETA, GAMMA, 1 << e), Y, c["acc"][0]))
    return cols, stale, out[0], out[1]


def _tensors(cols, form, gpu):
    return {key: [sc.dev(_limbs(list(v), form), gpu) for v in vs] for key, vs in cols.items()}


def _perm(k, e, g, pending, in_place=False, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        cols, stale, want, old = _perm_io(k, e, g, pending)
        t = _tensors(cols, form, c.gpu)
        A = t[pending[0]][pending[1]]
        true, stale_t = A.clone(), sc.dev(_limbs(list(stale), form), c.gpu)
        s = _s_values(M)

        def call():
            acc = t["acc"][0]
            return dv.permutation_terms_device(t["cols"], t["sigmas"], s, CHUNK, t["z"], *t["l"], BETA, GAMMA, Y, k, LAST,
                                               shift=g, form=form, acc=acc, out=acc if in_place else None)

        return dict(inputs=[(A, true, stale_t)], call=call, finish=lambda r: r.cpu().numpy().tobytes(),
                    want=_limb_bytes(want, form), stale=_limb_bytes(old, form))
    return build


def _lookup(k, e, pending, in_place=False, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        cols, stale, want, old = _lookup_io(k, e, pending)
        t = _tensors(cols, form, c.gpu)
        A = t[pending[0]][pending[1]]
        true, stale_t = A.clone(), sc.dev(_limbs(list(stale), form), c.gpu)

        def call():
            acc = t["acc"][0]
            return dv.lookup_terms_device([t["look"]], *t["l"], BETA, GAMMA, Y, k, form=form, acc=acc,
                                          out=acc if in_place else None)

        return dict(inputs=[(A, true, stale_t)], call=call, finish=lambda r: r.cpu().numpy().tobytes(),
                    want=_limb_bytes(want, form), stale=_limb_bytes(old, form))
    return build


def _war_perm(k, e, g):
    def build(c):
        from svgpu import device as dv
        cols, _, want, _ = _perm_io(k, e, g, ("z", 0))
        t = _tensors(cols, CANONICAL, c.gpu)
        out = sc._pattern((1 << (k + e), 4), c.gpu)
        return dict(out=out, want=_limb_bytes(want, CANONICAL),
                    call=lambda: dv.permutation_terms_device(t["cols"], t["sigmas"], _s_values(M), CHUNK, t["z"], *t["l"],
                                                             BETA, GAMMA, Y, k, LAST, shift=g, form=CANONICAL,
                                                             acc=t["acc"][0], out=out))
    return build


def _war_lookup(k, e):
    def build(c):
        from svgpu import device as dv
        cols, _, want, _ = _lookup_io(k, e, ("look", 1))
        t = _tensors(cols, CANONICAL, c.gpu)
        out = sc._pattern((1 << (k + e), 4), c.gpu)
        return dict(out=out, want=_limb_bytes(want, CANONICAL),
                    call=lambda: dv.lookup_terms_device([t["look"]], *t["l"], BETA, GAMMA, Y, k, form=CANONICAL,
                                                        acc=t["acc"][0], out=out))
    return build


CASES = [
    sc.Case("permutation_terms-k3-e2-z0-pending", _perm(3, 2, ZETA, ("z", 0))),
    sc.Case("permutation_terms-k9-e2-z0-pending-montgomery", _perm(9, 2, ZETA, ("z", 0), form=MONTGOMERY)),
    sc.Case("permutation_terms-k9-e2-acc-pending-in-place", _perm(9, 2, None, ("acc", 0), in_place=True)),
    sc.Case("lookup_terms-k3-e2-permuted-input-pending", _lookup(3, 2, ("look", 1))),
    sc.Case("lookup_terms-k9-e2-permuted-input-pending-montgomery", _lookup(9, 2, ("look", 1), form=MONTGOMERY)),
    sc.Case("lookup_terms-k9-e2-acc-pending-in-place", _lookup(9, 2, ("acc", 0), in_place=True)),
]
WARS = [
    sc.War("permutation_terms-out-k3-e2", _war_perm(3, 2, ZETA)),
    sc.War("permutation_terms-out-k9-e2", _war_perm(9, 2, ZETA)),
    sc.War("lookup_terms-out-k3-e2", _war_lookup(3, 2)),
    sc.War("lookup_terms-out-k9-e2", _war_lookup(9, 2)),
]


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
            with sc.environ(getattr(case, "env", {})):
                for _ in range(2):           # the first call grows the pool; the second is the warm one
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
def test_terms_calls_are_ordered_after_the_callers_stream(ctx, case, mode):
    """Read after write on the input; synchronous: the stream has drained on return (run_ordering
    asserts both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_terms_outputs_written_after_earlier_readers(ctx, case, mode):
    """Write after read on an out-of-place output."""
    sc.run_war(ctx, case, mode)
