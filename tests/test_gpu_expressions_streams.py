"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for
sv_bn254_fr_expressions_device, under the pending-producer harness of tests/stream_cases.py, imported
and unchanged: read after write on an input (it is produced behind a calibrated delay on the caller's
stream: a column whose rotated rows other blocks read, and the accumulator of an in-place call), write
after read on an out-of-place output and on a store (an earlier clone still reads it), on a side
stream and on the NULL stream, and the stream has drained when the call returns.  The cases also
cover the call's one small table copy, which must run on the call's stream behind the caller's work
like the launch."""
import time

import pytest
import torch

import expr_cases as ec
import stream_cases as sc
from test_gpu_kzg_open import _limb_bytes, _limbs
from test_gpu_ntt import CANONICAL, MONTGOMERY
from test_gpu_quotient_terms import Y, _pool

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]
N_COLS = 4
SINKS = [("fold", ("mul", ("col", 0, 1), ("sub", ("col", 1, -1), ("col", 2, 0)))),
         ("store", 0, ("add", ("col", 0, -3), ("scaled", ("col", 3, 2), 5))),
         ("fold", ("neg", ("col", 0, 0)))]


def _io(k, e, pending):
    """The columns of one call and its results for the true and the stale `pending` column."""
    N = 1 << (k + e)
    pool = _pool(N)
    cols = dict(cols=list(pool[0:N_COLS]), acc=[pool[11]])
    stale = pool[12]
    out = []
    for col in (None, stale):
        c = {key: list(v) for key, v in cols.items()}
        if col is not None:
            c[pending[0]][pending[1]] = col
        out.append(ec.program_rows(SINKS, c["cols"], 1 << e, Y, c["acc"][0]))
    return cols, stale, out[0], out[1]


def _tensors(cols, form, gpu):
    return {key: [sc.dev(_limbs(list(v), form), gpu) for v in vs] for key, vs in cols.items()}


def _program():
    import svgpu
    ops, consts, _ = svgpu.compile_expressions(SINKS)
    return ops, consts


def _both(out, store):
    """The fold's output and the store as one byte string."""
    return out.cpu().numpy().tobytes() + store.cpu().numpy().tobytes()


def _case(k, e, pending, in_place=False, form=CANONICAL):
    def build(c):
        import svgpu
        cols, stale, want, old = _io(k, e, pending)
        t = _tensors(cols, form, c.gpu)
        A = t[pending[0]][pending[1]]
        true, stale_t = A.clone(), sc.dev(_limbs(list(stale), form), c.gpu)
        ops, consts = _program()

        def call():
            acc = t["acc"][0]
            return svgpu.expressions_device(ops, t["cols"], consts, stores=1, y=Y, acc=acc, out=acc if in_place else None,
                                            log_n=k, form=form)

        return dict(inputs=[(A, true, stale_t)], call=call, finish=lambda r: _both(r[0], r[1][0]),
                    want=_limb_bytes(want[0], form) + _limb_bytes(want[1][0], form),
                    stale=_limb_bytes(old[0], form) + _limb_bytes(old[1][0], form))
    return build


def _war(k, e, which):
    """Write after read on d_out (which = "out") or on the store."""
    def build(c):
        import svgpu
        cols, _, want, _ = _io(k, e, ("cols", 0))
        t = _tensors(cols, CANONICAL, c.gpu)
        target = sc._pattern((1 << (k + e), 4), c.gpu)
        ops, consts = _program()
        kw = dict(out=target, stores=1) if which == "out" else dict(stores=[target])

        def call():
            return svgpu.expressions_device(ops, t["cols"], consts, y=Y, acc=t["acc"][0], log_n=k, form=CANONICAL, **kw)

        return dict(out=target, want=_limb_bytes(want[0] if which == "out" else want[1][0], CANONICAL), call=call)
    return build


CASES = [
    sc.Case("expressions-k3-e2-column-pending", _case(3, 2, ("cols", 0))),
    sc.Case("expressions-k9-e2-column-pending-montgomery", _case(9, 2, ("cols", 0), form=MONTGOMERY)),
    sc.Case("expressions-k9-e2-acc-pending-in-place", _case(9, 2, ("acc", 0), in_place=True)),
]
WARS = [
    sc.War("expressions-out-k3-e2", _war(3, 2, "out")),
    sc.War("expressions-out-k9-e2", _war(9, 2, "out")),
    sc.War("expressions-store-k9-e2", _war(9, 2, "store")),
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
def test_expressions_call_is_ordered_after_the_callers_stream(ctx, case, mode):
    """Read after write on the input; synchronous: the stream has drained on return (run_ordering
    asserts both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_expressions_outputs_written_after_earlier_readers(ctx, case, mode):
    """Write after read on an out-of-place output and on a store."""
    sc.run_war(ctx, case, mode)
