"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for
sv_bn254_fr_grand_product_device and sv_bn254_fr_batch_invert_device, under the pending-producer
harness of tests/stream_cases.py, imported and unchanged: read after write on a column (one of the
call's columns is produced behind a calibrated delay on the caller's stream), write after read on
d_z / an out-of-place d_out (an earlier clone still reads it), at n = 3 and n = S + 1, on a side
stream and on the NULL stream, and the stream has drained when the call returns.  The harness wants
a context with the cases built and a delay sized from their warm times; the one below holds only
these cases.  Expected values are Python-int arithmetic (test_gpu_grand_product.Case)."""
import time

import pytest
import torch

import stream_cases as sc
from test_gpu_grand_product import CANONICAL, COLUMN, MONTGOMERY, R, S, Z0_GEN, _case, _column
from test_gpu_kzg_open import _limb_bytes, _limbs

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]
SIZES = [3, S + 1]


def _factors(case, cols):
    from svgpu import device as dv
    return ([dv.Factor(kind, cols[x], cols[y] if kind == COLUMN else None, s, c) for kind, x, y, s, c in case.num],
            [dv.Factor(kind, cols[x], cols[y] if kind == COLUMN else None, s, c) for kind, x, y, s, c in case.den])


def _product(shape, n, name, form=CANONICAL):
    """The column `name` is the one produced behind the delay; its stale content is another column."""
    def build(c):
        from svgpu import device as dv
        true = _case(shape, n)
        stale = true.with_column(name, _column(n, 20))
        cols = {k: sc.dev(_limbs(list(v), form), c.gpu) for k, v in true.cols.items()}
        A = cols[name]
        num, den = _factors(true, cols)

        def exp(case):
            z, total = case.expected(Z0_GEN)
            return total, _limb_bytes(z, form)
        return dict(inputs=[(A, sc.dev(_limbs(list(true.cols[name]), form), c.gpu),
                             sc.dev(_limbs(list(stale.cols[name]), form), c.gpu))],
                    call=lambda: dv.grand_product_device(num, den, z0=Z0_GEN, omega=true.omega, form=form),
                    finish=lambda r: (r[1], r[0].cpu().numpy().tobytes()), want=exp(true), stale=exp(stale))
    return build


def _inverses(a, form):
    return _limb_bytes([pow(x, -1, R) if x else 0 for x in a], form)


def _invert(n, in_place=False, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        true, stale = list(_column(n, 21)), list(_column(n, 22))
        A = sc.dev(_limbs(stale, form), c.gpu)
        return dict(inputs=[(A, sc.dev(_limbs(true, form), c.gpu), sc.dev(_limbs(stale, form), c.gpu))],
                    call=lambda: dv.batch_invert_device(A, form=form, out=A if in_place else None),
                    finish=lambda r: r.cpu().numpy().tobytes(), want=_inverses(true, form), stale=_inverses(stale, form))
    return build


def _war_product(shape, n):
    def build(c):
        from svgpu import device as dv
        case = _case(shape, n)
        cols = {k: sc.dev(_limbs(list(v), CANONICAL), c.gpu) for k, v in case.cols.items()}
        num, den = _factors(case, cols)
        out = sc._pattern((n, 4), c.gpu)
        return dict(out=out, call=lambda: dv.grand_product_device(num, den, z0=Z0_GEN, omega=case.omega, form=CANONICAL,
                                                                  out=out),
                    want=_limb_bytes(case.expected(Z0_GEN)[0], CANONICAL))
    return build


def _war_invert(n):
    def build(c):
        from svgpu import device as dv
        a = list(_column(n, 21))
        A, out = sc.dev(_limbs(a, CANONICAL), c.gpu), sc._pattern((n, 4), c.gpu)
        return dict(out=out, call=lambda: dv.batch_invert_device(A, form=CANONICAL, out=out), want=_inverses(a, CANONICAL))
    return build


CASES = [sc.Case(f"grand_product_device-lookup-n{n}", _product("lookup", n, "sp")) for n in SIZES]
CASES += [sc.Case(f"grand_product_device-perm3-n{n}-montgomery", _product("perm3", n, "sigma1", MONTGOMERY)) for n in SIZES]
CASES += [sc.Case(f"batch_invert_device-n{n}", _invert(n)) for n in SIZES]
CASES += [sc.Case(f"batch_invert_device-n{S + 1}-in-place-montgomery", _invert(S + 1, in_place=True, form=MONTGOMERY))]
WARS = [sc.War(f"grand_product_device-out-lookup-n{n}", _war_product("lookup", n)) for n in SIZES]
WARS += [sc.War(f"batch_invert_device-out-n{n}", _war_invert(n)) for n in SIZES]


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
    """Read after write on a column; synchronous: the stream has drained on return (run_ordering
    asserts both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_outputs_written_after_earlier_readers(ctx, case, mode):
    """Write after read on d_z and on an out-of-place d_out."""
    sc.run_war(ctx, case, mode)
