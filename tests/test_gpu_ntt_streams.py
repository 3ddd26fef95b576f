"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for sv_bn254_fr_ntt_device,
under the pending-producer harness of tests/stream_cases.py, imported and unchanged: read after
write on d_in (the input is produced behind a calibrated delay on the caller's stream), write after
read on an out-of-place d_out (an earlier clone still reads it), on a side stream and on the NULL
stream, and the stream has drained when the call returns.  The harness wants a context with the
cases built and a delay sized from their warm times; the one below holds only the NTT's cases."""
import time

import pytest
import torch

import stream_cases as sc
from test_gpu_ntt import CANONICAL, G_GEN, MONTGOMERY, T, _forward, _gen
from test_gpu_kzg_open import _limb_bytes, _limbs

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]


def _inputs(k, count=1):
    """Two different inputs of count 2^k elements: the true one and the stale one."""
    n = count << k
    flat = _gen(2 * n)
    return list(flat[:n]), list(flat[n:])


def _expected(a, k, count, g, inverse, form):
    """Bytes the call must leave for the input a.  The inverse cases are fed forward(x) and must
    return x, so the expected value is never the code's own."""
    n = 1 << k
    return _limb_bytes(a if inverse else [v for t in range(count) for v in _forward(a[t * n:(t + 1) * n], k, g)], form)


def _fed(a, k, count, g, inverse):
    n = 1 << k
    return [v for t in range(count) for v in _forward(a[t * n:(t + 1) * n], k, g)] if inverse else a


def _ntt(k, count=1, g=1, inverse=False, in_place=False, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        true, stale = _inputs(k, count)
        shape = (count, 1 << k, 4) if count > 1 else (1 << k, 4)
        rows = {key: sc.dev(_limbs(_fed(a, k, count, g, inverse), form), c.gpu).reshape(shape)
                for key, a in (("true", true), ("stale", stale))}
        A = rows["stale"].clone()
        return dict(inputs=[(A, rows["true"], rows["stale"])],
                    call=lambda: dv.ntt_device(A, inverse=inverse, shift=g, form=form, out=A if in_place else None),
                    finish=lambda r: r.cpu().numpy().tobytes(),
                    want=_expected(true, k, count, g, inverse, form), stale=_expected(stale, k, count, g, inverse, form))
    return build


def _war(k, g=1, inverse=False):
    def build(c):
        from svgpu import device as dv
        a, _ = _inputs(k)
        A = sc.dev(_limbs(_fed(a, k, 1, g, inverse), CANONICAL), c.gpu)
        out = sc._pattern((1 << k, 4), c.gpu)
        return dict(out=out, call=lambda: dv.ntt_device(A, inverse=inverse, shift=g, form=CANONICAL, out=out),
                    want=_expected(a, k, 1, g, inverse, CANONICAL))
    return build


CASES = [
    sc.Case("ntt_device-k3-one-pass", _ntt(3)),
    sc.Case(f"ntt_device-k{T + 1}-two-passes", _ntt(T + 1)),
    sc.Case(f"ntt_device-k{T + 1}-inverse-coset-in-place", _ntt(T + 1, g=G_GEN, inverse=True, in_place=True, form=MONTGOMERY)),
    sc.Case(f"ntt_device-k{T - 1}-batch-3-in-place", _ntt(T - 1, count=3, g=G_GEN, in_place=True)),
    sc.Case("ntt_device-k7-four-passes", _ntt(7), env={"SVGPU_NTT_TILE_LOG": "2"}),
]
WARS = [
    sc.War("ntt_device-out-k3", _war(3)),
    sc.War(f"ntt_device-out-k{T + 1}", _war(T + 1)),
    sc.War(f"ntt_device-out-k{T + 1}-inverse-coset", _war(T + 1, g=G_GEN, inverse=True)),
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
def test_ntt_is_ordered_after_the_callers_stream(ctx, case, mode):
    """Read after write on d_in; synchronous: the stream has drained on return (run_ordering asserts
    both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_ntt_output_written_after_earlier_readers(ctx, case, mode):
    """Write after read on an out-of-place d_out."""
    sc.run_war(ctx, case, mode)
