"""The caller-stream contract (include/svgpu.h, "Streams", points 1 and 2) for
sv_bn254_fr_coset_lde_device and sv_bn254_fr_quotient_coeffs_device, under the pending-producer
harness of tests/stream_cases.py, imported and unchanged: read after write on the input (it is
produced behind a calibrated delay on the caller's stream), write after read on an out-of-place
output (an earlier clone still reads it), on a side stream and on the NULL stream, and the stream
has drained when the call returns.  The quotient's cases also cover its one small table copy, which
must run on the call's stream behind the caller's work like the launches."""
import time

import pytest
import torch

import stream_cases as sc
from test_gpu_extended import ZETA, _lde_pair, _quot_pair
from test_gpu_kzg_open import _limb_bytes, _limbs
from test_gpu_ntt import CANONICAL, G_GEN, MONTGOMERY, T

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]


def _lde_io(k, e, g, count):
    """(coefficients, evaluations) of the true and of the stale input: `count` polynomials each."""
    out = []
    for base in (0, 1000):
        pairs = [_lde_pair(k, e, g, base + 50 * t) for t in range(count)]
        out.append(([v for a, _ in pairs for v in a], [v for _, A in pairs for v in A]))
    return out


def _lde(k, e, g=None, count=1, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        (true, want), (stale, old) = _lde_io(k, e, g, count)
        shape = (count, 1 << k, 4) if count > 1 else (1 << k, 4)
        rows = {key: sc.dev(_limbs(a, form), c.gpu).reshape(shape) for key, a in (("true", true), ("stale", stale))}
        A = rows["stale"].clone()
        return dict(inputs=[(A, rows["true"], rows["stale"])],
                    call=lambda: dv.coset_lde_device(A, e, shift=g, form=form),
                    finish=lambda r: r.cpu().numpy().tobytes(),
                    want=_limb_bytes(want, form), stale=_limb_bytes(old, form))
    return build


def _quot(k, e, pieces, g, in_place=False, form=CANONICAL):
    def build(c):
        from svgpu import device as dv
        keep = pieces << k
        (true, want), (stale, old) = _quot_pair(k, e, g), _quot_pair(k, e, g, 1000)
        rows = {key: sc.dev(_limbs(list(a), form), c.gpu) for key, a in (("true", true), ("stale", stale))}
        A = rows["stale"].clone()
        return dict(inputs=[(A, rows["true"], rows["stale"])],
                    call=lambda: dv.quotient_coeffs_device(A, k, pieces, g, form=form, out=A if in_place else None),
                    finish=lambda r: r.cpu().numpy().tobytes(),
                    want=_limb_bytes(list(want[:keep]), form), stale=_limb_bytes(list(old[:keep]), form))
    return build


def _war_lde(k, e, g=None):
    def build(c):
        from svgpu import device as dv
        a, A = _lde_pair(k, e, g)
        src = sc.dev(_limbs(list(a), CANONICAL), c.gpu)
        out = sc._pattern((1 << (k + e), 4), c.gpu)
        return dict(out=out, call=lambda: dv.coset_lde_device(src, e, shift=g, form=CANONICAL, out=out),
                    want=_limb_bytes(list(A), CANONICAL))
    return build


def _war_quot(k, e, pieces, g):
    def build(c):
        from svgpu import device as dv
        numer, h = _quot_pair(k, e, g)
        src = sc.dev(_limbs(list(numer), CANONICAL), c.gpu)
        out = sc._pattern((pieces << k, 4), c.gpu)
        return dict(out=out, call=lambda: dv.quotient_coeffs_device(src, k, pieces, g, form=CANONICAL, out=out),
                    want=_limb_bytes(list(h[:pieces << k]), CANONICAL))
    return build


CASES = [
    sc.Case("coset_lde-k3-e2-one-pass", _lde(3, 2, ZETA)),
    sc.Case(f"coset_lde-k{T - 1}-e2-two-passes", _lde(T - 1, 2, G_GEN, form=MONTGOMERY)),
    sc.Case(f"coset_lde-k{T - 2}-e2-batch-3-no-shift", _lde(T - 2, 2, None, count=3)),
    sc.Case("coset_lde-k4-e3-four-passes", _lde(4, 3, ZETA), env={"SVGPU_NTT_TILE_LOG": "2"}),
    sc.Case("quotient_coeffs-k3-e2-one-pass", _quot(3, 2, 3, ZETA)),
    sc.Case(f"quotient_coeffs-k{T - 1}-e2-two-passes-in-place", _quot(T - 1, 2, 3, G_GEN, in_place=True, form=MONTGOMERY)),
    sc.Case("quotient_coeffs-k4-e3-four-passes", _quot(4, 3, 5, ZETA), env={"SVGPU_NTT_TILE_LOG": "2"}),
]
WARS = [
    sc.War("coset_lde-out-k3-e2", _war_lde(3, 2, ZETA)),
    sc.War(f"coset_lde-out-k{T - 1}-e2", _war_lde(T - 1, 2, G_GEN)),
    sc.War("quotient_coeffs-out-k3-e2", _war_quot(3, 2, 3, ZETA)),
    sc.War(f"quotient_coeffs-out-k{T - 1}-e2", _war_quot(T - 1, 2, 3, G_GEN)),
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
def test_extended_calls_are_ordered_after_the_callers_stream(ctx, case, mode):
    """Read after write on the input; synchronous: the stream has drained on return (run_ordering
    asserts both, and that the producer was still pending when the call was made)."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", WARS, ids=lambda c: c.name)
def test_extended_outputs_written_after_earlier_readers(ctx, case, mode):
    """Write after read on an out-of-place output."""
    sc.run_war(ctx, case, mode)
