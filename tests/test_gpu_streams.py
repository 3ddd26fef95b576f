"""The caller-stream contract of every `*_device` entry point (include/svgpu.h, "Streams";
INTEGRATION.md, "Streams"):

1. everything enqueued on `stream` before a call happens-before every read and write the call makes
   through its device pointers; NULL means the device's legacy default stream;
2. every call but the two Poseidon device calls is synchronous: on return its outputs are complete
   and, given 1, so is all the work enqueued on `stream` before it;
3. the Poseidon device calls are enqueued on `stream` and return at once; their results are ordered
   for later work on the same stream.

The harness, its cases and how the delay is sized are in tests/stream_cases.py.  Every ordering case
runs in two modes: `null` (torch's default stream, whose handle is 0: the library runs on a stream of
its own that it orders after the default stream) and `side` (a torch.cuda.Stream made current: the
library runs on that stream).  tests/COVERAGE.md, "Caller streams", has the ledger and the measured
figures."""
import os
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import stream_cases as sc
from conftest import ROOT
from oracle import bn254 as b

pytestmark = pytest.mark.gpu

MODES = ["null", "side"]


@pytest.fixture(scope="module")
def ctx(gpu, oracle_cpp):
    c = sc.Context(gpu, oracle_cpp)
    yield c
    torch.cuda.synchronize()
    c.close()


def test_delay_calibration(ctx):
    """The figures the delay is sized from (printed for the ledger), and that it is what the module
    says: 50 x the slowest warm call, at least 10 ms, and reached when asked for."""
    d = ctx.delay
    cycles, ms = d.calibration
    print(f"\n_sleep calibration: {cycles} cycles in {ms:.3f} ms = {d.cycles_per_ms:.0f} cycles/ms; "
          f"delay target {d.target_ms:.2f} ms")
    for name, w in sorted(d.warm_ms.items(), key=lambda kv: -kv[1]):
        print(f"  warm {w:8.3f} ms  {name}")
    assert set(d.warm_ms) == {c.name for c in sc.CASES + sc.WARS}
    assert d.target_ms >= 10.0 and d.target_ms >= 50 * max(d.warm_ms.values())
    token = d.enqueue()
    assert not torch.cuda.current_stream().query()
    d.check(token)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_ordered_after_the_callers_stream(ctx, case, mode):
    """Read after write: the call's device inputs are produced behind a delay on the caller's stream."""
    sc.run_ordering(ctx, case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sc.WARS, ids=lambda c: c.name)
def test_output_written_after_earlier_readers(ctx, case, mode):
    """Write after read: earlier work on the caller's stream (a clone behind the delay) still reads
    the buffer the call writes."""
    sc.run_war(ctx, case, mode)


def test_cold_key_decide_on_a_side_stream():
    """A process whose first decide runs under a side stream: the key's lines are uploaded on the
    caller's stream (decider_lines).  A fresh child; it compares with the C++ oracle itself."""
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "stream_decide_child.py")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "OK"


def test_bdfg21_round_trip_under_one_side_stream(ctx):
    """Uploads, construction (the evaluation passes), W and W' under one side stream, no
    synchronisation of the test's own in between."""
    import svgpu
    polys = [ctx.A[0][:sc.SHPLONK_LENS[0]], ctx.A[1][:sc.SHPLONK_LENS[1]]]
    h, q = sc._reference(sc.SHPLONK_SETS, polys, sc.Z, sc.MU, sc.GAMMA, sc.ZP)
    want = ([sc._horner(polys[p], s * sc.Z % b.R)[1] for p, s in sc.SHPLONK_QUERIES], ctx.witness(h), ctx.witness(q))
    with torch.cuda.stream(torch.cuda.Stream(ctx.gpu)):
        T = [sc.dev(sc._limbs(a, sc.CANONICAL), ctx.gpu) for a in polys]
        got = svgpu.bdfg21_open(ctx.rset, T, sc.SHPLONK_QUERIES, sc.Z, (sc.MU, sc.GAMMA, sc.ZP), offset=sc.OFF,
                                form=sc.CANONICAL)
    assert got == want


THREADS, ROUNDS = 8, 4


def test_eight_threads_each_on_its_own_stream(ctx, oracle_cpp):
    """Pooled workspaces move between callers' streams: eight threads, each with its own stream, its
    own inputs and its own oracle answers, run the harness on one resident handle
    (msm_bases_device, n = 16384) and on msm_batch_device (count = 65), four rounds each.  No
    thread's answer may depend on another thread's pending work."""
    cases = [sc.Case("msm_bases_device-16384", sc._msm_bases(16384)), sc.Case("msm_batch_device-65", sc._msm_batch(65))]
    states = []
    for i in range(THREADS):
        scalars = [oracle_cpp.gen_scalars(b.SEED_SCALARS, 16384, start=(20 + 2 * i + k) * sc.NB) for k in range(2)]
        states.append([c.build(ctx, scalars) for c in cases])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(ctx.gpu) for _ in range(THREADS)]
    warm = threading.Barrier(THREADS)

    def job(i):
        with torch.cuda.stream(streams[i]):
            warm.wait(timeout=60)
            for st in states[i]:              # all threads at once: every workspace they will lease has grown
                st["call"]()
            streams[i].synchronize()
            for _ in range(ROUNDS):
                for case, st in zip(cases, states[i]):
                    sc._fill(st, "stale")
                    streams[i].synchronize()
                    wrong = sc.ordered_call(case, st, streams[i], ctx.delay)
                    assert not wrong, (i, case.name, wrong)
        return True

    with ThreadPoolExecutor(THREADS) as ex:
        assert all(f.result(timeout=300) for f in [ex.submit(job, i) for i in range(THREADS)])
