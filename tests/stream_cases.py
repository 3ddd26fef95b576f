"""Helpers of tests/test_gpu_streams.py (not collected by pytest): the caller-stream contract of the
`*_device` entry points (include/svgpu.h, "Streams").

The pending-producer harness.  A case names the device inputs of one call, a *stale but valid*
content for them and the true content, and what the oracle gives for each.  The harness

1. writes the stale content and synchronises, makes one warm-up call (pool growth and key uploads
   free and allocate device memory, which synchronises the device and would hide a race) and
   checks that it returns the oracle's result for the stale inputs, synchronises;
2. on the stream under test enqueues a calibrated device delay (torch.cuda._sleep: one block, it
   takes no compute unit from the call) and behind it the copies of the true content;
3. asserts that the stream is still busy (a run whose producer is no longer pending proves
   nothing, so it FAILS), makes the call, and for a synchronous call asserts that the stream has
   drained on return;
4. compares the result with the oracle's for the true inputs, bit for bit, and asserts that it is
   not the stale result; then asserts by events that the delay lasted as long as it was sized for.

A call that read its inputs before the caller's stream produced them returns the stale result (or,
having read half-copied data, neither); one that returned before its stream drained fails step 3.

The delay is sized once per session (Delay): cycles per millisecond from one timed _sleep, then
50 x the warm wall time of the slowest call of the file, at least 10 ms.  Every expected value comes
from oracle/ (the C++ Pippenger and decider, the Python Poseidon) or from Python-int arithmetic."""
import contextlib
import ctypes
import os
import random
import time

import numpy as np
import torch

from oracle import bn254 as b
from oracle import poseidon as op
from test_gpu_kzg_open import _horner, _ints, _limb_bytes, _limbs
from test_gpu_kzg_open_batch import _combine
from test_gpu_shplonk_open import _reference

CANONICAL = 0
NB = 1 << 16                    # the shared base set: rows of the resident set and of every MSM case
NA = 20000                      # the shared coefficients
OFF = 37                        # a non-zero offset into the resident set
TERMS = 17                      # terms per MSM of the batched cases
Z, V, MU, GAMMA, ZP, W1 = (b.gen_scalar(b.SEED_SCALARS, 818100 + i) for i in range(6))
XS = [b.gen_scalar(b.SEED_SCALARS, 828200 + i) for i in range(5)]
PATTERN = 0x5A5A5A5A5A5A5A5A    # what a write-after-read case leaves in the output before the call
ONE12 = [1] + [0] * 11          # Gt's identity


def dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C").view(np.int64)).to(gpu)  # a copy: the shared inputs are read-only


def _pt(raw):
    return b.g1_from_bytes(raw.tobytes())


def _points_of(t):
    from svgpu import encoding as enc
    return [enc.g1_from_limbs(r) for r in t.cpu().numpy().view(np.uint64)]


def _ints_of(t):
    return _ints(t.cpu().numpy().view(np.uint64))


@contextlib.contextmanager
def environ(env):
    """The per-call switches of a case, set for its calls only."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Delay:
    """The bounded device delay: torch.cuda._sleep(cycles), calibrated with events."""
    FLOOR_MS = 10.0
    TIMES = 50          # the delay against the slowest call
    MARGIN = 1.5        # cycles asked for against cycles computed: the check below is on the target

    def __init__(self):
        torch.cuda._sleep(1000)  # loads the kernel
        torch.cuda.synchronize()
        cycles = 1_000_000
        while True:                # one short sleep; longer only if it was too short to time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0 or cycles >= 10 ** 10:
                break
            cycles *= 10
        assert ms > 0
        self.cycles_per_ms = cycles / ms
        self.calibration = (cycles, ms)
        self.warm_ms = {}
        self.target_ms = None

    def size(self, warm_ms):
        self.warm_ms = dict(warm_ms)
        self.target_ms = max(self.FLOOR_MS, self.TIMES * max(warm_ms.values()))

    def enqueue(self, factor=1.0):
        """The delay on the current stream -> a token for check()."""
        target = self.target_ms * factor
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(int(target * self.MARGIN * self.cycles_per_ms))
        e1.record()
        return e0, e1, target

    @staticmethod
    def check(token):
        e0, e1, target = token
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms >= target, f"the delay lasted {ms:.2f} ms, sized for {target:.2f} ms"


class Case:
    """One call under the harness.  build(ctx) -> dict(inputs=[(tensor the call reads, true
    content, stale content)], call=() -> raw result, finish=raw -> comparable value (read-backs
    happen here, after the stream query), want=, stale=)."""

    def __init__(self, name, build, env=None, sync=True):
        self.name, self.build, self.env, self.sync = name, build, env or {}, sync


class War:
    """A write-after-read case.  build(ctx) -> dict(out=the output tensor, call=, read=() -> bytes
    of the result, want=bytes)."""

    def __init__(self, name, build):
        self.name, self.build = name, build


# ---- the cases --------------------------------------------------------------------------------

def _msm_device(n):
    def build(c):
        from svgpu import device as dv
        Bt, Bs, St, Ss = c.B[0][:n], c.B[1][:n], c.S[0][:n], c.S[1][:n]
        Bd, Sd = dev(Bs, c.gpu), dev(Ss, c.gpu)
        return dict(inputs=[(Bd, dev(Bt, c.gpu), dev(Bs, c.gpu)), (Sd, dev(St, c.gpu), dev(Ss, c.gpu))],
                    call=lambda: dv.msm(Bd, Sd, CANONICAL),
                    want=_pt(c.o.msm_pippenger(Bt, St, 0)), stale=_pt(c.o.msm_pippenger(Bs, Ss, 0)))
    return build


def _bases_create(c):
    import svgpu
    n = 16384
    Bt, Bs, S = c.B[0][:n], c.B[1][:n], c.S[2][:n]
    T = dev(Bs, c.gpu)

    def finish(rs):
        with rs:
            return rs.msm_arrays(S)
    return dict(inputs=[(T, dev(Bt, c.gpu), dev(Bs, c.gpu))],
                call=lambda: svgpu.ResidentBases.from_device(T, form=CANONICAL), finish=finish,
                want=_pt(c.o.msm_pippenger(Bt, S, 0)), stale=_pt(c.o.msm_pippenger(Bs, S, 0)))


def _msm_bases(n):
    def build(c, scalars=None):
        St, Ss = (a[:n] for a in (scalars or c.S[:2]))
        Sd = dev(Ss, c.gpu)
        Bn = c.B[0][OFF:OFF + n]
        return dict(inputs=[(Sd, dev(St, c.gpu), dev(Ss, c.gpu))],
                    call=lambda: c.rset.msm_device(Sd, offset=OFF, form=CANONICAL),
                    want=_pt(c.o.msm_pippenger(Bn, St, 0)), stale=_pt(c.o.msm_pippenger(Bn, Ss, 0)))
    return build


def _coeff_input(c, n, lo=0):
    at, as_ = c.A[0][lo:lo + n], c.A[1][lo:lo + n]
    A = dev(_limbs(as_, CANONICAL), c.gpu)
    return at, as_, A, (A, dev(_limbs(at, CANONICAL), c.gpu), dev(_limbs(as_, CANONICAL), c.gpu))


def _poly_div(n):
    def build(c):
        from svgpu import device as dv
        at, as_, A, inp = _coeff_input(c, n)

        def exp(a):
            q, v = _horner(a, Z)
            return v, _limb_bytes(q, CANONICAL)
        return dict(inputs=[inp], call=lambda: dv.poly_div_linear_device(A, Z, form=CANONICAL),
                    finish=lambda r: (r[0], r[1].cpu().numpy().tobytes()), want=exp(at), stale=exp(as_))
    return build


def _poly_div_strided(c):
    """Through the mirror with a strided view: the mirror's own .contiguous() copy, enqueued behind
    the pending producer of the view's storage, is what the call has to wait for."""
    from svgpu import device as dv
    n = 257
    at, as_ = c.A[0][:n], c.A[1][:n]

    def wide(a):
        rows = np.zeros((2 * n, 4), np.uint64)
        rows[::2] = _limbs(a, CANONICAL)
        return dev(rows, c.gpu)
    A2 = wide(as_)

    def exp(a):
        q, v = _horner(a, Z)
        return v, _limb_bytes(q, CANONICAL)
    return dict(inputs=[(A2, wide(at), wide(as_))],
                call=lambda: dv.poly_div_linear_device(A2[::2], Z, form=CANONICAL),
                finish=lambda r: (r[0], r[1].cpu().numpy().tobytes()), want=exp(at), stale=exp(as_))


def _kzg_open(n):
    def build(c):
        at, as_, A, inp = _coeff_input(c, n)

        def exp(a):
            q, v = _horner(a, Z)
            return v, c.witness(q)
        return dict(inputs=[inp], call=lambda: c.rset.open_device(A, Z, offset=OFF, form=CANONICAL),
                    want=exp(at), stale=exp(as_))
    return build


BATCH_LENS = [2049, 1025, 300]  # ragged; the middle polynomial is the one produced behind the delay


def _batch_polys(c):
    p0, p2 = c.A[0][:BATCH_LENS[0]], c.A[0][5000:5000 + BATCH_LENS[2]]
    at, as_, A, inp = _coeff_input(c, BATCH_LENS[1], lo=3000)
    T = [dev(_limbs(p0, CANONICAL), c.gpu), A, dev(_limbs(p2, CANONICAL), c.gpu)]
    return [p0, at, p2], [p0, as_, p2], T, inp


def _combine_eval(c):
    from svgpu import device as dv
    pt_, ps, T, inp = _batch_polys(c)

    def exp(polys):
        return [_horner(a, Z)[1] for a in polys], _limb_bytes(_combine(polys, V), CANONICAL)
    return dict(inputs=[inp], call=lambda: dv.poly_combine_eval_device(T, Z, V, form=CANONICAL),
                finish=lambda r: (r[0], r[1].cpu().numpy().tobytes()), want=exp(pt_), stale=exp(ps))


def _open_batch(c):
    pt_, ps, T, inp = _batch_polys(c)

    def exp(polys):
        return [_horner(a, Z)[1] for a in polys], c.witness(_horner(_combine(polys, V), Z)[0])
    return dict(inputs=[inp], call=lambda: c.rset.open_batch_device(T, Z, V, offset=OFF, form=CANONICAL),
                want=exp(pt_), stale=exp(ps))


def _eval_points(K):
    def build(c):
        from svgpu import device as dv
        at, as_, A, inp = _coeff_input(c, 1025)
        return dict(inputs=[inp], call=lambda: dv.poly_eval_points_device([A], XS[:K], form=CANONICAL),
                    want=[[_horner(at, x)[1] for x in XS[:K]]], stale=[[_horner(as_, x)[1] for x in XS[:K]]])
    return build


def _div_roots(K):
    def build(c):
        from svgpu import device as dv
        at, as_, A, inp = _coeff_input(c, 1025)

        def exp(a):
            for x in XS[:K]:
                a = _horner(a, x)[0]
            return _limb_bytes(a, CANONICAL)
        return dict(inputs=[inp], call=lambda: dv.poly_div_roots_device(A, XS[:K], form=CANONICAL),
                    finish=lambda r: r.cpu().numpy().tobytes(), want=exp(at), stale=exp(as_))
    return build


SHPLONK_LENS = [1025, 600]
SHPLONK_QUERIES = [(0, 1), (1, 1), (1, W1)]
SHPLONK_SETS = [([1], [0]), ([1, W1], [1])]  # two sets, of one and two points; N = 1025


def _shplonk(c):
    """-> (the opening, its polynomials' tensors, the true and the stale polynomials).  The opening
    is constructed under a stream of its own, which is neither of the streams it is called under:
    Bdfg21Opening reads the current stream per call."""
    import svgpu
    pt_ = [c.A[0][:SHPLONK_LENS[0]], c.A[0][7000:7000 + SHPLONK_LENS[1]]]
    ps = [c.A[1][:SHPLONK_LENS[0]], c.A[1][7000:7000 + SHPLONK_LENS[1]]]
    T = [dev(_limbs(a, CANONICAL), c.gpu) for a in ps]
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        opening = svgpu.Bdfg21Opening(c.rset, T, SHPLONK_QUERIES, Z, offset=OFF, form=CANONICAL)
    return opening, T, pt_, ps


def _shplonk_quotient(c):
    opening, T, pt_, ps = _shplonk(c)
    inputs = [(t, dev(_limbs(a, CANONICAL), c.gpu), dev(_limbs(s, CANONICAL), c.gpu)) for t, a, s in zip(T, pt_, ps)]
    return dict(inputs=inputs, call=lambda: opening.quotient(MU, GAMMA), keep=opening,
                want=c.witness(_reference(SHPLONK_SETS, pt_, Z, MU, GAMMA, ZP)[0]),
                stale=c.witness(_reference(SHPLONK_SETS, ps, Z, MU, GAMMA, ZP)[0]))


def _shplonk_witness(c):
    """The second call reads only the work buffer: it is overwritten with the (valid) work of the
    stale polynomials' opening and restored behind the delay.  Both contents are what
    quotient() left there; the expected W' are the oracle's."""
    opening, T, pt_, ps = _shplonk(c)
    work = {}
    for key, polys in (("stale", ps), ("true", pt_)):
        for t, a in zip(T, polys):
            t.copy_(dev(_limbs(a, CANONICAL), c.gpu))
        torch.cuda.synchronize()
        opening.quotient(MU, GAMMA)
        torch.cuda.synchronize()
        work[key] = opening.work.clone()
    torch.cuda.synchronize()
    return dict(inputs=[(opening.work, work["true"], work["stale"])], call=lambda: opening.witness(ZP),
                want=c.witness(_reference(SHPLONK_SETS, pt_, Z, MU, GAMMA, ZP)[1]),
                stale=c.witness(_reference(SHPLONK_SETS, ps, Z, MU, GAMMA, ZP)[1]))


def _batch_expected(c, B, S, count):
    return [_pt(c.o.msm_pippenger(B[k * TERMS:(k + 1) * TERMS], S[k * TERMS:(k + 1) * TERMS], 1)) for k in range(count)]


def _msm_batch(count):
    def build(c, scalars=None):
        from svgpu import device as dv
        n = count * TERMS
        B = c.B[0][:n]
        St, Ss = (a[:n] for a in (scalars or c.S[:2]))
        Bd, Sd = dev(B, c.gpu), dev(Ss, c.gpu)
        od = torch.arange(0, n + 1, TERMS, dtype=torch.int64, device=c.gpu)
        return dict(inputs=[(Sd, dev(St, c.gpu), dev(Ss, c.gpu))],
                    call=lambda: dv.msm_batch(Bd, Sd, od, TERMS, CANONICAL), finish=_points_of,
                    want=_batch_expected(c, B, St, count), stale=_batch_expected(c, B, Ss, count))
    return build


def _batch_indexed(table):
    def build(c):
        from svgpu import device as dv
        rows, count = 16, 8
        n = count * TERMS
        Th = c.B[0][:rows]
        rng = np.random.default_rng(16)
        it, is_ = (rng.integers(0, rows, n).astype(np.uint32) for _ in range(2))
        St, Ss = c.S[0][:n], c.S[1][:n]
        idx = torch.from_numpy(is_.view(np.int32)).to(c.gpu)
        Sd = dev(Ss, c.gpu)
        od = torch.arange(0, n + 1, TERMS, dtype=torch.int64, device=c.gpu)
        inputs = [(idx, torch.from_numpy(it.view(np.int32)).to(c.gpu), torch.from_numpy(is_.view(np.int32)).to(c.gpu)),
                  (Sd, dev(St, c.gpu), dev(Ss, c.gpu))]
        if table:
            call = lambda: c.table.msm_batch_device(idx, Sd, od, CANONICAL)  # noqa: E731
        else:
            Td = dev(Th, c.gpu)
            call = lambda: dv.msm_batch_indexed(Td, idx, Sd, od, TERMS, form=CANONICAL, table_form=CANONICAL)  # noqa: E731
        return dict(inputs=inputs, call=call, finish=_points_of,
                    want=_batch_expected(c, Th[it], St, count), stale=_batch_expected(c, Th[is_], Ss, count))
    return build


def decider_case(bad, start):
    """-> (g2, s_g2, lhs rows, rhs rows) of four accumulators under ONE key (the seed fixes s)."""
    from svgpu import encoding as enc
    g2, sg2, accs = b.gen_decider_case(4, seed=0x57AE, bad=bad, start=start)
    return g2, sg2, enc.bases_array([a[0] for a in accs]), enc.bases_array([a[1] for a in accs])


def decider_expected(o, g2, sg2, L, R):
    from svgpu import encoding as enc
    ff, egt = o.decide_all(np.frombuffer(b.g2_bytes(g2), np.uint64), np.frombuffer(b.g2_bytes(sg2), np.uint64),
                           L, R, threads=0, want_gt=True)
    gts = [[enc.limbs_to_int(egt[i][4 * k:4 * k + 4]) for k in range(12)] for i in range(len(L))]
    return ff, [g == ONE12 for g in gts], gts


def _decide(c):
    """Stale: four valid accumulators of which three fail; true: others, of which one fails.  The
    warm-up call uploads the key's lines (a cold key allocates: the ordering case wants it warm)."""
    from svgpu import device as dv
    g2, sg2, Lt, Rt = decider_case([2], 0)
    _, _, Ls, Rs = decider_case([0, 1, 3], 100)
    Ld, Rd = dev(Ls, c.gpu), dev(Rs, c.gpu)

    def finish(r):
        return r[0], [bool(v) for v in r[1]], [[int(x) for x in g] for g in r[2]]
    return dict(inputs=[(Ld, dev(Lt, c.gpu), dev(Ls, c.gpu)), (Rd, dev(Rt, c.gpu), dev(Rs, c.gpu))],
                call=lambda: dv.decide(g2, sg2, Ld, Rd, CANONICAL, want_gt=True), finish=finish,
                want=decider_expected(c.o, g2, sg2, Lt, Rt), stale=decider_expected(c.o, g2, sg2, Ls, Rs))


def _decode(encoding, n):
    def build(c):
        from svgpu import _lib, encoding as enc
        code = _lib.SV_ENC_EVM if encoding == "evm" else _lib.SV_ENC_HALO2_COMPRESSED
        encode = b.g1_evm_encode if encoding == "evm" else b.g1_compress
        pts = [[enc.g1_from_limbs(r) for r in c.B[k][:n - 1]] + [None] for k in (0, 1)]  # the identity last
        data = [torch.from_numpy(np.frombuffer(b"".join(encode(p) for p in ps), np.uint8).copy()).to(c.gpu) for ps in pts]
        D = data[1].clone()
        out = torch.zeros((n, 8), dtype=torch.int64, device=c.gpu)

        def call():
            bad = ctypes.c_int64(-1)
            _lib.check(_lib.lib.sv_bn254_g1_decode_device(D.data_ptr(), n, code, CANONICAL, 0,
                                                          torch.cuda.current_stream(c.gpu).cuda_stream, out.data_ptr(),
                                                          ctypes.byref(bad)), "sv_bn254_g1_decode_device")
            return out
        return dict(inputs=[(D, data[0], data[1])], call=call, finish=_points_of, want=pts[0], stale=pts[1])
    return build


POSEIDON_N = 300


def _permute(t):
    def build(c):
        from svgpu import device as dv, encoding as enc
        rng = random.Random(300 + t)
        true = [[rng.randrange(b.R) for _ in range(t)] for _ in range(POSEIDON_N)]
        buf = dev(enc.scalars_array([0] * (POSEIDON_N * t)), c.gpu)   # in place: the input is the output
        return dict(inputs=[(buf, dev(enc.scalars_array([v for s in true for v in s]), c.gpu), torch.zeros_like(buf))],
                    call=lambda: dv.poseidon_permute(buf, t, CANONICAL), finish=_ints_of,
                    want=[v for s in true for v in op.permutation(s, t, *op.PARAMS[t])],
                    stale=op.permutation([0] * t, t, *op.PARAMS[t]) * POSEIDON_N)
    return build


def _squeeze(t):
    def build(c):
        from svgpu import device as dv, encoding as enc
        rng = random.Random(500 + t)
        lens = [(0, 1, 2, 3, t + 1)[j % 5] for j in range(POSEIDON_N)]
        offs = [0]
        for m in lens:
            offs.append(offs[-1] + m)
        true = [rng.randrange(b.R) for _ in range(offs[-1])]
        default = dev(enc.scalars_array(([1 << 64] + [0] * (t - 1)) * POSEIDON_N), c.gpu)
        states = default.clone()                                       # in and out: restored with the inputs
        els = dev(enc.scalars_array([0] * offs[-1]), c.gpu)
        od = torch.tensor(offs, dtype=torch.int64, device=c.gpu)
        out = torch.zeros((POSEIDON_N, 4), dtype=torch.int64, device=c.gpu)

        def exp(values):
            memo, res, sts = {}, [], []
            for j in range(POSEIDON_N):
                key = tuple(values[offs[j]:offs[j + 1]])
                if key not in memo:
                    s = op.Sponge(t)
                    s.update(key)
                    memo[key] = (s.squeeze(), list(s.state))
                res.append(memo[key][0])
                sts += memo[key][1]
            return res, sts
        return dict(inputs=[(states, default, default), (els, dev(enc.scalars_array(true), c.gpu), torch.zeros_like(els))],
                    call=lambda: dv.poseidon_squeeze(states, els, od, t, CANONICAL, out),
                    finish=lambda r: (_ints_of(r), _ints_of(states)), want=exp(true), stale=exp([0] * offs[-1]))
    return build


CASES = [
    Case("msm_device-200-small", _msm_device(200)),
    Case("msm_device-257-pipeline", _msm_device(257)),
    Case("msm_device-16384-glv", _msm_device(16384)),
    # SVGPU_MSM_SPLIT applies from 2^16 points (msm_plan.hpp msm_shape): 20 000 stays on run_device,
    # 65 536 is the smallest size whose half B is sorted on the sort stream forked from the caller's
    Case("msm_device-20000-split-not-reached", _msm_device(20000), env={"SVGPU_MSM_SPLIT": "1"}),
    Case("msm_device-65536-split", _msm_device(1 << 16), env={"SVGPU_MSM_SPLIT": "1"}),
    Case("bases_create_device-16384", _bases_create),
    Case("msm_bases_device-256", _msm_bases(256)),
    Case("msm_bases_device-16384", _msm_bases(16384)),
    Case("poly_div_linear_device-1", _poly_div(1)),
    Case("poly_div_linear_device-257", _poly_div(257)),
    Case("poly_div_linear_device-16385", _poly_div(16385)),
    Case("poly_div_linear_device-strided-257", _poly_div_strided),
    Case("kzg_open_device-1", _kzg_open(1)),
    Case("kzg_open_device-257", _kzg_open(257)),
    Case("kzg_open_device-16385", _kzg_open(16385)),
    Case("poly_combine_eval_device-3", _combine_eval),
    Case("kzg_open_batch_device-3", _open_batch),
    Case("poly_eval_points_device-K1", _eval_points(1)),
    Case("poly_eval_points_device-K5", _eval_points(5)),
    Case("poly_div_roots_device-K1", _div_roots(1)),
    Case("poly_div_roots_device-K5", _div_roots(5)),
    Case("shplonk_quotient_device", _shplonk_quotient),
    Case("shplonk_witness_device", _shplonk_witness),
    Case("msm_batch_device-8-host", _msm_batch(8)),
    Case("msm_batch_device-65-fused", _msm_batch(65)),
    Case("msm_batch_device-513-two-kernels", _msm_batch(513)),
    Case("msm_batch_table_device-8", _batch_indexed(True)),
    Case("msm_batch_indexed_device-8", _batch_indexed(False)),
    Case("kzg_decide_device-4-wg", _decide),
    Case("kzg_decide_device-4-lanes48", _decide, env={"SVGPU_DECIDER_LANES": "48"}),
    Case("g1_decode_device-300-compressed", _decode("compressed", 300)),
    Case("g1_decode_device-257-evm", _decode("evm", 257)),
    Case("poseidon_permute_device-t3", _permute(3), sync=False),
    Case("poseidon_permute_device-t5", _permute(5), sync=False),
    Case("poseidon_squeeze_device-t3", _squeeze(3), sync=False),
    Case("poseidon_squeeze_device-t5", _squeeze(5), sync=False),
]


def _pattern(shape, gpu):
    return torch.full(shape, PATTERN, dtype=torch.int64, device=gpu)


def _war_gen(kind):
    def build(c):
        from svgpu import device as dv
        n = 1000
        if kind == "scalars":
            out, want = _pattern((n, 4), c.gpu), c.o.gen_scalars(b.SEED_SCALARS, n, start=4242)
            call = lambda: dv.gen_scalars(out, b.SEED_SCALARS, 4242, CANONICAL)  # noqa: E731
        else:
            out, want = _pattern((n, 8), c.gpu), c.o.gen_bases(b.SEED_BASES, n, start=4242)
            call = lambda: dv.gen_bases(out, b.SEED_BASES, 4242, CANONICAL)  # noqa: E731
        return dict(out=out, call=call, want=want.tobytes())
    return build


def _war_poly_div(c):
    from svgpu import device as dv
    n = 257
    a = c.A[0][:n]
    A, out = dev(_limbs(a, CANONICAL), c.gpu), _pattern((n - 1, 4), c.gpu)
    return dict(out=out, call=lambda: dv.poly_div_linear_device(A, Z, form=CANONICAL, out=out),
                want=_limb_bytes(_horner(a, Z)[0], CANONICAL))


def _war_msm_batch(count):
    def build(c):
        from svgpu import device as dv, encoding as enc
        n = count * TERMS
        B, S = c.B[0][:n], c.S[0][:n]
        Bd, Sd, out = dev(B, c.gpu), dev(S, c.gpu), _pattern((count, 8), c.gpu)
        od = torch.arange(0, n + 1, TERMS, dtype=torch.int64, device=c.gpu)
        return dict(out=out, call=lambda: dv.msm_batch(Bd, Sd, od, TERMS, CANONICAL, out=out),
                    want=enc.bases_array(_batch_expected(c, B, S, count)).tobytes())
    return build


WARS = [
    War("gen_scalars_device-1000", _war_gen("scalars")),
    War("gen_bases_device-1000", _war_gen("bases")),
    War("poly_div_linear_device-out-257", _war_poly_div),
    War("msm_batch_device-out-8-host", _war_msm_batch(8)),
    War("msm_batch_device-out-65-fused", _war_msm_batch(65)),
]


# ---- the session's context and the harness ------------------------------------------------------

class Context:
    """Shared inputs (never modified by a test), the resident set and base table, every case built
    once, each case's warm wall time, and the delay sized from the slowest."""

    def __init__(self, gpu, oracle):
        import svgpu
        self.gpu, self.o = gpu, oracle
        self.B = [oracle.gen_bases(b.SEED_BASES, NB, start=k * NB) for k in range(2)]
        self.S = [oracle.gen_scalars(b.SEED_SCALARS, NB, start=k * NB) for k in range(3)]
        self.A = [_ints(oracle.gen_scalars(b.SEED_SCALARS, NA, start=(5 + k) * NB)) for k in range(2)]
        for a in self.B + self.S:
            a.setflags(write=False)
        self.rset = svgpu.ResidentBases(self.B[0])
        self.table = svgpu.BaseTable(self.B[0][:16])
        self.built = {}
        self.delay = Delay()
        warm = {}
        for case in CASES + WARS:
            st = self.built[case.name] = case.build(self)
            torch.cuda.synchronize()
            with environ(getattr(case, "env", {})):
                for _ in range(2):           # the first call grows the pool; the second is the warm one
                    t0 = time.perf_counter()
                    raw = st["call"]()
                    torch.cuda.synchronize()
                    warm[case.name] = (time.perf_counter() - t0) * 1e3
                    if isinstance(case, Case) and "finish" in st and case.name.startswith("bases_create"):
                        st["finish"](raw)    # the handle of a created set is closed
        self.delay.size(warm)

    def witness(self, q):
        if not q:
            return None
        return _pt(self.o.msm_pippenger(self.B[0][OFF:OFF + len(q)], _limbs(q, CANONICAL), 0))

    def close(self):
        self.built.clear()
        self.rset.close()
        self.table.close()


@contextlib.contextmanager
def stream_mode(mode, gpu):
    """null: the device's default stream (handle 0); side: a new stream made current."""
    if mode == "null":
        s = torch.cuda.current_stream(gpu)
        assert s.cuda_stream == 0, "the test thread's current stream is not the default stream"
        yield s
    else:
        s = torch.cuda.Stream(gpu)
        assert s.cuda_stream != 0
        with torch.cuda.stream(s):
            yield s


def passes(mode):
    """A process has few hardware queues (four by default) and the runtime spreads its streams over
    them.  A library stream that shares the side stream's queue runs behind the delay whether the
    library ordered it or not, and the case would pass by accident (measured: with WsLease made to
    ignore the caller's stream, 7 of 31 side cases passed on one stream).  So a side case runs twice,
    on two streams created one after the other, which the runtime puts on different queues."""
    return 2 if mode == "side" else 1


def _fill(st, which):
    for dst, true, stale in st["inputs"]:
        dst.copy_(true if which == "true" else stale)


def ordered_call(case, st, stream, delay, factor=1.0):
    """Steps 2-4 of the harness on `stream`, which is current: asserts that the producer was pending
    at call time and that the delay reached its target, and judges the rest -> a list of what is
    wrong with the call (empty: it kept the contract).  Everything is looked at before anything is
    reported, so a failure names every way the call failed."""
    finish = st.get("finish", lambda r: r)
    token = delay.enqueue(factor)
    _fill(st, "true")
    assert not stream.query(), "the producer is no longer pending: the delay is too short to prove anything"
    raw = st["call"]()
    drained = stream.query()
    got = finish(raw)
    stream.synchronize()
    delay.check(token)
    wrong = []
    if case.sync and not drained:
        wrong.append("a synchronous call returned with work still pending on the caller's stream")
    if not case.sync and drained:
        wrong.append("the call is documented to return at once, but the stream had drained")
    if got == st["stale"]:
        wrong.append("the call read its inputs before the caller's stream produced them (the stale result)")
    elif got != st["want"]:
        wrong.append("the result is neither the oracle's nor the stale one (inputs read while they were produced?)")
    return wrong


def run_ordering(ctx, case, mode):
    st = ctx.built[case.name]
    finish = st.get("finish", lambda r: r)
    assert st["want"] != st["stale"], "the stale inputs must give another result"
    wrong = []
    with environ(case.env):
        for k in range(passes(mode)):
            _fill(st, "stale")
            torch.cuda.synchronize()
            warm = finish(st["call"]())
            torch.cuda.synchronize()
            assert warm == st["stale"], "the warm-up call on the stale inputs (nothing pending) is wrong"
            with stream_mode(mode, ctx.gpu) as stream:
                wrong += [f"stream {k}: {w}" for w in ordered_call(case, st, stream, ctx.delay)]
    assert not wrong, "; ".join(wrong)


def run_war(ctx, case, mode):
    st = ctx.built[case.name]
    out = st["out"]
    old = bytes(np.full(out.numel(), PATTERN, np.int64).tobytes())
    assert st["want"] != old
    st["call"]()                                    # warm (the pool has grown)
    wrong = []
    for k in range(passes(mode)):
        out.fill_(PATTERN)
        torch.cuda.synchronize()
        with stream_mode(mode, ctx.gpu) as stream:
            token = ctx.delay.enqueue()
            snap = out.clone()                      # the earlier enqueued reader of the output
            assert not stream.query(), "the reader is no longer pending: the delay is too short to prove anything"
            st["call"]()
            drained = stream.query()
            got_snap, got = snap.cpu().numpy().tobytes(), out.cpu().numpy().tobytes()
            ctx.delay.check(token)
        if not drained:
            wrong.append(f"stream {k}: a synchronous call returned with work still pending on the caller's stream")
        if got_snap != old:
            wrong.append(f"stream {k}: the call wrote its output while earlier work on the caller's stream still read it")
        if got != st["want"]:
            wrong.append(f"stream {k}: the output is not the oracle's")
    assert not wrong, "; ".join(wrong)
