"""Host-side mirror of the reference's KZG decider / accumulation, executed on the GPU.

* ``KzgAs.decide`` / ``KzgAs.decide_all`` mirror ``AccumulationDecider for KzgAs`` on
  NativeLoader (snark-verifier/src/pcs/kzg/decider.rs:60-80): pass -> None, failure ->
  ``AssertionFailure("e(lhs, g2)·e(rhs, -s_g2) == O")`` (decider.rs:66-67); an empty list panics
  (``assert!(!accumulators.is_empty())``, decider.rs:74).
* ``KzgAs.create_proof`` / ``KzgAs.verify`` mirror the accumulation MSMs of
  snark-verifier/src/pcs/kzg/accumulation.rs:146-195 / :40-62 without the zk blind:
  lhs = sum r^i lhs_i, rhs = sum r^i rhs_i with r^0 = 1 (snark-verifier/src/loader.rs:71-78).
  ``create_proof(instances, transcript)`` is the reference's own signature: the accumulators' lhs
  and rhs are absorbed through ``transcript.common_ec_point`` and r is squeezed from it
  (accumulation.rs:156-176).  Given a fresh ``PoseidonTranscript`` (what the SDK passes,
  snark-verifier-sdk/src/halo2/aggregation.rs:235-242) the whole call is ONE library call,
  ``sv_bn254_kzg_create_proof`` (host sponge, device MSMs); a used transcript's sponge state goes
  in and comes back out of the same call, and one with buffered input is absorbed and squeezed
  through ``svgpu.poseidon`` first.  An ``int`` in place of the
  transcript is taken as r itself (``sv_bn254_kzg_accumulate``).
"""
from __future__ import annotations

import ctypes
import numbers
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import encoding as enc
from .loader import Point, ReferencePanic

G2Point = Optional[Tuple[Tuple[int, int], Tuple[int, int]]]

DECIDE_MSG = "e(lhs, g2)·e(rhs, -s_g2) == O"


class AssertionFailure(Exception):
    """snark_verifier::Error::AssertionFailure"""


@dataclass(frozen=True)
class KzgDecidingKey:
    """KzgDecidingKey{svk.g, g2, s_g2} (decider.rs:6-30); From<(G1, G2, G2)> (:26-30)."""

    g: Point
    g2: G2Point
    s_g2: G2Point


@dataclass(frozen=True)
class KzgAccumulator:
    """KzgAccumulator{lhs, rhs} (snark-verifier/src/pcs/kzg/accumulator.rs:6-26)."""

    lhs: Point
    rhs: Point


def decide_arrays(dk: KzgDecidingKey, lhs: np.ndarray, rhs: np.ndarray, form: int = _lib.SV_CANONICAL,
                  num_gpus: int = 0) -> int:
    """Batched decider over host arrays (n, 8) u64; returns the first failing index or -1."""
    lhs = np.ascontiguousarray(lhs, dtype=np.uint64)
    rhs = np.ascontiguousarray(rhs, dtype=np.uint64)
    if lhs.shape[0] == 0:
        raise ReferencePanic("assertion failed: !accumulators.is_empty()")
    ff = ctypes.c_int32(-2)
    g2 = enc.g2_struct(dk.g2, form)
    sg2 = enc.g2_struct(dk.s_g2, form)
    _lib.check(_lib.lib.sv_bn254_kzg_decide(ctypes.byref(g2), ctypes.byref(sg2), lhs.ctypes.data, rhs.ctypes.data,
                                            lhs.shape[0], form, num_gpus, ctypes.byref(ff)), "sv_bn254_kzg_decide")
    return ff.value


class KzgAs:
    """KzgAs<Bn256, MOS> on NativeLoader: decider + accumulation (no zk blind)."""

    @staticmethod
    def decide(dk: KzgDecidingKey, acc: KzgAccumulator) -> None:
        KzgAs.decide_all(dk, [acc])

    @staticmethod
    def decide_all(dk: KzgDecidingKey, accumulators: Sequence[KzgAccumulator], num_gpus: int = 0) -> None:
        if len(accumulators) == 0:
            raise ReferencePanic("assertion failed: !accumulators.is_empty()")
        lhs = enc.bases_array([a.lhs for a in accumulators])
        rhs = enc.bases_array([a.rhs for a in accumulators])
        if decide_arrays(dk, lhs, rhs, _lib.SV_CANONICAL, num_gpus) >= 0:
            raise AssertionFailure(DECIDE_MSG)

    @staticmethod
    def first_failure(dk: KzgDecidingKey, accumulators: Sequence[KzgAccumulator], num_gpus: int = 0) -> int:
        lhs = enc.bases_array([a.lhs for a in accumulators])
        rhs = enc.bases_array([a.rhs for a in accumulators])
        return decide_arrays(dk, lhs, rhs, _lib.SV_CANONICAL, num_gpus)

    @staticmethod
    def create_proof(instances: Sequence[KzgAccumulator], transcript=None) -> KzgAccumulator:
        """KzgAs::create_proof with the default proving key (no blind), accumulation.rs:146-195.

        ``transcript``: None or a fresh ``PoseidonTranscript`` -> r from the library's transcript
        (one call); a used ``PoseidonTranscript`` -> absorbed / squeezed through it; an integer
        (``numbers.Integral``: int, numpy integers) -> r."""
        if len(instances) == 0:
            raise ReferencePanic("assertion failed: !instances.is_empty()")
        from .poseidon import PoseidonTranscript
        if isinstance(transcript, numbers.Integral):  # int, numpy integers, ...: r itself
            return KzgAs._accumulate(instances, int(transcript))
        if transcript is not None and (not isinstance(transcript, PoseidonTranscript) or transcript.buf.buf
                                       or transcript.buf.t != 3):
            # a transcript with pending input (or another kind): absorb and squeeze through it
            for a in instances:
                transcript.common_ec_point(a.lhs)
                transcript.common_ec_point(a.rhs)
            return KzgAs._accumulate(instances, transcript.squeeze_challenge())
        lhs = enc.bases_array([a.lhs for a in instances])
        rhs = enc.bases_array([a.rhs for a in instances])
        out_l, out_r = _lib.sv_g1_affine(), _lib.sv_g1_affine()
        r = np.zeros(4, dtype=np.uint64)
        state = None
        if transcript is not None:  # continue from the transcript's sponge state, then hand it back
            state = enc.ints_to_limbs([int(v) for v in transcript.buf.state])
        _lib.check(_lib.lib.sv_bn254_kzg_create_proof(lhs.ctypes.data, rhs.ctypes.data, len(instances),
                                                      _lib.SV_CANONICAL, 0, ctypes.byref(out_l), ctypes.byref(out_r),
                                                      None if state is None else state.ctypes.data, r.ctypes.data),
                   "sv_bn254_kzg_create_proof")
        if transcript is not None:
            transcript.buf.state = [enc.limbs_to_int(row) for row in state]
        KzgAs.last_challenge = enc.limbs_to_int(r)
        return KzgAccumulator(enc.g1_from_struct(out_l), enc.g1_from_struct(out_r))

    last_challenge: Optional[int] = None

    @staticmethod
    def _accumulate(instances: Sequence[KzgAccumulator], r: int) -> KzgAccumulator:
        if not 0 <= r < enc.R:
            raise ValueError("r must be a reduced Fr element")
        lhs = enc.bases_array([a.lhs for a in instances])
        rhs = enc.bases_array([a.rhs for a in instances])
        rr = enc.fe_struct(r)
        out_l, out_r = _lib.sv_g1_affine(), _lib.sv_g1_affine()
        _lib.check(_lib.lib.sv_bn254_kzg_accumulate(lhs.ctypes.data, rhs.ctypes.data, len(instances),
                                                    ctypes.byref(rr), _lib.SV_CANONICAL, 0, ctypes.byref(out_l),
                                                    ctypes.byref(out_r)), "sv_bn254_kzg_accumulate")
        KzgAs.last_challenge = r
        return KzgAccumulator(enc.g1_from_struct(out_l), enc.g1_from_struct(out_r))

    @staticmethod
    def verify(instances: Sequence[KzgAccumulator], transcript=None) -> KzgAccumulator:
        """AccumulationScheme::verify (accumulation.rs:40-62): the same transcript and MSMs."""
        return KzgAs.create_proof(instances, transcript)


def gwc19_query_sets(queries: Sequence[Tuple[int, int]]) -> list:
    """The point sets of a GWC19 opening, grouped as the reference's query_sets does
    (snark-verifier/src/pcs/kzg/multiopen/gwc19.rs:140-158): sets in order of the first appearance of
    a shift, each with its polynomials in query order -> [(shift, [poly index], [query index])]."""
    sets: list = []
    for qi, (poly, shift) in enumerate(queries):
        for s in sets:
            if s[0] == shift:
                s[1].append(poly)
                s[2].append(qi)
                break
        else:
            sets.append((shift, [poly], [qi]))
    return sets


def bdfg21_query_sets(queries: Sequence[Tuple[int, int]]) -> list:
    """The query sets of a SHPLONK opening, grouped as the reference's query_sets does
    (snark-verifier/src/pcs/kzg/multiopen/bdfg21.rs:117-167): first every polynomial collects its
    distinct shifts in query order (a repeated query is dropped), then polynomials group by the SET
    of their shifts, in order of first appearance; a set keeps the shift order of its first
    polynomial -> [([shift], [poly index], [[query index per shift of the set] per polynomial])]."""
    poly_shifts: list = []
    for qi, (poly, shift) in enumerate(queries):
        for ps in poly_shifts:
            if ps[0] == poly:
                if shift not in ps[1]:
                    ps[1].append(shift)
                    ps[2].append(qi)
                break
        else:
            poly_shifts.append((poly, [shift], [qi]))
    sets: list = []
    for poly, shifts, where in poly_shifts:
        for s in sets:
            if set(s[0]) == set(shifts):
                s[1].append(poly)
                s[2].append([where[shifts.index(x)] for x in s[0]])
                break
        else:
            sets.append((shifts, [poly], [where]))
    return sets


class Bdfg21Opening:
    """The prover's side of Bdfg21::verify (bdfg21.rs:47-79) on a resident base set, in the order a
    transcript needs it: the evaluations on construction (`.evals`, one per query, in query order),
    then W = `.quotient(mu, gamma)`, then W' = `.witness(z_prime)`.  `polys` are (n_j, 4) int64 torch
    tensors in `form` in HBM on the set's device, `queries` a list of (poly index, shift), z a
    canonical int; query (p, shift) opens polynomial p at shift * z.  The object owns the work
    buffer that carries the combinations c_i and h from the first call to the second; the library
    keeps nothing.  Two MSMs whatever the number of shifts.

    Streams: nothing is captured at construction.  The constructor's evaluation passes,
    `quotient` and `witness` each run on the stream that is current (torch.cuda.current_stream) on
    the polynomials' device when that call is made, like every other device call of this package;
    each is synchronous, so the three may be made under different streams."""

    def __init__(self, rset, polys, queries: Sequence[Tuple[int, int]], z: int, offset: int = 0,
                 form: int = _lib.SV_MONTGOMERY):
        import torch
        from . import device as dv
        if rset.handle is None:
            raise _lib.ArgumentError("base set is closed")
        self.rset, self.offset, self.form = rset, offset, form
        self.sets = bdfg21_query_sets(queries)
        ordered = [polys[p] for _, members, _ in self.sets for p in members]
        self._keep, self._ptrs, self._lens = dv.batch_tables(ordered)
        self.points, descr, self.set_lens = [], [], []
        first_poly = 0
        for shifts, members, _ in self.sets:
            descr.append((first_poly, len(members), len(self.points), len(shifts)))
            self.set_lens.append(max(self._keep[first_poly + j].shape[0] for j in range(len(members))))
            self.points += [shift * z % enc.R for shift in shifts]
            first_poly += len(members)
        self._sets = (_lib.sv_shplonk_set * max(len(descr), 1))(*[_lib.sv_shplonk_set(*d) for d in descr])
        self._points = dv.fe_array(self.points, form)
        self._set_lens = (ctypes.c_uint64 * max(len(descr), 1))(*self.set_lens)
        # the evaluations enter the transcript before mu exists: one multi-point pass per set
        at = {}
        for (shifts, members, _), (fp, np_, fk, nk) in zip(self.sets, descr):
            sub_p = (ctypes.c_void_p * np_)(*[self._ptrs[fp + j] for j in range(np_)])
            sub_l = (ctypes.c_uint64 * np_)(*[self._lens[fp + j] for j in range(np_)])
            es = dv.eval_points_pointers(sub_p, sub_l, np_, self.points[fk:fk + nk], form, rset.device, self._stream)
            for j, p in enumerate(members):
                for k, shift in enumerate(shifts):
                    at[(p, shift)] = es[j][k]
        self.evals = [at[(p, shift)] for p, shift in queries]
        elems = ctypes.c_uint64(0)
        _lib.check(_lib.lib.sv_bn254_shplonk_work_elems(len(descr), max(self.set_lens, default=0), ctypes.byref(elems)),
                   "sv_bn254_shplonk_work_elems")
        self.work = torch.empty((elems.value, 4), dtype=torch.int64, device=f"cuda:{rset.device}")
        self._gamma = None

    @property
    def _stream(self):
        """The current stream of the polynomials' device, read per call."""
        from . import device as dv
        return dv._stream_handle(self._keep[0].device) if self._keep else None

    def _affine(self, part):
        out = _lib.sv_g1_affine()
        _lib.check(_lib.lib.sv_bn254_g1_fold(ctypes.byref(part), 1, ctypes.byref(out), _lib.SV_CANONICAL),
                   "sv_bn254_g1_fold")
        return enc.g1_from_struct(out)

    def quotient(self, mu: int, gamma: int):
        """W = sum_k h_k set[offset + k] for h = sum_i gamma^i h_i (None = the identity)."""
        if self.rset.handle is None:
            raise _lib.ArgumentError("base set is closed")
        ms, gs, part = enc.fr_struct(mu, self.form), enc.fr_struct(gamma, self.form), _lib.sv_g1_jacobian()
        _lib.check(_lib.lib.sv_bn254_shplonk_quotient_device(
            self.rset.handle, self.offset, self._ptrs, self._lens, len(self._keep), self._sets, len(self.sets),
            self._points, len(self.points), ctypes.byref(ms), ctypes.byref(gs), self.form, self._stream,
            self.work.data_ptr(), self.work.shape[0], ctypes.byref(part)), "sv_bn254_shplonk_quotient_device")
        self._gamma = gamma
        return self._affine(part)

    def witness(self, z_prime: int):
        """W' = the witness of the linearisation L at z' (None = the identity); after quotient()."""
        if self.rset.handle is None:
            raise _lib.ArgumentError("base set is closed")
        if self._gamma is None:
            raise _lib.ArgumentError("witness() needs the work buffer that quotient() fills")
        gs, zs, part = enc.fr_struct(self._gamma, self.form), enc.fr_struct(z_prime, self.form), _lib.sv_g1_jacobian()
        _lib.check(_lib.lib.sv_bn254_shplonk_witness_device(
            self.rset.handle, self.offset, self._sets, len(self.sets), self._points, len(self.points),
            self._set_lens, ctypes.byref(gs), ctypes.byref(zs), self.form, self._stream, self.work.data_ptr(),
            self.work.shape[0], ctypes.byref(part)), "sv_bn254_shplonk_witness_device")
        return self._affine(part)


def bdfg21_open(rset, polys, queries: Sequence[Tuple[int, int]], z: int, challenges, offset: int = 0,
                form: int = _lib.SV_MONTGOMERY) -> Tuple[list, Point, Point]:
    """A SHPLONK opening on a resident base set -> (evaluations in query order, W, W').
    `challenges` is (mu, gamma, z') as canonical ints, or a transcript, driven in the order of
    Bdfg21Proof::read (bdfg21.rs:101-114): squeeze mu, squeeze gamma, absorb W, squeeze z', absorb W'
    (the caller absorbs the evaluations before the call, as its protocol orders them)."""
    op = Bdfg21Opening(rset, polys, queries, z, offset=offset, form=form)
    if isinstance(challenges, (tuple, list)):
        mu, gamma, z_prime = challenges
        w = op.quotient(mu, gamma)
        return op.evals, w, op.witness(z_prime)
    mu = challenges.squeeze_challenge()
    gamma = challenges.squeeze_challenge()
    w = op.quotient(mu, gamma)
    challenges.common_ec_point(w)
    z_prime = challenges.squeeze_challenge()
    w_prime = op.witness(z_prime)
    challenges.common_ec_point(w_prime)
    return op.evals, w, w_prime


def gwc19_open(rset, polys, queries: Sequence[Tuple[int, int]], z: int, v: int, offset: int = 0,
               form: int = _lib.SV_MONTGOMERY) -> Tuple[list, list]:
    """The prover's side of Gwc19::verify (gwc19.rs:43-80) on a resident base set: `polys` are
    (n_j, 4) int64 torch tensors in `form` in HBM on the set's device, `queries` a list of
    (poly index, shift), z and v canonical ints.  Point set i (gwc19_query_sets) is opened at
    shift_i * z with one batched call -- W_i = the witness of sum_j v^j p_ij there -- so the several
    points of an opening cost one MSM each, however many polynomials share a point.
    Returns ([evaluation per query, in query order], [W_i per set])."""
    evals = [None] * len(queries)
    witnesses = []
    for shift, members, where in gwc19_query_sets(queries):
        es, w = rset.open_batch_device([polys[j] for j in members], shift * z % enc.R, v, offset=offset, form=form)
        for qi, e in zip(where, es):
            evals[qi] = e
        witnesses.append(w)
    return evals, witnesses
