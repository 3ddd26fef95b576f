// KZG decider for BN254 on gfx950: for every accumulator i,
//     e(lhs_i, g2) * e(rhs_i, -s_g2) == 1
// Replaces AccumulationDecider::{decide, decide_all} for KzgAs on NativeLoader
// (snark-verifier/src/pcs/kzg/decider.rs:60-80).
//
// The two G2 points are fixed per call, so their Miller-loop line coefficients (88 steps x 3 Fq2
// each, 33.8 KB for both) are computed once on the host (G2Prepared::from, which the reference
// redoes inside every decide, decider.rs:64) and uploaded.  Each accumulator is then decided by a
// group of 6 x S lanes (below): a 2-term multi-Miller loop with sparse 034 line multiplications and
// the exact final exponentiation (the chain of curve.hpp), Fq12 spread one coefficient per 6 lanes.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "curve.hpp"
#include "decider.hpp"
#include "fq12_lanes.hpp"
#include "runtime.hpp"

namespace sv {

__device__ __forceinline__ G1Aff load_aff_d(const G1Aff* __restrict__ a, uint32_t i, int mont_in) {
  const uint4* p = reinterpret_cast<const uint4*>(a + i);
  uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
  G1Aff r;
  r.x.v[0] = q0.x; r.x.v[1] = q0.y; r.x.v[2] = q0.z; r.x.v[3] = q0.w;
  r.x.v[4] = q1.x; r.x.v[5] = q1.y; r.x.v[6] = q1.z; r.x.v[7] = q1.w;
  r.y.v[0] = q2.x; r.y.v[1] = q2.y; r.y.v[2] = q2.z; r.y.v[3] = q2.w;
  r.y.v[4] = q3.x; r.y.v[5] = q3.y; r.y.v[6] = q3.z; r.y.v[7] = q3.w;
  if (!mont_in && !r.is_identity()) {
    r.x = fe_to_mont(r.x);
    r.y = fe_to_mont(r.y);
  }
  return r;
}

// ---------------------------------------------------------------------------------------------
// Lane groups: each accumulator is decided by 6 x S lanes.  Lane (k, s) holds the w^k coefficient
// g_k of the Fq12 accumulator (replicated over its S sub-lanes; fq12_lanes.hpp), and computes the
// products of its coefficient whose index is = s (mod S); the S partial sums are combined with
// cross-lane xor-shuffles, so an Fq12 multiply costs ceil(6/S) Fq2 products of latency, a square
// ceil(4/S), a sparse line step ceil(3/S).  Operands are exchanged through LDS.  Control flow is
// uniform across the wave (identity inputs use the neutral line 1), so the single-wave block can
// use __syncthreads() between the write and read phases of each exchange.
// ---------------------------------------------------------------------------------------------
__constant__ uint32_t c_gamma[3 * 6 * 16] = SV_GAMMA_TAB_INIT;
__constant__ SqrTerm c_sqr[6][4] = SV_SQR_TERMS;
__constant__ int8_t c_naf[ATE_NAF_LEN] = SV_ATE_NAF_INIT;

struct Grp {
  Fq2* a;         // this group's 6 LDS slots for operand A
  Fq2* b;         // ... and operand B
  Fq2* tab;       // kTab x 6 LDS slots: odd powers (and conjugates) for the windowed x-power
  Fq2* keep;      // kKeep x 6 LDS slots: long-lived final-exponentiation values
  int k;          // coefficient index (lanes past 6*S mirror k = 5 and never write)
  int s;          // sub-lane
  bool w;         // writer (s == 0, active)
  SqrTerm sq[4];  // this lane's square terms (slots s, s + S, ...), kept in registers
  SqrTerm sqh;    // S = 8 half-product squaring: term s >> 1 of coefficient k
};

// Cross-lane moves inside 8-lane sub-lane groups by DPP (a VALU operand modifier, no LDS round
// trip like the ds_bpermute behind __shfl_xor): level 1 swaps lane pairs (quad_perm [1,0,3,2]),
// level 2 swaps pairs of pairs (quad_perm [2,3,0,1]); after those every lane of a quad holds the
// quad's sum, so level 3 only needs the other quad of the 8: row_half_mirror (lane i <- 7 - i).
template <int LEVEL>
__device__ __forceinline__ uint32_t dpp_partner(uint32_t x) {
  constexpr int ctrl = LEVEL == 0 ? 0xB1 : (LEVEL == 1 ? 0x4E : 0x141);
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, ctrl, 0xF, 0xF, false);
}

template <int LEVEL>
__device__ __forceinline__ Fq2 dpp_partner(const Fq2& v) {
  Fq2 o;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    o.c0.v[i] = dpp_partner<LEVEL>(v.c0.v[i]);
    o.c1.v[i] = dpp_partner<LEVEL>(v.c1.v[i]);
  }
  return o;
}

template <int S>
__device__ __forceinline__ Fq2 sub_reduce(Fq2 v) {
  // sum over the S consecutive sub-lanes of one coefficient (S = 1, 2, 4, 8; groups 8-aligned)
  static_assert(S == 1 || S == 2 || S == 4 || S == 8, "sub-lane count");
  if constexpr (S >= 2) v = v + dpp_partner<0>(v);
  if constexpr (S >= 4) v = v + dpp_partner<1>(v);
  if constexpr (S >= 8) v = v + dpp_partner<2>(v);
  return v;
}

template <int S>
__device__ __forceinline__ Fq2 g_mul(const Grp& G, const Fq2& x, const Fq2& y) {
  if (G.w) {
    G.a[G.k] = x;
    G.b[G.k] = y;
  }
  __syncthreads();
  Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll
  for (int t = 0; t < (6 + S - 1) / S; t++) {
    const int i = t * S + G.s;
    if (i < 6) {
      const int j = G.k - i;
      const Fq2 p = G.a[i] * G.b[j < 0 ? j + 6 : j];
      if (j >= 0) lo = lo + p;
      else hi = hi + p;
    }
  }
  __syncthreads();
  return sub_reduce<S>(lo + fq2_mul_xi(hi));
}

template <int S>
__device__ __forceinline__ Fq2 g_sqr(const Grp& G, const Fq2& x) {
  if (G.w) G.a[G.k] = x;
  __syncthreads();
  Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll
  for (int t = 0; t < (4 + S - 1) / S; t++) {
    const int slot = t * S + G.s;
    if (slot < 4) {
      const SqrTerm q = G.sq[t];
      if (q.i >= 0) {
        Fq2 p = G.a[q.i] * G.a[q.j];
        if (q.dbl) p = p + p;
        if (q.xi) hi = hi + p;
        else lo = lo + p;
      }
    }
  }
  __syncthreads();
  return sub_reduce<S>(lo + fq2_mul_xi(hi));
}

// f * (l0 + l1 w + l3 w^3)
template <int S>
__device__ __forceinline__ Fq2 g_line(const Grp& G, const Fq2& x, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
  if (G.w) G.a[G.k] = x;
  __syncthreads();
  Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll
  for (int t = 0; t < (3 + S - 1) / S; t++) {
    const int term = t * S + G.s;
    if (term < 3) {
      const int sh = term == 0 ? 0 : (term == 1 ? 1 : 3);
      const int src = G.k - sh;
      const Fq2& l = term == 0 ? l0 : (term == 1 ? l1 : l3);
      const Fq2 p = G.a[src < 0 ? src + 6 : src] * l;
      if (src >= 0) lo = lo + p;
      else hi = hi + p;
    }
  }
  __syncthreads();
  return sub_reduce<S>(lo + fq2_mul_xi(hi));
}

// ---- S = 8 half-product forms: sub-lane s = 2t + h computes component h (0: re, 1: im) of term t
// with two independent Fq products (re(xy) = x0 y0 - x1 y1, im(xy) = x0 y1 + x1 y0) instead of a
// whole Karatsuba Fq2 product (3 dependent-issue products), and its contribution to the
// coefficient: plain (v, 0) / (0, v); wrapped terms carry xi: xi (a + b u) = (9a - b) + (a + 9b) u,
// so a re-lane adds (9v, v) and an im-lane (-v, 9v).  Control flow stays uniform: idle lanes
// compute on slot 0 and contribute zero.
__device__ __forceinline__ Fq fq_mul9(const Fq& a) {
  const Fq a2 = a + a, a4 = a2 + a2;
  return a4 + a4 + a;
}

__device__ __forceinline__ Fq2 half_term(const Fq2& x, const Fq2& y, int h, bool xi, bool live) {
  const Fq m1 = x.c0 * (h ? y.c1 : y.c0);
  const Fq m2 = x.c1 * (h ? y.c0 : y.c1);
  const Fq v = h ? m1 + m2 : fe_sub_lat(m1, m2);
  const Fq v9 = fq_mul9(v);
  Fq cr, ci;
  if (!xi) {
    cr = h ? Fq::zero() : v;
    ci = h ? v : Fq::zero();
  } else {
    cr = h ? -v : v9;
    ci = h ? v9 : v;
  }
  if (!live) cr = ci = Fq::zero();
  return {cr, ci};
}

template <int S>
__device__ __forceinline__ Fq2 g_sqr_h(const Grp& G, const Fq2& x) {
  static_assert(S == 8, "half-product squaring needs 8 sub-lanes");
  if (G.w) G.a[G.k] = x;
  __syncthreads();
  const SqrTerm q = G.sqh;
  const bool live = q.i >= 0;
  const Fq2 X = G.a[live ? q.i : 0], Y = G.a[live ? q.j : 0];
  Fq2 c = half_term(X, Y, G.s & 1, q.xi, live);
  if (q.dbl) c = c + c;
  __syncthreads();
  return sub_reduce<S>(c);
}

// f * (l0 + l1 w + l3 w^3): terms t = 0, 1, 2 take f_k, f_{k-1}, f_{k-3} (wrapping with xi)
template <int S>
__device__ __forceinline__ Fq2 g_line_h(const Grp& G, const Fq2& x, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
  static_assert(S == 8, "half-product line step needs 8 sub-lanes");
  if (G.w) G.a[G.k] = x;
  __syncthreads();
  const int t = G.s >> 1;
  const bool live = t < 3;
  const int sh = t == 0 ? 0 : (t == 1 ? 1 : 3);
  const int src = G.k - sh;
  const Fq2& l = t == 0 ? l0 : (t == 1 ? l1 : l3);
  const Fq2 c = half_term(G.a[live ? (src < 0 ? src + 6 : src) : 0], l, G.s & 1, src < 0, live);
  __syncthreads();
  return sub_reduce<S>(c);
}

__device__ __forceinline__ Fq2 g_conj(const Grp& G, const Fq2& x) { return (G.k & 1) ? -x : x; }
__device__ __forceinline__ Fq2 g_frob(const Grp& G, int n, const Fq2& x) {
  Fq2 y = (n & 1) ? fq2_conj(x) : x;
  if (G.k == 0) return y;
  const uint32_t* t = c_gamma + ((n - 1) * 6 + G.k) * 16;
  Fq2 c;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c.c0.v[i] = t[i];
    c.c1.v[i] = t[8 + i];
  }
  return y * c;
}
// f^-1 = conj(f) N^-1 with N = f conj(f) = a^2 - v b^2 in Fq6 (f = a + b w over Fq6, v = w^2):
// N sits on the even w-coefficients, its Fq6 inverse (t0 + t1 v + t2 v^2) / d is formed with the
// three t_j on the lanes of coefficients 0, 2, 4 in parallel, and only the norm of d in Fq is
// inverted (one fe_inv, on every lane, uniform) -- instead of a whole Fq12 inversion per lane.
template <int S>
__device__ __forceinline__ Fq2 g_inv(const Grp& G, const Fq2& f) {
  const Fq2 fc = g_conj(G, f);
  const Fq2 nk = g_mul<S>(G, f, fc);  // odd coefficients vanish
  if (G.w) G.a[G.k] = nk;
  __syncthreads();
  const Fq2 c0 = G.a[0], c1 = G.a[2], c2 = G.a[4];
  const int j = G.k >> 1;
  // t0 = c0^2 - xi c1 c2, t1 = xi c2^2 - c0 c1, t2 = c1^2 - c0 c2 (lanes of coefficient 2j)
  const Fq2 x = j == 0 ? c0 : (j == 1 ? c2 : c1);
  const Fq2 y0 = j == 0 ? c1 : c0, y1 = j == 0 ? c2 : (j == 1 ? c1 : c2);
  const Fq2 sq = x * x, pr = y0 * y1;
  const Fq2 tj = j == 0 ? sq - fq2_mul_xi(pr) : (j == 1 ? fq2_mul_xi(sq) - pr : sq - pr);
  __syncthreads();
  if (G.w && !(G.k & 1)) G.b[j] = tj;
  __syncthreads();
  const Fq2 t0 = G.b[0], t1 = G.b[1], t2 = G.b[2];
  __syncthreads();
  const Fq2 d = c0 * t0 + fq2_mul_xi(c2 * t1 + c1 * t2);
  const Fq2 di = fq2_inv(d);
  const Fq2 ninv = (G.k & 1) ? Fq2::zero() : (j == 0 ? t0 : (j == 1 ? t1 : t2)) * di;
  return g_mul<S>(G, fc, ninv);
}
// Squaring / line steps: the half-product forms at S = 8, the whole-product forms otherwise
// (measured per op on one wave, tools/ubench_decops.hip: g_sqr 4.8 us, g_sqr_h 3.2 us; a Granger-Scott
// cyclotomic squaring with one product level measured 6.1 us -- single-wave code is bound by
// dependent-instruction latency, and its many Fq2 additions cost more than the products it saves)
template <int S>
__device__ __forceinline__ Fq2 g_msq(const Grp& G, const Fq2& x) {
  if constexpr (S == 8) return g_sqr_h<S>(G, x);
  else return g_sqr<S>(G, x);
}
template <int S>
__device__ __forceinline__ Fq2 g_mline(const Grp& G, const Fq2& x, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
  if constexpr (S == 8) return g_line_h<S>(G, x, l0, l1, l3);
  else return g_line<S>(G, x, l0, l1, l3);
}

// f * y with y's six coefficients already in LDS (yb[0..5]): no operand write on the critical path
template <int S>
__device__ __forceinline__ Fq2 g_mul_lds(const Grp& G, const Fq2& x, const Fq2* yb) {
  if (G.w) G.a[G.k] = x;
  __syncthreads();
  Fq2 lo = Fq2::zero(), hi = Fq2::zero();
#pragma unroll
  for (int t = 0; t < (6 + S - 1) / S; t++) {
    const int i = t * S + G.s;
    if (i < 6) {
      const int j = G.k - i;
      const Fq2 p = G.a[i] * yb[j < 0 ? j + 6 : j];
      if (j >= 0) lo = lo + p;
      else hi = hi + p;
    }
  }
  __syncthreads();
  return sub_reduce<S>(lo + fq2_mul_xi(hi));
}

__device__ __forceinline__ void g_put(const Grp& G, Fq2* slots, int e, const Fq2& v) {
  if (G.w) slots[e * 6 + G.k] = v;
}
__device__ __forceinline__ Fq2 g_get(const Grp& G, const Fq2* slots, int e) { return slots[e * 6 + G.k]; }

// x = 0x44e992b44a6909f1 in width-4 NAF (odd digits in [-7, 7], 14 non-zero of 63): 62 squarings
// and 13 multiplications by a tabulated odd power instead of 27 for plain binary.  Negative digits
// multiply by the conjugate, which is the inverse on the cyclotomic subgroup the hard part of the
// final exponentiation works in.
struct XNaf {
  int8_t d[66];
  int len;
};
constexpr XNaf make_xnaf() {
  XNaf r{};
  uint64_t k = BN_X;
  int i = 0;
  while (k) {
    int v = 0;
    if (k & 1) {
      v = (int)(k & 15);
      if (v >= 8) v -= 16;
      k = v >= 0 ? k - (uint64_t)v : k + (uint64_t)(-v);
    }
    r.d[i++] = (int8_t)v;
    k >>= 1;
  }
  r.len = i;
  return r;
}
__constant__ XNaf c_xnaf = make_xnaf();
static constexpr int kTab = 8;   // a, a^3, a^5, a^7, then their conjugates
static constexpr int kKeep = 6;

template <int S>
__device__ __forceinline__ Fq2 g_pow_x(const Grp& G, const Fq2& a) {
  const Fq2 a2 = g_msq<S>(G, a);
  g_put(G, G.tab, 0, a);
  g_put(G, G.tab, 4, g_conj(G, a));
  Fq2 ak = a;
  for (int e = 1; e < 4; e++) {
    ak = g_mul<S>(G, ak, a2);
    g_put(G, G.tab, e, ak);
    g_put(G, G.tab, 4 + e, g_conj(G, ak));
  }
  __syncthreads();  // the last table entries are read below without an intervening exchange
  const int len = c_xnaf.len;
  const int top = c_xnaf.d[len - 1];
  Fq2 r = g_get(G, G.tab, top > 0 ? (top - 1) / 2 : 4 + (-top - 1) / 2);
  for (int i = len - 2; i >= 0; i--) {
    r = g_msq<S>(G, r);
    const int d = c_xnaf.d[i];
    if (d) r = g_mul_lds<S>(G, r, G.tab + 6 * (d > 0 ? (d - 1) / 2 : 4 + (-d - 1) / 2));
  }
  return r;
}

// Prologue: the group's lanes evaluate all 2 x ATE_NUM_LINES lines at their accumulator's points
// into LDS (l0 = c0 yP, l1 = c3 xP, l3 = c4; the neutral line 1 when P is the identity), so the
// Miller loop's line steps do no global loads and no line arithmetic on the critical path.
__device__ __forceinline__ void eval_lines(LineCoeff* __restrict__ E, const LineCoeff* __restrict__ L1,
                                           const LineCoeff* __restrict__ L2, const G1Aff& p1, const G1Aff& p2,
                                           int lane_in_group, int group_lanes) {
  for (int it = lane_in_group; it < 2 * ATE_NUM_LINES; it += group_lanes) {
    const int idx = it >> 1;
    const bool second = it & 1;
    const G1Aff& p = second ? p2 : p1;
    LineCoeff out;
    if (!p.is_identity()) {
      const LineCoeff c = (second ? L2 : L1)[idx];
      out.c0 = c.c0 * p.y;
      out.c3 = c.c3 * p.x;
      out.c4 = c.c4;
    } else {
      out.c0 = Fq2::one();
      out.c3 = Fq2::zero();
      out.c4 = Fq2::zero();
    }
    E[it] = out;
  }
}

// ---- Step multipliers (S = 8 path): the Miller loop's line products are known once the lines are
// evaluated, so the prologue folds them off the critical path.  Pair idx (the lines of both G2
// points at one step) becomes the 5-sparse D_idx = (a0 + a1 w + a3 w^3)(b0 + b1 w + b3 w^3), and a
// step with an addition (or the final Frobenius steps) multiplies its two pairs into a dense M.
// The loop then costs one square and ONE multiplication per step (66) instead of a square and
// 2-4 sparse line steps (176).
struct MergeTab {
  int8_t first[32];  // first pair index of each merged step (the second is first + 1)
  int n;
};
constexpr MergeTab make_merges() {
  MergeTab t{};
  int idx = 0, m = 0;
  for (int i = ATE_NAF_LEN - 1; i >= 1; i--) {
    if (ATE_NAF[i - 1] != 0) {
      t.first[m++] = (int8_t)idx;
      idx += 2;
    } else {
      idx += 1;
    }
  }
  t.first[m++] = (int8_t)idx;  // the two Frobenius steps
  t.n = m;
  return t;
}
__constant__ MergeTab c_merge = make_merges();
static constexpr int kMaxMerge = 32;

// D_idx for pairs idx = lane, lane + lanes, ...: 6 Fq2 products (Karatsuba on the three cross terms)
__device__ __forceinline__ void pair_products(Fq2* __restrict__ D, const LineCoeff* __restrict__ E, int lane,
                                              int lanes) {
  for (int idx = lane; idx < ATE_NUM_LINES; idx += lanes) {
    const LineCoeff A = E[2 * idx], Bq = E[2 * idx + 1];
    const Fq2 m00 = A.c0 * Bq.c0, m11 = A.c3 * Bq.c3, m33 = A.c4 * Bq.c4;
    const Fq2 x01 = (A.c0 + A.c3) * (Bq.c0 + Bq.c3);
    const Fq2 x03 = (A.c0 + A.c4) * (Bq.c0 + Bq.c4);
    const Fq2 x13 = (A.c3 + A.c4) * (Bq.c3 + Bq.c4);
    Fq2* d = D + 6 * idx;
    d[0] = m00 + fq2_mul_xi(m33);
    d[1] = x01 - m00 - m11;
    d[2] = m11;
    d[3] = x03 - m00 - m33;
    d[4] = x13 - m11 - m33;
    d[5] = Fq2::zero();
  }
}

// M_m = D_a D_{a+1} (both 5-sparse) for every merged step; job = (step, output coefficient)
__device__ __forceinline__ void merge_products(Fq2* __restrict__ M, const Fq2* __restrict__ D, int lane, int lanes) {
  for (int job = lane; job < c_merge.n * 6; job += lanes) {
    const int m = job / 6, k = job % 6;
    const Fq2* a = D + 6 * c_merge.first[m];
    const Fq2* b = a + 6;
    Fq2 lo = Fq2::zero(), hi = Fq2::zero();
    for (int i = 0; i < 5; i++) {
      const int j = k - i;
      if (j >= 0 && j < 5) lo = lo + a[i] * b[j];
      const int jw = k + 6 - i;
      if (jw >= 0 && jw < 5) hi = hi + a[i] * b[jw];
    }
    M[6 * m + k] = lo + fq2_mul_xi(hi);
  }
}

// Round 3 (k_decide_wg): the pair products D_idx from per-key constants.  With A = (c0 y1, c3 x1, c4)
// and B = (c0' y2, c3' x2, c4') the line values at the accumulator's points, every coefficient of
// D = A B is a sum of (product of two line coefficients: the key's) x (product of point coordinates:
// the accumulator's) --
//   d0 = (c0 c0') y1 y2 + xi c4 c4',  d1 = (c0 c3') y1 x2 + (c3 c0') x1 y2,  d2 = (c3 c3') x1 x2,
//   d3 = (c0 c4') y1 + (c4 c0') y2,    d4 = (c3 c4') x1 + (c4 c3') x2,        d5 = 0
// -- so the nine key products per step (kKc, computed once per deciding key on the host) leave one
// fused two-product sum per Fq component: 880 independent jobs over the block instead of the line
// evaluation (4 products per line) and a 6-product Karatsuba per pair (18 Fq products deep).
// Identity points keep eval_lines + pair_products (the neutral line is not of this form).
constexpr int kKc = 9;  // c0c0', c3c3', xi c4c4', c0c3', c3c0', c0c4', c4c0', c3c4', c4c3'
__device__ __forceinline__ void pair_products_kc(Fq2* __restrict__ D, const Fq2* __restrict__ kc, const Fq* sc,
                                                 const G1Aff& p1, const G1Aff& p2, int t, int nt) {
  // sc: y1 y2, x1 x2, y1 x2, x1 y2 (LDS)
  for (int job = t; job < ATE_NUM_LINES * 10; job += nt) {
    const int idx = job / 10, r = job % 10, k = r >> 1, comp = r & 1;
    const Fq2* K = kc + kKc * idx;
    const int ja = k == 0 ? 0 : (k == 1 ? 3 : (k == 2 ? 1 : (k == 3 ? 5 : 7)));
    const Fq2 ka = K[ja];
    const Fq2 kb = K[k == 1 ? 4 : (k == 3 ? 6 : (k == 4 ? 8 : 2))];  // second term (k = 0: xi c4c4')
    const bool two = k == 1 || k >= 3;
    const Fq sa = k == 0 ? sc[0] : (k == 1 ? sc[2] : (k == 2 ? sc[1] : (k == 3 ? p1.y : p1.x)));
    const Fq sb = k == 1 ? sc[3] : (k == 3 ? p2.y : p2.x);
    const Fq x[2] = {comp ? ka.c1 : ka.c0, two ? (comp ? kb.c1 : kb.c0) : Fq::zero()};
    const Fq y[2] = {sa, two ? sb : Fq::zero()};
    Fq v = fe_mul_sum(x, y);
    if (k == 0) v = v + (comp ? kb.c1 : kb.c0);
    Fq2& d = D[6 * idx + k];
    if (comp) d.c1 = v;
    else d.c0 = v;
  }
  for (int idx = t; idx < ATE_NUM_LINES; idx += nt) D[6 * idx + 5] = Fq2::zero();
}

// the nine key products of kKc per step (host, once per deciding key): lines L1 (g2), L2 (-s_g2)
static void pair_constants(const LineCoeff* L1, const LineCoeff* L2, Fq2* kc) {
  for (int i = 0; i < ATE_NUM_LINES; i++) {
    const LineCoeff& a = L1[i];
    const LineCoeff& b = L2[i];
    Fq2* K = kc + kKc * i;
    K[0] = a.c0 * b.c0;
    K[1] = a.c3 * b.c3;
    K[2] = fq2_mul_xi(a.c4 * b.c4);
    K[3] = a.c0 * b.c3;
    K[4] = a.c3 * b.c0;
    K[5] = a.c0 * b.c4;
    K[6] = a.c4 * b.c0;
    K[7] = a.c3 * b.c4;
    K[8] = a.c4 * b.c3;
  }
}

template <int S>
__global__ void __launch_bounds__(64) k_decide_lanes(const G1Aff* __restrict__ lhs, const G1Aff* __restrict__ rhs,
                                                      uint32_t n, const LineCoeff* __restrict__ L1,
                                                      const LineCoeff* __restrict__ L2, int mont_in,
                                                      int32_t* __restrict__ verdict, Fq12* __restrict__ gt,
                                                      int phases) {
  constexpr int GL = 8 * S;         // lanes per group (6 * S active)
  constexpr int NGRP = 64 / GL;     // groups per single-wave block
  __shared__ Fq2 sh[2 * NGRP * 6];
  __shared__ LineCoeff ev[NGRP][2 * ATE_NUM_LINES];
  __shared__ Fq2 tabk[NGRP][(kTab + kKeep) * 6];
  constexpr bool kMerged = S == 8;  // one group per wave: room for the step multipliers in LDS
  __shared__ Fq2 dmul[kMerged ? ATE_NUM_LINES * 6 : 1];
  const int lane = threadIdx.x, grp = lane / GL, gl = lane % GL;
  const bool active = gl < 6 * S;
  const int k = active ? gl / S : 5, sub = active ? gl % S : 0;
  const uint32_t acc = blockIdx.x * NGRP + grp;
  Grp G{sh + grp * 12, sh + grp * 12 + 6, tabk[grp], tabk[grp] + kTab * 6, k, sub, active && sub == 0, {}, {}};
  G.sqh = (S == 8 && active) ? c_sqr[k][sub >> 1] : SqrTerm{-1, -1, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int slot = t * S + sub;
    G.sq[t] = slot < 4 ? c_sqr[k][slot] : SqrTerm{-1, -1, 0, 0};
  }
  const bool valid = acc < n;
  G1Aff p1 = {Fq::zero(), Fq::zero()}, p2 = p1;
  if (valid) {
    p1 = load_aff_d(lhs, acc, mont_in);
    p2 = load_aff_d(rhs, acc, mont_in);
  }
  eval_lines(ev[grp], L1, L2, p1, p2, gl, GL);
  __syncthreads();
  const LineCoeff* E = ev[grp];
  Fq2 f = G.k == 0 ? Fq2::one() : Fq2::zero();
  int idx = 0;
  if constexpr (kMerged) {
    pair_products(dmul, E, gl, GL);
    __syncthreads();
    Fq2* M = reinterpret_cast<Fq2*>(ev[grp]);  // the evaluated lines are dead now
    static_assert(sizeof(ev[0]) >= kMaxMerge * 6 * sizeof(Fq2), "merged steps must fit the line buffer");
    merge_products(M, dmul, gl, GL);
    __syncthreads();
    int m = 0;
    for (int i = ATE_NAF_LEN - 1; i >= 1 && (phases & 1); i--) {
      const Fq2* mul = c_naf[i - 1] != 0 ? M + 6 * m++ : dmul + 6 * idx;
      idx += c_naf[i - 1] != 0 ? 2 : 1;
      if (i == ATE_NAF_LEN - 1) f = mul[G.k];  // f = 1 * mul
      else f = g_mul_lds<S>(G, g_msq<S>(G, f), mul);
    }
    if (phases & 1) f = g_mul_lds<S>(G, f, M + 6 * m);  // the two Frobenius steps
  } else {
    for (int i = ATE_NAF_LEN - 1; i >= 1 && (phases & 1); i--) {
      if (i != ATE_NAF_LEN - 1) f = g_msq<S>(G, f);
      f = g_mline<S>(G, f, E[2 * idx].c0, E[2 * idx].c3, E[2 * idx].c4);
      f = g_mline<S>(G, f, E[2 * idx + 1].c0, E[2 * idx + 1].c3, E[2 * idx + 1].c4);
      idx++;
      if (c_naf[i - 1] != 0) {
        f = g_mline<S>(G, f, E[2 * idx].c0, E[2 * idx].c3, E[2 * idx].c4);
        f = g_mline<S>(G, f, E[2 * idx + 1].c0, E[2 * idx + 1].c3, E[2 * idx + 1].c4);
        idx++;
      }
    }
    for (int st = 0; st < 2 && (phases & 1); st++) {
      f = g_mline<S>(G, f, E[2 * idx].c0, E[2 * idx].c3, E[2 * idx].c4);
      f = g_mline<S>(G, f, E[2 * idx + 1].c0, E[2 * idx + 1].c3, E[2 * idx + 1].c4);
      idx++;
    }
  }
  // final exponentiation (same chain as curve.hpp final_exponentiation)
  // (phases: debug/profiling knob SVGPU_DECIDER_PHASES, 3 = both halves; results are only valid at 3)
  // inversion-free: the easy part stays the fraction conj(w) / w (see make_wprog below), so this
  // chain computes W with result conj(W) / W
  Fq2 e = f;
  if (phases & 2) {
  f = g_mul<S>(G, g_frob(G, 2, f), f);
  // hard part: f^(l0 + l1 p + l2 p^2 + p^3) with the x-power chain; the small powers of fx and
  // fx^2 share their ladders (fx^6 -> fx^12 -> fx^18, fx2^6 -> fx2^12 -> fx2^18 -> fx2^30)
  enum { K_F, K_B12, K_B18, K_A6, K_A18, K_A30 };
  g_put(G, G.keep, K_F, f);
  const Fq2 fx = g_pow_x<S>(G, f);
  {
    const Fq2 b6 = g_msq<S>(G, g_mul<S>(G, g_msq<S>(G, fx), fx));
    const Fq2 b12 = g_msq<S>(G, b6);
    g_put(G, G.keep, K_B12, b12);
    g_put(G, G.keep, K_B18, g_mul<S>(G, b12, b6));
  }
  const Fq2 fx2 = g_pow_x<S>(G, fx);
  {
    const Fq2 a6 = g_msq<S>(G, g_mul<S>(G, g_msq<S>(G, fx2), fx2));
    const Fq2 a12 = g_msq<S>(G, a6);
    const Fq2 a18 = g_mul<S>(G, a12, a6);
    g_put(G, G.keep, K_A6, a6);
    g_put(G, G.keep, K_A18, a18);
    g_put(G, G.keep, K_A30, g_mul<S>(G, a18, a12));
  }
  const Fq2 fx3 = g_pow_x<S>(G, fx2);
  Fq2 y = g_msq<S>(G, g_msq<S>(G, g_msq<S>(G, fx3)));        // fx3^8
  const Fq2 y36 = g_msq<S>(G, g_msq<S>(G, g_mul<S>(G, y, fx3)));  // fx3^36
  f = g_get(G, G.keep, K_F);
  const Fq2 l2v = g_mul_lds<S>(G, f, G.keep + 6 * K_A6);
  Fq2 t = g_mul_lds<S>(G, g_mul_lds<S>(G, y36, G.keep + 6 * K_A18), G.keep + 6 * K_B12);
  const Fq2 l1v = g_mul_lds<S>(G, g_conj(G, t), G.keep + 6 * K_F);
  t = g_mul_lds<S>(G, g_mul_lds<S>(G, y36, G.keep + 6 * K_A30), G.keep + 6 * K_B18);
  t = g_mul<S>(G, t, g_msq<S>(G, f));
  const Fq2 l0v = g_conj(G, t);
  e = g_mul<S>(G, g_mul<S>(G, g_mul<S>(G, l0v, g_frob(G, 1, l1v)), g_frob(G, 2, l2v)), g_frob(G, 3, f));
  }
  const bool one_k = (G.k & 1) ? e.is_zero() : true;  // conj(W) == W
  if (gt && (phases & 2)) e = g_mul<S>(G, g_conj(G, e), g_inv<S>(G, e));  // the Gt value conj(W) / W
  const uint64_t bal = __ballot(one_k || !active);
  const uint64_t gmask = GL == 64 ? ~0ull : ((1ull << GL) - 1);
  const bool ok = ((bal >> (grp * GL)) & gmask) == gmask;
  if (valid && G.w) {
    if (G.k == 0) verdict[acc] = ok ? 1 : 0;
    if (gt) {
      Fq2* dst = reinterpret_cast<Fq2*>(gt + acc) + (G.k & 1) * 3 + (G.k >> 1);
      *dst = e;
    }
  }
}

// =============================================================================================
// Workgroup decider (default): one block per accumulator -- 512 threads since round 5, two waves per
// SIMD of a CU (the Fq12 operations below use waves 0-2; the prologue's independent jobs use all
// eight, and a second wave on a SIMD issues at the full single-wave rate: tools/ubench_issue.hip).
// The single-wave kernel above keeps one SIMD busy per accumulator, so 256 accumulators leave three
// quarters of the chip's 1024 SIMDs idle, and each of its lanes runs two or three dependent Fq
// products per Fq12 operation (~0.65 us each on one wave).  Here every Fq12
// operation spreads its Fq products over the block, ONE product per lane:
//   w_mul   144 lanes (6 output coefficients x 6 terms x 4 schoolbook Fq2 partial products),
//   w_sqr    96 lanes (6 coefficients x <= 4 pair terms x <= 4 partial products),
//   w_frob   24 lanes (6 coefficients x 4),
// each lane scales its product by its place in the result (the w^6 = xi wrap multiplies by 9 + u),
// and a coefficient's lanes add up with cross-lane moves (a reduce-scatter of DPP moves and one
// ds_swizzle for the 32-lane level, lane_sum) -- no LDS round trip inside an operation.  Operands
// and results live in LDS slots of 6 Fq2 (the w-basis of fq12_lanes.hpp); an operation never
// writes a slot it reads (one barrier per operation).  The Miller loop (merged step multipliers)
// and the inversion-free final exponentiation are one straight-line program over the slots
// (make_wprog), run by an interpreter loop so each operation's code exists once.
// =============================================================================================
#ifndef SV_WG_FN
#define SV_WG_FN __device__ __forceinline__
#endif
namespace wg {
#ifndef SV_WG_THREADS
#define SV_WG_THREADS 512
#endif
constexpr int kThreads = SV_WG_THREADS;  // two waves per SIMD: the prologue jobs run at twice the issue rate

template <int L>
__device__ __forceinline__ uint32_t xmove(uint32_t x) {
  if constexpr (L == 0) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);   // lane ^ 1
  else if constexpr (L == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, false);  // lane ^ 2
  else if constexpr (L == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xF, 0xF, false);  // 7 - i in 8
  else if constexpr (L == 3) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xF, 0xF, false);  // 15 - i in 16
  else if constexpr (L == 5) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x124, 0xF, 0xF, false);  // row_ror 4
  else if constexpr (L == 6) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x128, 0xF, 0xF, false);  // row_ror 8
  else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x401F);  // lane ^ 16 (bit mode, within 32)
}
// 16-B LDS accesses of a 32-B field element (slots, D, M and the gamma table are 32-B aligned)
__device__ __forceinline__ Fq ld_fq(const Fq* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 x = q[0], y = q[1];
  Fq r;
  r.v[0] = x.x, r.v[1] = x.y, r.v[2] = x.z, r.v[3] = x.w;
  r.v[4] = y.x, r.v[5] = y.y, r.v[6] = y.z, r.v[7] = y.w;
  return r;
}
__device__ __forceinline__ void st_fq(Fq* p, const Fq& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  q[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}
// Lazily reduced sums: a lane's contribution and the cross-lane partial sums are plain 9-limb
// integers, reduced mod p ONCE per coefficient (lane products and slot values lie in [0, 2p), so a
// w_mul coefficient sums at most 6 terms x 40 p and a w_sqr one 4 x 80 p: below 330 p < 2^263) -- a
// cross-lane level then costs one 9-limb carry chain instead of a modular addition, and the xi
// factor 9 is a shift and an add.
struct Lz {
  uint32_t v[9];
};
__device__ __forceinline__ Lz lz(const Fq& a) {
  Lz r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = a.v[i];
  r.v[8] = 0;
  return r;
}
__device__ __forceinline__ Lz lz_zero() {
  Lz r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = 0;
  return r;
}
__device__ __forceinline__ Lz lz_add(const Lz& a, const Lz& b) {
  Lz r;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = __builtin_addc(a.v[i], b.v[i], c, &c);
  return r;
}
__device__ __forceinline__ Lz lz_mul9(const Lz& a) {  // (a << 3) + a
  Lz s;
  s.v[0] = a.v[0] << 3;
#pragma unroll
  for (int i = 1; i < 9; i++) s.v[i] = __builtin_amdgcn_alignbit(a.v[i], a.v[i - 1], 29);
  return lz_add(s, a);
}
// a mod p for a < 2^264, to [0, 2p): k = floor(a / p) from the top 40 bits (exact in double; never
// above the true quotient, at most one below), a - k p.  Slots hold such partially reduced values:
// the Montgomery product is exact for inputs below 2p (4 p^2 < 2^256 p) and returns them reduced.
// (tests/test_gpu_decider_ops.py runs this on every multiple of p up to 2^264 - 1 and its
// neighbours, next to every multiple of 2^256, and next to the multiples of 2^224 at which the
// estimate steps -- a >> 224 = j (p_top + 1) -- with the low words all zeros and all ones)
__device__ __forceinline__ Fq lz_reduce(const Lz& a) {
  const uint64_t hi = ((uint64_t)a.v[8] << 32) | a.v[7];  // a >> 224
  // times 1 / (p_top + 1) instead of a division: the product stays below a / p (the divisor's
  // rounding up outweighs the multiply's rounding error), so k is still floor(a / p) or one less
  constexpr double kInvPtop = 1.0 / (double)(FQ_P[7] + 1ull);
  const uint32_t k = (uint32_t)((double)hi * kInvPtop);
  uint32_t r[9];
  uint32_t br = 0;
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t kp = (uint64_t)k * FQ_P[i] + carry;  // v_mad_u64_u32
    carry = kp >> 32;
    r[i] = __builtin_subc(a.v[i], (uint32_t)kp, br, &br);
  }
  Fq t;
#pragma unroll
  for (int i = 0; i < 8; i++) t.v[i] = r[i];
  return t;
}
// [0, 2p) -> fully reduced
__device__ __forceinline__ Fq fq_canon(const Fq& a) {
  Fq d;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d.v[i] = __builtin_subc(a.v[i], FQ_P[i], br, &br);
  return br ? a : d;
}
__device__ __forceinline__ Fq2 fq2_canon(const Fq2& a) { return {fq_canon(a.c0), fq_canon(a.c1)}; }
// the negation of a partially reduced value, again in [0, 2p): 2p - a for a in (0, 2p], and 0 for
// a raw 0 (2p - 0 would leave the slot range)
__device__ __forceinline__ Fq fq_neg2p(const Fq& a) {
  static constexpr uint32_t P2[8] = {0xb0f9fa8eu, 0x7841182du, 0xd0e3951au, 0x2f02d522u,
                                     0x0302b0bbu, 0x70a08b6du, 0xc2634053u, 0x60c89ce5u};
  Fq r;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = __builtin_subc(P2[i], a.v[i], br, &br);
  return a.is_zero() ? a : r;
}
template <int L>
__device__ __forceinline__ Lz xmove(const Lz& a) {
  Lz r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = xmove<L>(a.v[i]);
  return r;
}
// (re, im) summed over aligned groups of 2^LEVELS lanes as a reduce-scatter: the first level
// trades halves with the neighbour lane, so even lanes carry re and odd lanes im from then on and
// every later level moves and adds ONE 9-limb value (not two).  The later levels pair lanes of
// equal parity: lane ^ 2, then row rotations by 4 and 8 (within a 16-lane row), then lane ^ 16.
// Every even (odd) lane of a group ends with the group's re (im) sum.
template <int LEVELS>
__device__ __forceinline__ Lz lane_sum(const Lz& re, const Lz& im) {
  static_assert(LEVELS == 1 || LEVELS == 2 || LEVELS == 4 || LEVELS == 5, "row rotations need 16-lane groups");
  const bool odd = threadIdx.x & 1;
  Lz keep, send;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    keep.v[i] = odd ? im.v[i] : re.v[i];
    send.v[i] = odd ? re.v[i] : im.v[i];
  }
  Lz v = lz_add(keep, xmove<0>(send));
  if constexpr (LEVELS > 1) v = lz_add(v, xmove<1>(v));
  if constexpr (LEVELS > 2) v = lz_add(v, xmove<5>(v));
  if constexpr (LEVELS > 3) v = lz_add(v, xmove<6>(v));
  // (lane ^ 16 by v_permlane16_swap instead of ds_swizzle measured the same: 3611 vs 3554 cycles;
  // folding the moves into v_addc_co_u32_dpp chains was slower, 0.670 -> 0.679 ms: back-to-back
  // v_addc need s_nop 1 between them, which the interleaved v_mov_dpp otherwise fill)
  if constexpr (LEVELS > 4) v = lz_add(v, xmove<4>(v));
  return v;
}

// (the 9-limb carry form above is the round-4 lane sum, kept for tools/ubench_wg.hip's op A/B)
// a lane's contribution l (a reduced v, doubled or not) placed in a coefficient: a real-part term
// (l, 0) or an imaginary one (0, l); wrapped terms (index sum >= 6) carry xi = 9 + u:
// (l, 0) -> (9l, l), (0, l) -> (-l, 9l) with -l from the negated reduced value nv
__device__ __forceinline__ void place(const Lz& l, const Lz& nl, bool imag, bool wrap, Lz& re, Lz& im) {
  if (!wrap) {
    re = imag ? lz_zero() : l;
    im = imag ? l : lz_zero();
  } else {
    const Lz l9 = lz_mul9(l);
    re = imag ? nl : l9;
    im = imag ? l9 : l;
  }
}

// ---- Round 5: lane sums in 24-bit signed limbs.  A lane's contribution to its coefficient's
// (re, im) is (m_re v, m_im v) for its product v in [0, 2p) and small signed integers fixed by the
// lane's role (the sign of a1 b1 in the real part, the 2 of a cross term, the xi = 9 + u wrap, 0
// for an idle lane: WLane), so the placement is a multiply per limb instead of negations, doublings
// and selects.  v splits into 11 limbs of 24 bits (one v_perm_b32 each).  Over one coefficient the
// |m| sum to at most 102 (positive ones to 97, negative ones to 56, w_mul and w_sqr alike), and
// 102 * 2^24 < 2^31, so every partial sum stays an int32 per limb and a level of the lane sum is
// ONE v_add_u32 per limb with the partner's limb read through DPP: no carry chain, whose VCC
// hazards cost an s_nop per dependent v_addc.  The coefficient sum lies in (-112 p, 194 p); w_mul's
// conj flags negate whole terms, which raises the negative figure to 59 (kConjA or kConjB) or 80
// (both) with the positive one still within 97: (-160 p, 194 p).  Biased by 240 p the sum is
// positive and below 434 p < 2^263, and one signed carry pass normalises it into the 9-word Lz
// form that lz_reduce takes.  (tests/test_gpu_decider_ops.py restates the multiplier table and
// confirms these figures.)
constexpr int kL24 = 11;  // 11 x 24 = 264 bits
struct Limbs24 {
  uint32_t v[kL24];
};
constexpr Limbs24 make_bias24() {  // 240 p in 24-bit limbs
  uint32_t w[9] = {};
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t x = (uint64_t)FQ_P[i] * 240u + c;
    w[i] = (uint32_t)x;
    c = x >> 32;
  }
  w[8] = (uint32_t)c;
  Limbs24 b{};
  for (int i = 0; i < kL24; i++) {
    const int wi = 24 * i / 32, o = 24 * i % 32;
    const uint64_t x = (uint64_t)w[wi] | (wi + 1 < 9 ? (uint64_t)w[wi + 1] << 32 : 0);
    b.v[i] = (uint32_t)(x >> o) & 0xFFFFFFu;
  }
  return b;
}
constexpr Limbs24 kBias24 = make_bias24();
static_assert(kBias24.v[kL24 - 1] < (1u << 22), "240 p < 2^262");
// byte B of a 256-bit value is byte B % 4 of word B / 4; limb i = bytes 3i .. 3i + 2
__device__ __forceinline__ void split24(const Fq& a, uint32_t l[kL24]) {
#pragma unroll
  for (int i = 0; i < kL24; i++) {
    const int w = 3 * i / 4, o = 3 * i % 4;
    const uint32_t lo = a.v[w], hi = w + 1 < 8 ? a.v[w + 1] : 0u;
    // selector bytes 0-3 pick from lo, 4-7 from hi, 0x0C gives zero
    const uint32_t sel = (uint32_t)o | (uint32_t)(o + 1) << 8 | (uint32_t)(o + 2) << 16 | 0x0C000000u;
    l[i] = __builtin_amdgcn_perm(hi, lo, sel);
  }
}
// biased signed-limb sum -> 9 words: carries t_i >> 24 (arithmetic); word j = bytes 4j .. 4j + 3
// gathered from the low three bytes of two adjacent t (v_perm_b32); the top word takes all of t_10
// above bit 16 (the biased sum is non-negative).  Tested over the whole of (-112 p, 194 p): every
// multiple of p and its neighbours, both ends, and limbs at +-102 (2^24 - 1) in runs and alternating
__device__ __forceinline__ Lz norm24(const uint32_t s[kL24]) {
  uint32_t t[kL24];
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < kL24; i++) {
    t[i] = s[i] + kBias24.v[i] + (uint32_t)c;
    c = (int32_t)t[i] >> 24;
  }
  Lz r;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int l0 = 4 * j / 3;
    uint32_t sel = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int B = 4 * j + k, li = B / 3, pos = B % 3;
      sel |= (uint32_t)(li == l0 ? pos : 4 + pos) << (8 * k);
    }
    r.v[j] = __builtin_amdgcn_perm(t[l0 + 1], t[l0], sel);
  }
  r.v[8] = t[kL24 - 1] >> 16;
  return r;
}
// the coefficient sum of m_keep v over the lanes of an aligned group of 2^LEVELS lanes, as the
// reduce-scatter of lane_sum: level 1 adds the neighbour's m_send v, so even lanes carry re and odd
// lanes im; later levels pair lanes of equal parity (lane ^ 2, row rotations by 4 and 8, lane ^ 16)
// x + (x of the partner lane L): the move written as update_dpp with a zero "old" and bound_ctrl
// so the compiler folds it into the add (v_add_u32_dpp); the swizzle level stays a move + add
template <int L>
__device__ __forceinline__ uint32_t add_x(uint32_t acc, uint32_t x) {
  constexpr int ctrl = L == 0 ? 0xB1 : L == 1 ? 0x4E : L == 5 ? 0x124 : L == 6 ? 0x128 : -1;
  if constexpr (ctrl < 0) return acc + xmove<L>(x);
  else return acc + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, 0xF, 0xF, true);
}
template <int LEVELS>
__device__ __forceinline__ Lz lane_sum24(const Fq& v, uint32_t m_keep, uint32_t m_send) {
  static_assert(LEVELS == 2 || LEVELS == 4 || LEVELS == 5, "row rotations need 16-lane groups");
  uint32_t l[kL24], x[kL24];
  split24(v, l);
#pragma unroll
  for (int i = 0; i < kL24; i++) x[i] = add_x<0>(m_keep * l[i], m_send * l[i]);
#pragma unroll
  for (int i = 0; i < kL24; i++) x[i] = add_x<1>(x[i], x[i]);
  if constexpr (LEVELS > 2) {
#pragma unroll
    for (int i = 0; i < kL24; i++) x[i] = add_x<5>(x[i], x[i]);
#pragma unroll
    for (int i = 0; i < kL24; i++) x[i] = add_x<6>(x[i], x[i]);
  }
  if constexpr (LEVELS > 4) {
#pragma unroll
    for (int i = 0; i < kL24; i++) x[i] = add_x<4>(x[i], x[i]);
  }
  return norm24(x);
}
// a lane's (keep, send) multipliers from its (re, im) ones: the xi wrap (r, i) -> (9r - i, r + 9i),
// even lanes keep re, odd lanes im
__device__ __forceinline__ void keep_send(int re, int im, bool wrap, uint32_t& keep, uint32_t& send) {
  if (wrap) {
    const int r = 9 * re - im, i = re + 9 * im;
    re = r;
    im = i;
  }
  const bool odd = threadIdx.x & 1;
  keep = (uint32_t)(odd ? im : re);
  send = (uint32_t)(odd ? re : im);
}

// Per-lane roles of w_mul / w_sqr, fixed for the whole program (computed once, kept in registers:
// the square-term table lookup was a per-operation vector load on the critical path).
struct WLane {
  // w_mul: output coefficient k, term i (operand b_jj), partial product q
  uint8_t mk, mi, mjj, mq;
  bool mwrap, mact;
  // w_sqr: coefficient, pair {si, sj}, partial product q, flags
  uint8_t sk, si, sj, sq;
  bool slive, ssquare, sxi, sgrp;
  // lane_sum24 multipliers of w_mul, w_sqr and w_frob (frob: for even n; odd n negates odd q)
  uint32_t mkeep, msend, skeep, ssend, fkeep, fsend;
};
__device__ __forceinline__ WLane wlane_init() {
  WLane L{};
  const int t = threadIdx.x;
  {
    const int grp = t >> 5, j = t & 31;
    L.mact = grp < 6 && j < 24;
    L.mk = grp < 6 ? grp : 0;
    L.mi = L.mact ? j >> 2 : 0;
    L.mq = j & 3;
    int jj = (int)L.mk - (int)L.mi;
    L.mwrap = jj < 0;
    L.mjj = (uint8_t)(jj < 0 ? jj + 6 : jj);
  }
  {
    const int grp = t >> 4, j = t & 15;
    L.sgrp = grp < 6;
    L.sk = L.sgrp ? grp : 0;
    L.sq = j & 3;
    const SqrTerm tm = c_sqr[L.sk][j >> 2];
    L.slive = L.sgrp && tm.i >= 0;
    L.si = L.slive ? tm.i : 0;
    L.sj = L.slive ? tm.j : 0;
    L.ssquare = L.si == L.sj;
    L.sxi = L.slive && tm.xi;
  }
  {  // w_mul q: 0 a0 b0 (re +), 1 a1 b1 (re -), 2 a0 b1 (im), 3 a1 b0 (im)
    const int q = L.mq;
    const int re = !L.mact ? 0 : (q == 0 ? 1 : (q == 1 ? -1 : 0)), im = L.mact && q >= 2 ? 1 : 0;
    keep_send(re, im, L.mwrap, L.mkeep, L.msend);
  }
  {  // w_sqr q: a square a0^2 (re +), a1^2 (re -), 2 a0 a1 (im); a cross term twice the w_mul terms
    const int q = L.sq, f = L.ssquare ? 1 : 2;
    int re = q == 0 ? f : (q == 1 ? -f : 0), im = q == 2 ? 2 : (q == 3 && !L.ssquare ? 2 : 0);
    if (!L.slive) re = im = 0;
    keep_send(re, im, L.sxi, L.skeep, L.ssend);
  }
  {  // w_frob lanes t < 24: coefficient t >> 2, q = t & 3 as in w_mul
    const int q = t & 3;
    const bool act = (t >> 2) < 6;
    const int re = !act ? 0 : (q == 0 ? 1 : (q == 1 ? -1 : 0)), im = act && q >= 2 ? 1 : 0;
    keep_send(re, im, false, L.fkeep, L.fsend);
  }
  return L;
}

// the lane pair (j = 0, 1) of a coefficient group reduces and stores re / im in parallel
__device__ __forceinline__ void store_coeff(Fq2* __restrict__ dst, int k, int j, const Lz& v) {
  if (j < 2) st_fq(j ? &dst[k].c1 : &dst[k].c0, lz_reduce(v));
}

// OP_MUL's imm: multiply by the conjugate (odd w-coefficients negated) of operand a / b
constexpr int kConjA = 1, kConjB = 2;
// dst = a * b (dst distinct from a and b); conj (kConjA / kConjB): multiply by conj(a) / conj(b),
// i.e. negate the terms of a's / b's odd w-coefficients -- a sign on the lane's multipliers
SV_WG_FN void w_mul(const WLane& L, Fq2* __restrict__ dst, const Fq2* a, const Fq2* b, int conj = 0) {
  const int t = threadIdx.x;
  if (t < 192) {  // waves 0-2 (uniform per wave)
    const int q = L.mq;
    // q: 0 a0 b0 (re +), 1 a1 b1 (re -), 2 a0 b1 (im +), 3 a1 b0 (im +); idle lanes multiply by 0
    const Fq ax = ld_fq((q & 1) ? &a[L.mi].c1 : &a[L.mi].c0);
    const Fq by = ld_fq((q == 1 || q == 2) ? &b[L.mjj].c1 : &b[L.mjj].c0);
    const bool flip = ((conj & kConjA) && (L.mi & 1)) != ((conj & kConjB) && (L.mjj & 1));
    const uint32_t keep = flip ? 0u - L.mkeep : L.mkeep, send = flip ? 0u - L.msend : L.msend;
    // [0, 2p): the lane sums reduce once per coefficient
    store_coeff(dst, L.mk, t & 31, lane_sum24<5>(fe_mul_lazy(ax, by), keep, send));
  }
  __syncthreads();
}

// dst = a^2 (dst distinct from a): coefficient k sums the pairs {i, j}, i + j = k (mod 6) of
// c_sqr; a square term a_i^2 = a0^2 - a1^2 + 2 a0 a1 u, a cross term 2 a_i a_j
SV_WG_FN void w_sqr(const WLane& L, Fq2* __restrict__ dst, const Fq2* a) {
  const int t = threadIdx.x;
  if (t < 128) {  // waves 0-1
    const int q = L.sq;
    const bool square = L.ssquare;
    // a_i^2 = a0^2 - a1^2 + 2 a0 a1 u: q 0 a0 a0, 1 a1 a1 (re -), 2 a0 a1 (im x2); a cross term
    // takes x from a_i (q odd: c1) and y from a_j (q 1, 2: c1)
    const bool xc1 = square ? q == 1 : (q & 1);
    const bool yc1 = square ? q != 0 : (q == 1 || q == 2);
    const Fq x = ld_fq(xc1 ? &a[L.si].c1 : &a[L.si].c0);
    const Fq y = ld_fq(yc1 ? &a[L.sj].c1 : &a[L.sj].c0);
    const Lz s = lane_sum24<4>(fe_mul_lazy(x, y), L.skeep, L.ssend);
    if (L.sgrp) store_coeff(dst, L.sk, t & 15, s);
  }
  __syncthreads();
}

// dst = frob^n(a): coefficient k -> conj^n(a_k) * gamma_(n,k); gam = c_gamma staged in LDS
SV_WG_FN void w_frob(const WLane& L, Fq2* __restrict__ dst, const Fq2* a, int n, const Fq* gam) {
  const int t = threadIdx.x;
  if (t < 64) {
    const int k = t >> 2, q = t & 3;
    const bool act = k < 6;
    const int kk = act ? k : 0;
    const Fq x = ld_fq((q & 1) ? &a[kk].c1 : &a[kk].c0);
    const Fq gc = ld_fq(gam + ((n - 1) * 6 + kk) * 2 + ((q == 1 || q == 2) ? 1 : 0));
    const bool flip = (n & 1) && (q & 1);  // conj^n: odd n negates a_k's c1 (the odd q lanes' x)
    const Lz s = lane_sum24<2>(fe_mul_lazy(x, gc), flip ? 0u - L.fkeep : L.fkeep, flip ? 0u - L.fsend : L.fsend);
    if (act) store_coeff(dst, k, q, s);
  }
  __syncthreads();
}

// dst = conj(a) (odd w-coefficients negated) or a copy.  Slots are [0, 2p); both representatives
// of a residue are valid inputs, and the result is a slot value again
SV_WG_FN void w_conj(Fq2* __restrict__ dst, const Fq2* a, bool neg_odd = true) {
  const int t = threadIdx.x;
  if (t < 12) {
    const int k = t >> 1;
    const Fq v = (t & 1) ? a[k].c1 : a[k].c0;
    const Fq r = (neg_odd && (k & 1)) ? fq_neg2p(v) : v;
    if (t & 1) dst[k].c1 = r;
    else dst[k].c0 = r;
  }
  __syncthreads();
}

// ni = N^-1 for N = a conj(a) (even coefficients = an Fq6 element c0 + c1 v + c2 v^2, v = w^2), as
// in g_inv: the three t_j on three lanes, the norm d and its Fq2 inverse (one fe_inv) on one lane.
// Slots are [0, 2p); both representatives of a residue are valid inputs (canonicalised on entry),
// the odd coefficients of nn are not read, and ni is fully reduced
__device__ __forceinline__ void w_norm_inv(Fq2* __restrict__ ni, const Fq2* nn, Fq2* tj, Fq2* di) {
  const int t = threadIdx.x;
  if (t < 3) {
    const Fq2 c0 = fq2_canon(nn[0]), c1 = fq2_canon(nn[2]), c2 = fq2_canon(nn[4]);
    const Fq2 x = t == 0 ? c0 : (t == 1 ? c2 : c1);
    const Fq2 y0 = t == 0 ? c1 : c0, y1 = t == 0 ? c2 : (t == 1 ? c1 : c2);
    const Fq2 sq = x * x, pr = y0 * y1;
    tj[t] = t == 0 ? sq - fq2_mul_xi(pr) : (t == 1 ? fq2_mul_xi(sq) - pr : sq - pr);
  }
  __syncthreads();
  if (t == 0) {
    const Fq2 d = fq2_canon(nn[0]) * tj[0] + fq2_mul_xi(fq2_canon(nn[4]) * tj[1] + fq2_canon(nn[2]) * tj[2]);
    *di = fq2_inv(d);
  }
  __syncthreads();
  if (t < 6) ni[t] = (t & 1) ? Fq2::zero() : tj[t >> 1] * (*di);
  __syncthreads();
}

// ---- The decider as a straight-line program over LDS slots, run by one interpreter loop: each
// operation's code exists once (no per-call register save / restore: an out-of-line operation cost
// ~1500 cycles of call overhead, measured with tools/ubench_wg.hip), and the op stream is read with
// wave-uniform scalar loads.  Operands: slot index, or a pair product D[i] / merged step M[i].
enum WCode : uint8_t { OP_MUL, OP_SQR, OP_FROB, OP_CONJ, OP_COPY, OP_NORM_INV };
struct WOp {
  uint8_t code, imm;
  uint16_t dst, a, b;
};
constexpr uint16_t kOpD = 1u << 14, kOpM = 2u << 14, kOpY = 3u << 14;  // (tag 3: a paired-step product Y)

// Round 4: TWO Miller steps per multiplication.  f <- (f^2 X_j)^2 X_{j+1} = f^4 Y_p with
// Y_p = X_j^2 X_{j+1}, X the steps' multipliers (pair products D / merged products M).  The Y_p do
// not depend on f, so the prologue forms all 32 of them in parallel (pair_steps: one output
// coefficient per lane, two rounds of Fq2 products); the loop then runs 2 squares + 1 product per
// pair instead of 2 + 2, 32 fewer Fq12 operations on the chain.
struct StepTab {
  uint16_t x[ATE_NAF_LEN];  // step multipliers in loop order; x[0] is the first step's (a copy)
  int n;
  int m_final;  // merged product of the two Frobenius steps
};
constexpr StepTab make_steps() {
  StepTab t{};
  int m = 0, idx = 0;
  for (int i = ATE_NAF_LEN - 1; i >= 1; i--) {
    t.x[t.n++] = ATE_NAF[i - 1] != 0 ? (uint16_t)(kOpM | m++) : (uint16_t)(kOpD | idx);
    idx += ATE_NAF[i - 1] != 0 ? 2 : 1;
  }
  t.m_final = m;
  return t;
}
constexpr int kStepPairs = (make_steps().n - 1) / 2;
enum WSlot {
  S_F0, S_F1, S_FI, S_AC, S_NN, S_NI, S_TAB, S_X0 = S_TAB + 8, S_X1, S_FX, S_FX2, S_FX3, S_A, S_B, S_C, S_B6, S_B12,
  S_B18, S_A6, S_A12, S_A18, S_A30, S_Y, S_Y36, S_L0, S_L1, S_L2, S_T0, S_T1, S_T2, S_E0, S_E1, S_E2, S_GT, kSlots,
  S_F0SQ = S_TAB + 4  // (the power table's upper half, free since round 6: no conjugate entries)
};
constexpr int kMaxOps = 512;
struct WProg {
  WOp ops[kMaxOps];
  int n;
  int nv;  // ops of the verdict program; ops[nv, n) append the Gt value (parity tests)
  constexpr void op(WCode c, int d, int a, int b = 0, int imm = 0) {
    ops[n++] = WOp{(uint8_t)c, (uint8_t)imm, (uint16_t)d, (uint16_t)a, (uint16_t)b};
  }
  // dst = a^x, x = BN_X in width-4 NAF; table of odd powers a, a^3, a^5, a^7 (a itself is entry 0,
  // read where it lies); a negative digit multiplies by the entry's conjugate (the inverse on the
  // cyclotomic subgroup), which OP_MUL applies as a sign of its odd-index terms (kConjB) -- round 6:
  // no OP_COPY / OP_CONJ ops (15 per pow_x, ~800 cycles each); the chain ping-pongs between S_X0
  // and S_X1
  // sq / cube: slots already holding a^2 / a^3 (the hard part forms them just before two of the
  // three calls), else formed here; sq_out: a slot to keep a^2 in (else S_X0, which the chain reuses)
  constexpr void pow_x(int dst, int a, int sq = -1, int cube = -1, int sq_out = -1) {
    const XNaf xn = make_xnaf();
    int a2 = sq;
    if (a2 < 0) {
      a2 = sq_out >= 0 ? sq_out : S_X0;
      op(OP_SQR, a2, a);
    }
    int a3 = cube;
    if (a3 < 0) {
      a3 = S_TAB + 1;
      op(OP_MUL, a3, a, a2);
    }
    op(OP_MUL, S_TAB + 2, a3, a2);
    op(OP_MUL, S_TAB + 3, S_TAB + 2, a2);
    auto entry = [a, a3](int d) {
      const int e = ((d > 0 ? d : -d) - 1) / 2;
      return e == 0 ? a : (e == 1 ? a3 : S_TAB + e);
    };
    int r = entry(xn.d[xn.len - 1]);  // (the NAF's top digit is positive)
    for (int i = xn.len - 2; i >= 0; i--) {
      const int d = xn.d[i];
      const bool last_sq = i == 0 && d == 0;
      const int s1 = last_sq ? dst : (r == S_X0 ? S_X1 : S_X0);
      op(OP_SQR, s1, r);
      r = s1;
      if (d) {
        const int s2 = i == 0 ? dst : (r == S_X0 ? S_X1 : S_X0);
        op(OP_MUL, s2, r, entry(d), d < 0 ? kConjB : 0);
        r = s2;
      }
    }
  }
};
constexpr WProg make_wprog(bool paired = false) {
  WProg P{};
  const StepTab st = make_steps();
  int f = st.x[0];  // f starts as the first step's multiplier, read where it lies (no copy)
  int j = 1;
  if (paired) {  // f <- f^4 Y_p (see StepTab)
    for (int p = 0; p < kStepPairs; p++, j += 2) {
      P.op(OP_SQR, S_T1, f);
      P.op(OP_SQR, S_F1, S_T1);
      P.op(OP_MUL, S_F0, S_F1, kOpY | p);
      f = S_F0;
    }
  }
  // Miller loop, merged step multipliers as in k_decide_lanes: f <- f^2 * (D_idx or M_m)
  for (; j < st.n; j++) {
    P.op(OP_SQR, S_F1, f);
    P.op(OP_MUL, S_F0, S_F1, st.x[j]);
    f = S_F0;
  }
  P.op(OP_MUL, S_F1, S_F0, kOpM | st.m_final);  // the two Frobenius steps
  // Final exponentiation with NO inversion.  The easy part f^(p^6 - 1) = conj(f) / f is kept as the
  // fraction conj(w) / w with w = f: every value of the chain below is a power v^k of
  // v = f^((p^6 - 1)(p^2 + 1)), and v^k = conj(w_k) / w_k where w_k is what the same chain computes
  // from w_0 = f^(p^2 + 1) -- a product of fractions multiplies the w's, a square squares w, a
  // Frobenius maps w, and conj (the inverse on the cyclotomic subgroup) conjugates w, because
  // conj(v^k) = w_k / conj(w_k) = conj(w') / w' with w' = conj(w_k).  So the result is
  // conj(W) / W, which is 1 iff W = conj(W), i.e. iff W's odd w-coefficients vanish: the verdict
  // needs no f^-1 (a single-lane field inversion, ~150k cycles, 8 % of the kernel).  The Gt value
  // itself (tests only) divides at the end: ops[nv, n).
  P.op(OP_FROB, S_C, S_F1, 0, 2);
  P.op(OP_MUL, S_F0, S_C, S_F1);         // w_0 = f^(p^2 + 1), standing for K_F = conj(w_0) / w_0
  P.pow_x(S_FX, S_F0, -1, -1, S_F0SQ);  // f^2 kept for l0 below
  P.op(OP_SQR, S_A, S_FX);
  P.op(OP_MUL, S_B, S_A, S_FX);
  P.op(OP_SQR, S_B6, S_B);
  P.op(OP_SQR, S_B12, S_B6);
  P.op(OP_MUL, S_B18, S_B12, S_B6);
  P.pow_x(S_FX2, S_FX, S_A, S_B);        // fx^2, fx^3 from just above
  P.op(OP_SQR, S_A, S_FX2);
  P.op(OP_MUL, S_B, S_A, S_FX2);
  P.op(OP_SQR, S_A6, S_B);
  P.op(OP_SQR, S_A12, S_A6);
  P.op(OP_MUL, S_A18, S_A12, S_A6);
  P.op(OP_MUL, S_A30, S_A18, S_A12);
  P.pow_x(S_FX3, S_FX2, S_A, S_B);       // fx2^2, fx2^3 from just above
  P.op(OP_SQR, S_A, S_FX3);
  P.op(OP_SQR, S_B, S_A);
  P.op(OP_SQR, S_Y, S_B);                // fx3^8
  P.op(OP_MUL, S_A, S_Y, S_FX3);
  P.op(OP_SQR, S_B, S_A);
  P.op(OP_SQR, S_Y36, S_B);              // fx3^36
  P.op(OP_MUL, S_L2, S_F0, S_A6);        // l2 = f a6
  P.op(OP_MUL, S_T0, S_Y36, S_A18);
  P.op(OP_MUL, S_T1, S_T0, S_B12);
  P.op(OP_MUL, S_L1, S_T1, S_F0, kConjA);  // l1 = conj(y36 a18 b12) f
  P.op(OP_MUL, S_T0, S_Y36, S_A30);
  P.op(OP_MUL, S_T1, S_T0, S_B18);
  P.op(OP_MUL, S_T0, S_T1, S_F0SQ);      // l0 = conj(T0) = conj(y36 a30 b18 f^2), applied below
  P.op(OP_FROB, S_T1, S_L1, 0, 1);
  P.op(OP_MUL, S_E0, S_T0, S_T1, kConjA);
  P.op(OP_FROB, S_T2, S_L2, 0, 2);
  P.op(OP_MUL, S_E1, S_E0, S_T2);
  P.op(OP_FROB, S_T0, S_F0, 0, 3);
  P.op(OP_MUL, S_E2, S_E1, S_T0);        // W: the result is conj(W) / W
  P.nv = P.n;
  P.op(OP_CONJ, S_AC, S_E2);
  P.op(OP_MUL, S_NN, S_E2, S_AC);        // N = W conj(W) in Fq6
  P.op(OP_NORM_INV, S_NI, S_NN);
  P.op(OP_MUL, S_FI, S_AC, S_NI);        // W^-1 = conj(W) / N
  P.op(OP_MUL, S_GT, S_AC, S_FI);        // conj(W) / W
  return P;
}
__constant__ WProg c_wprog = make_wprog();
__constant__ WProg c_wprog2 = make_wprog(true);
__constant__ StepTab c_steps = make_steps();
constexpr int kResultSlot = S_E2, kGtSlot = S_GT;
static_assert(make_wprog().n <= kMaxOps, "decider program too long");
static_assert(make_wprog(true).n + 32 == make_wprog().n, "pairing saves one product per step pair");
static_assert(kStepPairs * 6 * sizeof(Fq2) <= (size_t)kSlots * 6 * sizeof(Fq2), "Q fits the slots");

// Y_p = X_j^2 X_{j+1} for every step pair (j = 1 + 2p): Q_p = X_j^2 into Q (the slot region, free
// during the prologue), then Y_p = Q_p X_{j+1}; one (pair, output coefficient) per lane, Fq2
// convolutions with the w^6 = xi wrap
__device__ __forceinline__ const Fq2* step_x(uint16_t o, const Fq2* D, const Fq2* M) {
  const uint32_t i = o & (kOpD - 1);
  return (o >> 14) == 2 ? M + 6 * i : D + 6 * i;
}
// coefficient k of a * b (w^6 = xi); divergence-free: lanes of one wave hold different k, so every
// lane forms the same six products (an operand index and a wrap select per term)
__device__ __forceinline__ Fq2 conv6(const Fq2* a, const Fq2* b, int k) {
  Fq2 acc = Fq2::zero();
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int j = k - i;
    const bool wrap = j < 0;
    const Fq2 t = a[i] * b[wrap ? j + 6 : j];
    const Fq2 tx = fq2_mul_xi(t);
    acc = acc + (wrap ? tx : t);
  }
  return acc;
}
__device__ __forceinline__ void pair_steps(Fq2* __restrict__ Q, Fq2* __restrict__ Y, const Fq2* D, const Fq2* M,
                                           int lane, int lanes) {
  for (int job = lane; job < kStepPairs * 6; job += lanes) {
    const int p = job / 6, k = job % 6;
    const Fq2* x = step_x(c_steps.x[1 + 2 * p], D, M);
    Q[6 * p + k] = conv6(x, x, k);
  }
  __syncthreads();
  for (int job = lane; job < kStepPairs * 6; job += lanes) {
    const int p = job / 6, k = job % 6;
    Y[6 * p + k] = conv6(Q + 6 * p, step_x(c_steps.x[2 + 2 * p], D, M), k);
  }
}

// ---- Round 5: the prologue's products one Fq2 product per lane job.  merge_products and
// pair_steps above give each lane a whole output coefficient: 5-10 (merges) and 2 x 6 (paired
// steps) dependent Fq2 products per lane, 23 + 48 us of the kernel with most of the block's
// issue capacity unused (measured by SV_WG_PROLOGUE_ONLY builds).  Here every term product is its
// own job (written to an LDS scratch X, with the w^6 = xi wrap applied), and after a barrier one
// lane per output coefficient adds its terms: 575 + 744 + 1116 jobs over 256 lanes, 3 + 3 + 5
// products deep instead of 10 + 12.  The values are the same canonical field elements.
constexpr int kScratchJobs = kStepPairs * 36;  // the largest phase (Y_p = Q_p X_{j+1})
static_assert(kMaxMerge * 25 <= kScratchJobs && kStepPairs * 24 <= kScratchJobs, "scratch holds every phase");
// M_m = D_a D_{a+1} (both 5-sparse: coefficients 0-4) for every merged step
__device__ __forceinline__ void merge_products_wide(Fq2* __restrict__ M, const Fq2* __restrict__ D, Fq2* __restrict__ X,
                                                    int t, int nt) {
  const int nm = c_merge.n;
  for (int job = t; job < nm * 25; job += nt) {
    const int m = job / 25, r = job % 25, i = r / 5, j = r % 5;
    const Fq2* a = D + 6 * c_merge.first[m];
    const Fq2 v = a[i] * a[6 + j];
    X[job] = i + j >= 6 ? fq2_mul_xi(v) : v;
  }
  __syncthreads();
  for (int job = t; job < nm * 6; job += nt) {
    const int m = job / 6, k = job % 6;
    Fq2 acc = Fq2::zero();
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const int j = k - i < 0 ? k - i + 6 : k - i;
      if (j < 5) acc = acc + X[25 * m + 5 * i + j];
    }
    M[6 * m + k] = acc;
  }
}
// Y_p = X_j^2 X_{j+1} (j = 1 + 2p): the square by c_sqr's pair terms (<= 4 per coefficient, cross
// terms doubled), into Q (the slot region, free during the prologue), then the product's 36 terms
__device__ __forceinline__ void pair_steps_wide(Fq2* __restrict__ Q, Fq2* __restrict__ Y, const Fq2* D, const Fq2* M,
                                                Fq2* __restrict__ X, int t, int nt) {
  for (int job = t; job < kStepPairs * 24; job += nt) {
    const int pk = job >> 2, p = pk / 6, k = pk % 6;
    const SqrTerm tm = c_sqr[k][job & 3];
    const Fq2* x = step_x(c_steps.x[1 + 2 * p], D, M);
    const bool live = tm.i >= 0;
    Fq2 v = x[live ? tm.i : 0] * x[live ? tm.j : 0];
    if (tm.dbl) v = v + v;
    if (tm.xi) v = fq2_mul_xi(v);
    X[job] = live ? v : Fq2::zero();
  }
  __syncthreads();
  for (int job = t; job < kStepPairs * 6; job += nt)
    Q[job] = (X[4 * job] + X[4 * job + 1]) + (X[4 * job + 2] + X[4 * job + 3]);
  __syncthreads();
  for (int job = t; job < kStepPairs * 36; job += nt) {
    const int p = job / 36, r = job % 36, i = r / 6, j = r % 6;
    const Fq2 v = Q[6 * p + i] * step_x(c_steps.x[2 + 2 * p], D, M)[j];
    X[job] = i + j >= 6 ? fq2_mul_xi(v) : v;
  }
  __syncthreads();
  for (int job = t; job < kStepPairs * 6; job += nt) {
    const int p = job / 6, k = job % 6;
    Fq2 acc = Fq2::zero();
#pragma unroll
    for (int i = 0; i < 6; i++) acc = acc + X[36 * p + 6 * i + (k - i < 0 ? k - i + 6 : k - i)];
    Y[job] = acc;
  }
}

constexpr size_t kLdsE = 2 * (size_t)ATE_NUM_LINES * sizeof(LineCoeff);
constexpr size_t kLdsD = (size_t)ATE_NUM_LINES * 6 * sizeof(Fq2);
constexpr size_t kLdsSlots = (size_t)kSlots * 6 * sizeof(Fq2);
constexpr size_t kLdsGamma = sizeof(c_gamma);
constexpr size_t kLdsScratch = (size_t)kScratchJobs * sizeof(Fq2);
constexpr size_t kLds = kLdsE + kLdsD + kLdsSlots + kLdsGamma + kLdsScratch;
static_assert(kLds + 512 <= 160 * 1024, "the block's LDS (dynamic + static) fits a CU's 160 KiB");
static_assert((size_t)(kMaxMerge + kStepPairs) * 6 * sizeof(Fq2) <= kLdsE, "M and Y fit the line region");
}  // namespace wg

__global__ void __launch_bounds__(wg::kThreads) k_decide_wg(const G1Aff* __restrict__ lhs, const G1Aff* __restrict__ rhs,
                                                          uint32_t n, const LineCoeff* __restrict__ L1,
                                                          const LineCoeff* __restrict__ L2, int mont_in,
                                                          int32_t* __restrict__ verdict, Fq12* __restrict__ gt,
                                                          const Fq2* __restrict__ kc, int paired, int wide) {
  using namespace wg;
  extern __shared__ __attribute__((aligned(16))) unsigned char dec_lds[];
  __shared__ Fq2 tj[3], di;
  LineCoeff* E = reinterpret_cast<LineCoeff*>(dec_lds);
  Fq2* D = reinterpret_cast<Fq2*>(dec_lds + kLdsE);
  Fq2* S = reinterpret_cast<Fq2*>(dec_lds + kLdsE + kLdsD);
  Fq2* M = reinterpret_cast<Fq2*>(E);  // the evaluated lines are dead once M is formed
  Fq* gam = reinterpret_cast<Fq*>(dec_lds + kLdsE + kLdsD + kLdsSlots);
  Fq2* X = reinterpret_cast<Fq2*>(dec_lds + kLdsE + kLdsD + kLdsSlots + kLdsGamma);  // prologue scratch
  const int t = threadIdx.x;
  for (int i = t; i < (int)(kLdsGamma / 4); i += kThreads) reinterpret_cast<uint32_t*>(gam)[i] = c_gamma[i];
  const uint32_t acc = blockIdx.x;
  G1Aff p1 = load_aff_d(lhs, acc, mont_in), p2 = load_aff_d(rhs, acc, mont_in);
  // prologue: pair products D (from the key's constants; identity points evaluate the lines), merged
  // step multipliers M
  if (kc && !p1.is_identity() && !p2.is_identity()) {  // block-uniform
    __shared__ Fq sc[4];
    if (t < 4) sc[t] = (t == 1 || t == 3 ? p1.x : p1.y) * (t == 0 ? p2.y : (t == 3 ? p2.y : p2.x));
    __syncthreads();
    pair_products_kc(D, kc, sc, p1, p2, t, kThreads);
  } else {
    eval_lines(E, L1, L2, p1, p2, t, kThreads);
    __syncthreads();
    pair_products(D, E, t, kThreads);
  }
  __syncthreads();
#if defined(SV_WG_PROLOGUE_ONLY) && SV_WG_PROLOGUE_ONLY == 1
  if (t == 0) verdict[acc] = 0;  // timing of the pair products alone
  return;
#endif
  if (wide) merge_products_wide(M, D, X, t, kThreads);
  else merge_products(M, D, t, kThreads);  // (a divergence-free 5-term walk measured no faster)
  __syncthreads();
#if defined(SV_WG_PROLOGUE_ONLY) && SV_WG_PROLOGUE_ONLY == 2
  if (t == 0) verdict[acc] = 0;  // timing through the merged products
  return;
#endif
  Fq2* Y = M + 6 * kMaxMerge;  // the paired steps' products, behind M in the dead line region
  if (paired) {
    if (wide) pair_steps_wide(S, Y, D, M, X, t, kThreads);
    else pair_steps(S, Y, D, M, t, kThreads);
    __syncthreads();
  }
  const WProg& prog = paired ? c_wprog2 : c_wprog;
  auto opnd = [&](uint16_t o) -> Fq2* {
    const uint32_t i = o & (kOpD - 1), tag = o >> 14;
    return tag == 3 ? Y + 6 * i : (tag == 2 ? M + 6 * i : (tag == 1 ? D + 6 * i : S + 6 * i));
  };
  const WLane Ln = wlane_init();
#ifdef SV_WG_PROLOGUE_ONLY
  const int nops = 0;  // timing of the prologue alone (tools/decider_bench.py with SVGPU_LIB)
#else
  const int nops = gt ? prog.n : prog.nv;
#endif
  WOp nxt = prog.ops[0];
  for (int pc = 0; pc < nops; pc++) {
    const WOp op = nxt;
    if (pc + 1 < nops) nxt = prog.ops[pc + 1];  // next op's scalar load in flight during this one
    Fq2* dst = S + 6 * op.dst;
    const Fq2* a = opnd(op.a);
    switch (op.code) {
      case OP_MUL: w_mul(Ln, dst, a, opnd(op.b), op.imm); break;
      case OP_SQR: w_sqr(Ln, dst, a); break;
      case OP_FROB: w_frob(Ln, dst, a, op.imm, gam); break;
      case OP_CONJ: w_conj(dst, a, true); break;
      case OP_COPY: w_conj(dst, a, false); break;
      default: w_norm_inv(dst, a, tj, &di); break;
    }
  }
  const Fq2* e = S + 6 * kResultSlot;
  if (t < 6) {
    if (t == 0) {  // conj(W) / W == 1  <=>  the odd w-coefficients of W are zero
      // slots are [0, 2p): a zero coefficient is a raw 0 or a raw p, hence the fq2_canon
      const bool ok = fq2_canon(e[1]).is_zero() && fq2_canon(e[3]).is_zero() && fq2_canon(e[5]).is_zero();
      verdict[acc] = ok ? 1 : 0;
    }
    if (gt) reinterpret_cast<Fq2*>(gt + acc)[(t & 1) * 3 + (t >> 1)] = fq2_canon(S[6 * kGtSlot + t]);
  }
}

// ---------------------------------------------------------------------------------------------
// Host side: prepared-line cache.  Each deciding key's lines live in their own immutable device
// buffer, shared by refcount: a call holds its entry until its stream has synchronised, so a
// concurrent call with another key (a second verifier on another rayon worker) uploads into a NEW
// buffer and can never overwrite lines a running kernel reads.  A few keys are kept per device
// (verifiers rarely switch keys); an evicted entry is freed when its last in-flight call drops it.
// ---------------------------------------------------------------------------------------------
namespace {
struct LineEntry {
  unsigned char key[2 * sizeof(G2Aff)];
  int device = 0;
  LineCoeff* d_lines = nullptr;  // 2 * ATE_NUM_LINES, written once before the entry is published
  Fq2* d_kc = nullptr;           // kKc * ATE_NUM_LINES pair constants (k_decide_wg), same lifetime
  ~LineEntry() {
    if (d_lines || d_kc) {
      int prev = 0;
      (void)hipGetDevice(&prev);
      (void)hipSetDevice(device);
      if (d_lines) (void)hipFree(d_lines);
      if (d_kc) (void)hipFree(d_kc);
      (void)hipSetDevice(prev);
    }
  }
};
constexpr int kLineCacheKeys = 4;
struct LineCache {
  std::mutex mu;
  std::shared_ptr<LineEntry> e[kLineCacheKeys];  // most recently used first
};
// leaked on purpose: cached entries must not hipFree from static destructors after HIP teardown
LineCache* const g_cache = new LineCache[64];
}  // namespace

static G2Aff g2_from_abi(const sv_g2_affine* q, int mont_in) {
  G2Aff r;
  memcpy(&r.x.c0, &q->x.c0, 32);
  memcpy(&r.x.c1, &q->x.c1, 32);
  memcpy(&r.y.c0, &q->y.c0, 32);
  memcpy(&r.y.c1, &q->y.c1, 32);
  if (!mont_in) {
    r.x.c0 = fe_to_mont(r.x.c0);
    r.x.c1 = fe_to_mont(r.x.c1);
    r.y.c0 = fe_to_mont(r.y.c0);
    r.y.c1 = fe_to_mont(r.y.c1);
  }
  return r;
}

static bool g2_on_twist(const G2Aff& q) {
  Fq2 lhs = fq2_sqr(q.y);
  Fq2 rhs = fq2_sqr(q.x) * q.x + fq2_const(TWIST_B_C0, TWIST_B_C1);
  return lhs == rhs;
}

// The caller keeps `*out` alive until every kernel reading its lines has finished.
static int decider_lines(const sv_g2_affine* g2, const sv_g2_affine* s_g2, int form, int device,
                         hipStream_t st, std::shared_ptr<LineEntry>* out) {
  if (device < 0 || device >= 64) return SV_ERR_ARG;
  G2Aff q1 = g2_from_abi(g2, form == SV_MONTGOMERY);
  G2Aff q2 = g2_from_abi(s_g2, form == SV_MONTGOMERY);
  if (q1.is_identity() || q2.is_identity() || !g2_on_twist(q1) || !g2_on_twist(q2)) {
    set_error("deciding key G2 point is the identity or not on the twist");
    return SV_ERR_ARG;
  }
  q2.y = -q2.y;  // -s_g2
  unsigned char key[sizeof(LineEntry::key)];
  memcpy(key, &q1, sizeof(G2Aff));
  memcpy(key + sizeof(G2Aff), &q2, sizeof(G2Aff));
  LineCache& c = g_cache[device];
  {
    std::lock_guard<std::mutex> lk(c.mu);
    for (int i = 0; i < kLineCacheKeys; i++) {
      if (c.e[i] && memcmp(key, c.e[i]->key, sizeof key) == 0) {
        std::shared_ptr<LineEntry> hit = c.e[i];
        for (int j = i; j > 0; j--) c.e[j] = c.e[j - 1];
        c.e[0] = hit;
        *out = std::move(hit);
        return SV_OK;
      }
    }
  }
  // miss: prepare and upload outside the lock into a fresh buffer, then publish
  auto ent = std::make_shared<LineEntry>();
  memcpy(ent->key, key, sizeof key);
  ent->device = device;
  std::vector<LineCoeff> h(2 * ATE_NUM_LINES);
  g2_prepare(q1, h.data());
  g2_prepare(q2, h.data() + ATE_NUM_LINES);
  std::vector<Fq2> kc((size_t)kKc * ATE_NUM_LINES);
  pair_constants(h.data(), h.data() + ATE_NUM_LINES, kc.data());
  SV_HIP(hipMalloc(&ent->d_lines, h.size() * sizeof(LineCoeff)));
  SV_HIP(hipMalloc(&ent->d_kc, kc.size() * sizeof(Fq2)));
  SV_HIP(hipMemcpyAsync(ent->d_lines, h.data(), h.size() * sizeof(LineCoeff), hipMemcpyHostToDevice, st));
  SV_HIP(hipMemcpyAsync(ent->d_kc, kc.data(), kc.size() * sizeof(Fq2), hipMemcpyHostToDevice, st));
  SV_HIP(hipStreamSynchronize(st));
  {
    std::lock_guard<std::mutex> lk(c.mu);
    for (int j = kLineCacheKeys - 1; j > 0; j--) c.e[j] = c.e[j - 1];
    c.e[0] = ent;
  }
  *out = std::move(ent);
  return SV_OK;
}

int decide_run_device(const sv_g2_affine* g2, const sv_g2_affine* s_g2, const void* d_lhs,
                      const void* d_rhs, size_t n, int form, int device, hipStream_t user_stream,
                      int32_t* first_fail, int32_t* verdicts_host, sv_fq12* gt_host) {
  if (n == 0) {
    set_error("accumulators should not be empty");
    return SV_ERR_EMPTY;
  }
  if (form != SV_CANONICAL && form != SV_MONTGOMERY) {
    set_error("bad form %d", form);
    return SV_ERR_ARG;
  }
  WsLease lease(device, user_stream);
  if (!lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = lease.get();
  hipStream_t st = ws->stream;
  std::shared_ptr<LineEntry> line_ref;  // held until the stream has synchronised (below)
  SV_TRY(decider_lines(g2, s_g2, form, device, st, &line_ref));
  const LineCoeff* lines = line_ref->d_lines;
  size_t bytes = Workspace::aligned(n * 4) + (gt_host ? Workspace::aligned(n * sizeof(Fq12)) : 0);
  SV_TRY(ws->reserve(bytes));
  SV_TRY(ws->reserve_pinned(n * 4 + 256));
  // The kernel writes the verdicts straight into the workspace's pinned host buffer (device-mapped;
  // the stream synchronisation below makes them visible): no D2H copy after the kernel, 6-11 us
  // less per call (profiles/r05_decide_zc_ab.log).  SVGPU_DECIDE_ZC=0 keeps the device buffer + copy.
  const bool zc = !getenv("SVGPU_DECIDE_ZC") || atoi(getenv("SVGPU_DECIDE_ZC")) != 0;  // read per call
  int32_t* d_verdict = zc ? nullptr : ws->carve<int32_t>(n);
  if (zc) SV_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_verdict), ws->pinned, 0));
  Fq12* d_gt = gt_host ? ws->carve<Fq12>(n) : nullptr;
  // kernel timing events (sv_decide_last_kernel_ms); SVGPU_DECIDE_EVENTS=0 leaves them out (read per call)
  const bool timed = !getenv("SVGPU_DECIDE_EVENTS") || atoi(getenv("SVGPU_DECIDE_EVENTS")) != 0;
  if (timed) SV_HIP(hipEventRecord(ws->ev[0], st));
  // SVGPU_DECIDER_LANES = 48 (6 x 8 lanes per accumulator, 1 per wave; default) or 24 (6 x 4, 2 per wave)
  // SVGPU_DECIDER_LANES: 256 = k_decide_wg (one 4-wave block per accumulator: lowest latency, one
  // block per CU), 48 / 24 = k_decide_lanes (one wave per accumulator, two blocks per CU: higher
  // throughput once the accumulators outnumber the CUs).  Default: the workgroup kernel while every
  // accumulator gets its own CU, the single-wave one beyond.
  const int lanes_env = getenv("SVGPU_DECIDER_LANES") ? atoi(getenv("SVGPU_DECIDER_LANES")) : 0;
  static thread_local int cu_dev = -1, cus = 256;
  if (cu_dev != device) {
    SV_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    cu_dev = device;
  }
  const int lanes = lanes_env ? lanes_env : (n <= (size_t)cus ? 256 : 48);
  // k_decide_wg's pair products from the key's constants (SVGPU_DECIDER_KC=0: evaluate the lines)
  static const bool kc_env = !getenv("SVGPU_DECIDER_KC") || atoi(getenv("SVGPU_DECIDER_KC")) != 0;
  static const int phases = getenv("SVGPU_DECIDER_PHASES") ? atoi(getenv("SVGPU_DECIDER_PHASES")) : 3;
  // k_decide_wg's two Miller steps per product (SVGPU_DECIDER_PAIR=0: one per step), read per call
  const bool pair_env = !getenv("SVGPU_DECIDER_PAIR") || atoi(getenv("SVGPU_DECIDER_PAIR")) != 0;
  // the prologue's products one per lane job (SVGPU_DECIDER_WIDE=0: one output coefficient per lane)
  const bool wide_env = !getenv("SVGPU_DECIDER_WIDE") || atoi(getenv("SVGPU_DECIDER_WIDE")) != 0;
  const G1Aff* dl = reinterpret_cast<const G1Aff*>(d_lhs);
  const G1Aff* dr = reinterpret_cast<const G1Aff*>(d_rhs);
  const int mont = form == SV_MONTGOMERY ? 1 : 0;
  const LineCoeff* L2 = lines + ATE_NUM_LINES;
  static thread_local int wg_attr_dev = -1;  // > 64 KiB dynamic LDS opt-in, once per thread / device
  if (lanes == 256 && wg_attr_dev != device) {
    SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_decide_wg), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)wg::kLds));
    wg_attr_dev = device;
  }
  if (lanes == 256)
    hipLaunchKernelGGL(k_decide_wg, dim3((unsigned)n), dim3(wg::kThreads), wg::kLds, st, dl, dr, (uint32_t)n, lines,
                       L2, mont, d_verdict, d_gt, kc_env ? line_ref->d_kc : nullptr, pair_env ? 1 : 0, wide_env ? 1 : 0);
  else if (lanes == 48)
    hipLaunchKernelGGL(k_decide_lanes<8>, dim3((unsigned)n), dim3(64), 0, st, dl, dr, (uint32_t)n, lines, L2, mont,
                       d_verdict, d_gt, phases);
  else
    hipLaunchKernelGGL(k_decide_lanes<4>, dim3((unsigned)((n + 1) / 2)), dim3(64), 0, st, dl, dr, (uint32_t)n,
                       lines, L2, mont, d_verdict, d_gt, phases);
  SV_HIP(hipGetLastError());
  if (timed) SV_HIP(hipEventRecord(ws->ev[1], st));
  int32_t* hv = reinterpret_cast<int32_t*>(ws->pinned);
  if (!zc) SV_HIP(hipMemcpyAsync(hv, d_verdict, n * 4, hipMemcpyDeviceToHost, st));
  if (gt_host) {
    std::vector<Fq12> tmp(n);
    SV_HIP(hipMemcpyAsync(tmp.data(), d_gt, n * sizeof(Fq12), hipMemcpyDeviceToHost, st));
    SV_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++) {
      const Fq2* c[6] = {&tmp[i].c0.c0, &tmp[i].c0.c1, &tmp[i].c0.c2,
                         &tmp[i].c1.c0, &tmp[i].c1.c1, &tmp[i].c1.c2};
      for (int k = 0; k < 6; k++) {
        Fq a = fe_from_mont(c[k]->c0), b = fe_from_mont(c[k]->c1);
        memcpy(&gt_host[i].c[k].c0, a.v, 32);
        memcpy(&gt_host[i].c[k].c1, b.v, 32);
      }
    }
  }
  SV_HIP(hipStreamSynchronize(st));
  float ms = -1;
  if (timed) (void)hipEventElapsedTime(&ms, ws->ev[0], ws->ev[1]);
  decider_last_kernel_ms() = ms;
  int32_t ff = -1;
  for (size_t i = 0; i < n; i++) {
    if (verdicts_host) verdicts_host[i] = hv[i];
    if (ff < 0 && !hv[i]) ff = (int32_t)i;
  }
  if (first_fail) *first_fail = ff;
  return SV_OK;
}

float& decider_last_kernel_ms() {
  static thread_local float v = 0;
  return v;
}

}  // namespace sv
