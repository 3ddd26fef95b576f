// Pippenger bucket MSM for BN254 G1 on gfx950.
//
// Replaces util::msm::multi_scalar_multiplication (snark-verifier/src/util/msm.rs:238-316) and
// the naive NativeLoader::multi_scalar_multiplication (snark-verifier/src/loader/native.rs:61-71):
// same group element out, computed as a signed-digit bucket method.
//
// Pipeline (all on one stream, inputs already in HBM):
//   k_to_mont_bases   (canonical input only) bases -> Montgomery workspace copy
//   k_bin_hist        per block of sort_chunk points (1024 at 2^20; XCD-aware block map, sort_block): signed c-bit digits of every
//                     window (digits never stored; the GLV halves are, 32 B per point, for the scatter)
//                     + the point table, LDS
//                     histogram of (window, coarse bin = top bits of the bucket)
//   k_bin_scan_chunks / k_bin_scan   offsets of every (window, bin, block) run
//   k_bin_scatter     digits again (from the stored halves); entries appended to their block's (window, bin) run -> tmp
//   k_fine_sort<2>    one block per (window, bin), both region kinds in one launch: counting sort
//                     by the fine bucket index inside the bin's L2-resident region -> ent[], bucket
//                     offsets gst[], owner bucket of every accumulate chunk tstart[]
//   k_accumulate      each thread sums K consecutive sorted entries (mixed XYZZ adds over 29-bit
//                     limbs by default, points from a table in that form -- see AccChain; perfect
//                     load balance whatever the digit distribution), complete buckets written
//                     directly, bucket pieces that cross a thread boundary to pfirst/plast
//                     (two-piece buckets inside a block are joined at the end through LDS)
//   k_fixup           the other crossing buckets, queued by k_accumulate (heavy ones: block-level
//                     tree for buckets spanning more than 9 threads)
//   k_wsum_tree       bucket reduction: F_w = sum_b (b+1) S_b = sum_j acc_j + L sum_j j T_j with
//                     running sums over segments of L buckets (acc_j, T_j), then sum_j j T_j =
//                     sum_k 2^k U_k, U_k = sum_{j : bit k of j} T_j, as a subset-sum tree over each
//                     block's 256 segments in LDS (round 3; k_wsum + k_group_sum(_q) below for
//                     windows of fewer than 256 segments)
//   k_group_fin       the blocks' partial sums -> A and U_k per window
//   host              ONE Horner over every (window, bit) exponent -> affine, see host_ec.hpp
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "curve.hpp"
#include "curve29.hpp"
#include "glv.hpp"
#include "host_ec.hpp"
#include "msm.hpp"
#include "msm_batch.hpp"
#include "quad.hpp"
#include "runtime.hpp"

namespace sv {

// (kBlock and the other constants the host's buffer sizes depend on: msm_plan.hpp)
#ifndef SV_ACC_PREFETCH
// next entry index loaded a step ahead.  0 (none) and 2 (next point too -- 162 VGPRs, no gain) apply
// to the 32-bit chain only: the 29-bit chain is written for 1 (the static_assert in k_accumulate)
#define SV_ACC_PREFETCH 1
#endif

__device__ __forceinline__ G1Aff load_aff(const G1Aff* __restrict__ a, uint32_t i) {
  const uint4* p = reinterpret_cast<const uint4*>(a + i);
  uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
  G1Aff r;
  r.x.v[0] = q0.x; r.x.v[1] = q0.y; r.x.v[2] = q0.z; r.x.v[3] = q0.w;
  r.x.v[4] = q1.x; r.x.v[5] = q1.y; r.x.v[6] = q1.z; r.x.v[7] = q1.w;
  r.y.v[0] = q2.x; r.y.v[1] = q2.y; r.y.v[2] = q2.z; r.y.v[3] = q2.w;
  r.y.v[4] = q3.x; r.y.v[5] = q3.y; r.y.v[6] = q3.z; r.y.v[7] = q3.w;
  return r;
}

// virtual point idx: P_idx, or phi(P_(idx - nsplit)) = (beta x, y) for a GLV k2 entry (nsplit = n;
// ~0u without GLV): x from the beta-x table, y from the bases
// (phi64: the table holds whole phi(P) records, 64 B, one gather per entry)
__device__ __forceinline__ G1Aff load_vpoint(const G1Aff* __restrict__ bases, const uint4* __restrict__ phix,
                                             uint32_t idx, uint32_t nsplit, int phi64) {
  const bool ph = idx >= nsplit;
  const uint32_t i = ph ? idx - nsplit : idx;
  const uint4* p = reinterpret_cast<const uint4*>(bases + i);
  const uint4* px = ph ? phix + (phi64 ? 4 : 2) * i : p;
  const uint4* py = ph && phi64 ? px : p;
  const uint4 q0 = px[0], q1 = px[1], q2 = py[2], q3 = py[3];
  G1Aff r;
  r.x.v[0] = q0.x; r.x.v[1] = q0.y; r.x.v[2] = q0.z; r.x.v[3] = q0.w;
  r.x.v[4] = q1.x; r.x.v[5] = q1.y; r.x.v[6] = q1.z; r.x.v[7] = q1.w;
  r.y.v[0] = q2.x; r.y.v[1] = q2.y; r.y.v[2] = q2.z; r.y.v[3] = q2.w;
  r.y.v[4] = q3.x; r.y.v[5] = q3.y; r.y.v[6] = q3.z; r.y.v[7] = q3.w;
  return r;
}

__device__ __forceinline__ G1Xyzz load_xyzz(const G1Xyzz* __restrict__ a, uint32_t i) {
  const uint4* p = reinterpret_cast<const uint4*>(a + i);
  G1Xyzz r;
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint4 q = p[k];
    d[4 * k + 0] = q.x; d[4 * k + 1] = q.y; d[4 * k + 2] = q.z; d[4 * k + 3] = q.w;
  }
  return r;
}

__device__ __forceinline__ void store_xyzz(G1Xyzz* __restrict__ a, uint32_t i, const G1Xyzz& v) {
  uint4* p = reinterpret_cast<uint4*>(a + i);
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < 8; k++) p[k] = make_uint4(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
}

// Bucket-sum records (bsum, pfirst, plast).  The 32-bit chain stores canonical G1Xyzz (128 B).  The
// 29-bit chain (round 6) stores its own state as it is: 4 x 9 limbs, 144 B, X below 8p -- a segment
// end is nine 16-B stores and no conversion (round 4-5 packed the limbs into 8-word x R' values
// after a conditional subtraction of 4p: ~110 VALU instructions in the accumulate's divergent
// segment-end block, i.e. ~70 per bucket entry at 2^20).  The readers convert once per bucket.
// In a record the identity is ZZ == 0 only; its other limbs are arbitrary (a cancelled chain zeroes
// ZZ and stores X, Y, ZZZ as they were), so st_rec29 / ld_rec29 move the limbs as they are and every
// reader tests ZZ alone (r29::is_identity; tests/f29_cases.py's garbage-identity cases).
// Arrays stay typed G1Xyzz*: rec_at gives record i of either form.
// (kRec29Words, bucket_rec_bytes: msm_plan.hpp)
template <class T>
__host__ __device__ __forceinline__ T* rec_at(T* base, size_t i, int r29) {
  using U = typename std::conditional<std::is_const<T>::value, const uint32_t, uint32_t>::type;
  return r29 ? reinterpret_cast<T*>(reinterpret_cast<U*>(base) + kRec29Words * i) : base + i;
}
__device__ __forceinline__ void st_rec29(G1Xyzz* __restrict__ base, size_t i, const r29::Xyzz& a) {
  uint4* o = reinterpret_cast<uint4*>(rec_at(base, i, 1));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&a);
#pragma unroll
  for (int k = 0; k < 9; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
__device__ __forceinline__ r29::Xyzz ld_rec29(const G1Xyzz* __restrict__ base, size_t i) {
  const uint4* o = reinterpret_cast<const uint4*>(rec_at(base, i, 1));
  r29::Xyzz a;
  uint32_t* w = reinterpret_cast<uint32_t*>(&a);
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const uint4 q = o[k];
    w[4 * k] = q.x, w[4 * k + 1] = q.y, w[4 * k + 2] = q.z, w[4 * k + 3] = q.w;
  }
  return a;
}
// one coordinate (0..3: X, Y, ZZ, ZZZ) of a 29-bit record in field.hpp's canonical x R form
__device__ __forceinline__ Fq rec29_coord_canonical(const G1Xyzz* __restrict__ rec, int c) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(rec) + r29::L * c;
  r29::F f;
#pragma unroll
  for (int i = 0; i < r29::L; i++) f.v[i] = w[i];
  Fq r;
  r29::to_r32(r29::csub<4>(f), r.v);  // X below 8p; the others below 2p (csub leaves them)
  return r;
}
__device__ __forceinline__ void rec29_coord_store(G1Xyzz* __restrict__ rec, int c, const Fq& canon) {
  const r29::F f = r29::to_r29(canon.v);  // below 2p
  uint32_t* w = reinterpret_cast<uint32_t*>(rec) + r29::L * c;
#pragma unroll
  for (int i = 0; i < r29::L; i++) w[i] = f.v[i];
}
__device__ __forceinline__ G1Xyzz load_bucket(const G1Xyzz* __restrict__ a, uint32_t i, int r29w) {
  if (!r29w) return load_xyzz(a, i);
  const G1Xyzz* rec = rec_at(a, i, 1);
  return {rec29_coord_canonical(rec, 0), rec29_coord_canonical(rec, 1), rec29_coord_canonical(rec, 2),
          rec29_coord_canonical(rec, 3)};
}
// store a canonical sum into record i of either form
__device__ __forceinline__ void store_bucket(G1Xyzz* __restrict__ a, uint32_t i, const G1Xyzz& v, int r29w) {
  if (!r29w) {
    store_xyzz(a, i, v);
    return;
  }
  G1Xyzz* rec = rec_at(a, i, 1);
  rec29_coord_store(rec, 0, v.X);
  rec29_coord_store(rec, 1, v.Y);
  rec29_coord_store(rec, 2, v.ZZ);
  rec29_coord_store(rec, 3, v.ZZZ);
}

// ---------------------------------------------------------------------------------------------
__global__ void k_to_mont_bases(const G1Aff* __restrict__ in, G1Aff* __restrict__ out, uint32_t n,
                                uint32_t* __restrict__ err) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Aff a = load_aff(in, i);
  if (!a.x.is_reduced() || !a.y.is_reduced()) atomicOr(err, 1u);
  G1Aff r;
  if (a.is_identity()) {
    r = a;
  } else {
    r.x = fe_to_mont(a.x);
    r.y = fe_to_mont(a.y);
  }
  reinterpret_cast<uint4*>(out + i)[0] = make_uint4(r.x.v[0], r.x.v[1], r.x.v[2], r.x.v[3]);
  reinterpret_cast<uint4*>(out + i)[1] = make_uint4(r.x.v[4], r.x.v[5], r.x.v[6], r.x.v[7]);
  reinterpret_cast<uint4*>(out + i)[2] = make_uint4(r.y.v[0], r.y.v[1], r.y.v[2], r.y.v[3]);
  reinterpret_cast<uint4*>(out + i)[3] = make_uint4(r.y.v[4], r.y.v[5], r.y.v[6], r.y.v[7]);
}

// Signed windows: digit_w = bits[cw, cw+c) + carry, mapped to (-2^(c-1), 2^(c-1)].  W = ceil(NB/c)
// windows so the top digit never carries out: NB = 255 for full scalars (< r < 2^254), NB = 128 for
// GLV halves (magnitude < 2^127).  f(w, mag, neg) per window.
template <int C, int NB>
__host__ __device__ constexpr int num_windows() { return (NB + C - 1) / C; }
template <int C, int NB = 255, class F>
__device__ __forceinline__ void for_each_digit(const Fr& s, F&& f) {
  constexpr int W = num_windows<C, NB>();
  uint32_t carry = 0;
  const uint32_t half = 1u << (C - 1);
  const uint32_t mask = (1u << C) - 1;
#pragma unroll
  for (int w = 0; w < W; w++) {
    const int pos = w * C;
    const int limb = pos >> 5, off = pos & 31;
    const uint32_t lo = limb < 8 ? s.v[limb] : 0;
    const uint32_t hi = (limb + 1) < 8 ? s.v[limb + 1] : 0;
    uint32_t bits = off ? ((lo >> off) | (hi << (32 - off))) : lo;
    bits = (bits & mask) + carry;
    if (bits > half) {
      // digit = bits - 2^C <= 0; bits == 2^C (all-ones window + carry) is digit 0 with carry 1
      f(w, (1u << C) - bits, 1u);
      carry = 1;
    } else {
      f(w, bits, 0u);
      carry = 0;
    }
  }
}

__device__ __forceinline__ Fr scalar_in(const uint4 q0, const uint4 q1, int mont_in, uint32_t* __restrict__ err) {
  Fr s;
  s.v[0] = q0.x; s.v[1] = q0.y; s.v[2] = q0.z; s.v[3] = q0.w;
  s.v[4] = q1.x; s.v[5] = q1.y; s.v[6] = q1.z; s.v[7] = q1.w;
  if (err && !s.is_reduced()) atomicOr(err, 2u);
  return mont_in ? fe_from_mont(s) : s;
}
__device__ __forceinline__ Fr load_scalar(const Fr* __restrict__ scalars, uint32_t i, int mont_in,
                                          uint32_t* __restrict__ err) {
  const uint4* p = reinterpret_cast<const uint4*>(scalars + i);
  const uint4 q0 = p[0], q1 = p[1];
  Fr s;
  s.v[0] = q0.x; s.v[1] = q0.y; s.v[2] = q0.z; s.v[3] = q0.w;
  s.v[4] = q1.x; s.v[5] = q1.y; s.v[6] = q1.z; s.v[7] = q1.w;
  if (err && !s.is_reduced()) atomicOr(err, 2u);
  return mont_in ? fe_from_mont(s) : s;
}

// Entries of real point i for the sort passes.  Without GLV: the W signed digits of its scalar,
// all for virtual point i (half 0).  With GLV the scalar is split here (glv.hpp; the halves
// are stored for the scatter pass on the device path, see store()): the W digits of k1 belong to virtual point i (P_i, half 0) and the W digits of k2 to
// virtual point n + i (phi(P_i), half 1), each half's sign folded into its digits' signs; both
// halves share the W windows' buckets.  f(w, mag, neg, half) per digit.
template <int C, bool GLV>
struct Digits {
  static constexpr int NB = GLV ? 128 : 255;
  static constexpr int W = num_windows<C, NB>();
  static constexpr int EP = GLV ? 2 * W : W;  // entries per real point
  uint32_t h[GLV ? 2 : 1][GLV ? 4 : 8];
  uint32_t sgn[GLV ? 2 : 1];
  __device__ __forceinline__ void load(const Fr* __restrict__ scalars, uint32_t i, int mont_in,
                                       uint32_t* __restrict__ err) {
    from(load_scalar(scalars, i, mont_in, err));
  }
  __device__ __forceinline__ void from(const Fr& s) {
    if constexpr (GLV) {
      uint32_t h1[4], h2[4];
      glv_split(s.v, h1, h2);
#pragma unroll
      for (int k = 0; k < 4; k++) h[0][k] = h1[k], h[1][k] = h2[k];
#pragma unroll
      for (int q = 0; q < 2; q++) {
        sgn[q] = h[q][3] >> 31;
        h[q][3] &= 0x7fffffffu;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) h[0][k] = s.v[k];
      sgn[0] = 0;
    }
  }
  // The histogram pass stores what load() derived (GLV: both halves, the sign in bit 31 of the top
  // word; else the canonical scalar): 32 B per point, so the scatter pass reads it back instead of
  // converting from Montgomery form and splitting again (SVGPU_SORT_HALVES=0: recompute, as before)
  __device__ __forceinline__ void store(uint4* __restrict__ hv, uint32_t i) const {
    if constexpr (GLV) {
      hv[2 * i] = make_uint4(h[0][0], h[0][1], h[0][2], h[0][3] | (sgn[0] << 31));
      hv[2 * i + 1] = make_uint4(h[1][0], h[1][1], h[1][2], h[1][3] | (sgn[1] << 31));
    } else {
      hv[2 * i] = make_uint4(h[0][0], h[0][1], h[0][2], h[0][3]);
      hv[2 * i + 1] = make_uint4(h[0][4], h[0][5], h[0][6], h[0][7]);
    }
  }
  __device__ __forceinline__ void load_stored(const uint4* __restrict__ hv, uint32_t i) {
    const uint4 a = hv[2 * i], b = hv[2 * i + 1];
    if constexpr (GLV) {
      h[0][0] = a.x; h[0][1] = a.y; h[0][2] = a.z; h[0][3] = a.w & 0x7fffffffu;
      h[1][0] = b.x; h[1][1] = b.y; h[1][2] = b.z; h[1][3] = b.w & 0x7fffffffu;
      sgn[0] = a.w >> 31;
      sgn[1] = b.w >> 31;
    } else {
      h[0][0] = a.x; h[0][1] = a.y; h[0][2] = a.z; h[0][3] = a.w;
      h[0][4] = b.x; h[0][5] = b.y; h[0][6] = b.z; h[0][7] = b.w;
      sgn[0] = 0;
    }
  }
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
    for (int q = 0; q < (GLV ? 2 : 1); q++) {
      Fr s;
      if constexpr (GLV) {
#pragma unroll
        for (int k = 0; k < 4; k++) s.v[k] = h[q][k], s.v[4 + k] = 0u;
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) s.v[k] = h[0][k];
      }
      const uint32_t sg = sgn[q];
      for_each_digit<C, NB>(s, [&](int w, uint32_t mag, uint32_t neg) { f(w, mag, neg ^ sg, (uint32_t)q); });
    }
  }
};

// GLV: phi(P_i) = (beta x_i, y_i); only beta x_i is stored (phix[i], 32 B, written by k_bin_hist),
// the accumulate reads y_i from the bases (identity (0, 0) maps to itself).  With err set the point's
// coordinates are checked to be reduced (Montgomery input is used as is by the 2p-domain adds).
__device__ __forceinline__ void glv_phix(const G1Aff* __restrict__ bases, uint32_t i, uint4* __restrict__ phix,
                                         int phi64, uint32_t* __restrict__ err) {
  const uint4* b = reinterpret_cast<const uint4*>(bases + i);
  Fq x, beta;
  const uint4 x0 = b[0], x1 = b[1];
  x.v[0] = x0.x; x.v[1] = x0.y; x.v[2] = x0.z; x.v[3] = x0.w;
  x.v[4] = x1.x; x.v[5] = x1.y; x.v[6] = x1.z; x.v[7] = x1.w;
#pragma unroll
  for (int j = 0; j < 8; j++) beta.v[j] = GLV_BETA_MONT[j];
  const Fq bx = x * beta;
  uint4* o = phix + (phi64 ? 4 : 2) * i;
  o[0] = make_uint4(bx.v[0], bx.v[1], bx.v[2], bx.v[3]);
  o[1] = make_uint4(bx.v[4], bx.v[5], bx.v[6], bx.v[7]);
  if (phi64 || err) {
    const uint4 y0 = b[2], y1 = b[3];
    if (phi64) {
      o[2] = y0;
      o[3] = y1;
    }
    if (err) {
      Fq y;
      y.v[0] = y0.x; y.v[1] = y0.y; y.v[2] = y0.z; y.v[3] = y0.w;
      y.v[4] = y1.x; y.v[5] = y1.y; y.v[6] = y1.z; y.v[7] = y1.w;
      if (!x.is_reduced() || !y.is_reduced()) atomicOr(err, 1u);
    }
  }
}

// Host-fed pieces: the piece's table once its bases have landed (its sort ran on the scalars alone)
__global__ void k_glv_phix(const G1Aff* __restrict__ bases, uint32_t n, uint4* __restrict__ phix, int phi64,
                           uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) glv_phix(bases, i, phix, phi64, err);
}

// The 29-bit chain's table of virtual points (p.r29, replaces phix): every record the chain's own
// limbs, x R' as 9 x 29-bit limbs for x then y (72 B, 9 uint2), so the accumulate's per-entry point
// load is the whole conversion -- converted once per point here instead of once per bucket entry
// (16 entries per point at 2^20).  Round 6: the limbs themselves (round 4-5 stored 8-word x R'
// values, 64 B, and split them into limbs per entry: ~35 VALU instructions per entry).  P_i at
// record i and, with GLV, phi(P_i) = (beta x_i, y_i) at record nsplit + i.  With err set the bases
// are checked to be reduced (Montgomery input is used as is).
static constexpr int kPhiVtab = 2;  // k_bin_hist's phi64 value for "phix is the r29 table"
static constexpr int kVtabRec = 9;  // uint2 per record
// The identity's record carries this bit in y's top limb, which a point never sets (y below 2p keeps
// that limb below 2^23), and is otherwise zero: k_accumulate, the table's only reader, tests the one
// limb instead of OR-ing all eighteen for every entry, and reads nothing else of such a record.
static constexpr uint32_t kVtabIdentity = 0x80000000u;
__device__ __forceinline__ void st_rec29(uint2* o, const r29::F& x, const r29::F& y) {
  o[0] = make_uint2(x.v[0], x.v[1]);
  o[1] = make_uint2(x.v[2], x.v[3]);
  o[2] = make_uint2(x.v[4], x.v[5]);
  o[3] = make_uint2(x.v[6], x.v[7]);
  o[4] = make_uint2(x.v[8], y.v[0]);
  o[5] = make_uint2(y.v[1], y.v[2]);
  o[6] = make_uint2(y.v[3], y.v[4]);
  o[7] = make_uint2(y.v[5], y.v[6]);
  o[8] = make_uint2(y.v[7], y.v[8]);
}
__device__ __forceinline__ void ld_rec29(const uint2* __restrict__ o, r29::F& x, r29::F& y) {
  uint2 q[kVtabRec];
#pragma unroll
  for (int k = 0; k < kVtabRec; k++) q[k] = o[k];
  x.v[0] = q[0].x, x.v[1] = q[0].y, x.v[2] = q[1].x, x.v[3] = q[1].y, x.v[4] = q[2].x, x.v[5] = q[2].y;
  x.v[6] = q[3].x, x.v[7] = q[3].y, x.v[8] = q[4].x;
  y.v[0] = q[4].y, y.v[1] = q[5].x, y.v[2] = q[5].y, y.v[3] = q[6].x, y.v[4] = q[6].y, y.v[5] = q[7].x;
  y.v[6] = q[7].y, y.v[7] = q[8].x, y.v[8] = q[8].y;
}
// (uint4 per point of the table: vtab_uint4_per_point, msm_plan.hpp)
__device__ __forceinline__ void vtab_put_pt(const G1Aff& a, uint32_t i, uint4* __restrict__ vtab, uint32_t nsplit,
                                            bool glv, uint32_t* __restrict__ err) {
  if (err && (!a.x.is_reduced() || !a.y.is_reduced())) atomicOr(err, 1u);
  r29::F y = r29::to_r29(a.y.v);  // below 2p
  const r29::F x = r29::to_r29(a.x.v);
  // the identity (all-zero limbs), tested here once per point and marked for the per-entry reader
  if (r29::is_zero(x) && r29::is_zero(y)) y.v[r29::L - 1] = kVtabIdentity;
  uint2* t = reinterpret_cast<uint2*>(vtab);
  st_rec29(t + kVtabRec * (size_t)i, x, y);
  if (glv) {  // beta x in the 29-bit form directly: beta R' (GLV_BETA_MONT re-expressed, 2^261)
    constexpr uint32_t kBeta29[r29::L] = {0xa337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu,
                                         0x176f16du, 0xeed93bau,  0x14291140u, 0xc0afeu};
    r29::F beta;
#pragma unroll
    for (int j = 0; j < r29::L; j++) beta.v[j] = kBeta29[j];
    st_rec29(t + kVtabRec * ((size_t)nsplit + i), r29::mul(x, beta), y);  // below 2p
  }
}
__device__ __forceinline__ void vtab_put(const G1Aff* __restrict__ bases, uint32_t i, uint4* __restrict__ vtab,
                                         uint32_t nsplit, bool glv, uint32_t* __restrict__ err) {
  vtab_put_pt(load_aff(bases, i), i, vtab, nsplit, glv, err);
}
// Host-fed pieces with the 29-bit chain: the piece's table once its bases have landed
__global__ void k_vtab(const G1Aff* __restrict__ bases, uint32_t n, uint4* __restrict__ vtab, int glv,
                       uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vtab_put(bases, i, vtab, n, glv != 0, err);
}

// Resident base set (msm_resident_prepare), once per set: rows in either form -> Montgomery rows
// (64 B per point, the small route's input) and the 29-bit table of the whole set, P_i at record i
// and phi(P_i) at record n + i for every set size (any call size may take the GLV plan); unreduced
// coordinates set the error flag.  in may equal out (a thread reads its row before it writes it), so
// neither is __restrict__.  n <= 2^26: record n + i stays below 2^27.
__global__ void __launch_bounds__(kBlock) k_resident_prepare(const G1Aff* in, G1Aff* out, uint32_t n, int mont_in,
                                                             uint4* __restrict__ vtab, uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Aff a;
  {
    const uint4* p = reinterpret_cast<const uint4*>(in + i);
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    a.x.v[0] = q0.x; a.x.v[1] = q0.y; a.x.v[2] = q0.z; a.x.v[3] = q0.w;
    a.x.v[4] = q1.x; a.x.v[5] = q1.y; a.x.v[6] = q1.z; a.x.v[7] = q1.w;
    a.y.v[0] = q2.x; a.y.v[1] = q2.y; a.y.v[2] = q2.z; a.y.v[3] = q2.w;
    a.y.v[4] = q3.x; a.y.v[5] = q3.y; a.y.v[6] = q3.z; a.y.v[7] = q3.w;
  }
  if (!a.x.is_reduced() || !a.y.is_reduced()) {
    atomicOr(err, 1u);
    a.x = Fq::zero();  // the set is discarded: keep the stored limbs in range all the same
    a.y = Fq::zero();
  }
  if (!mont_in && !a.is_identity()) {
    a.x = fe_to_mont(a.x);
    a.y = fe_to_mont(a.y);
  }
  uint4* o = reinterpret_cast<uint4*>(out + i);
  o[0] = make_uint4(a.x.v[0], a.x.v[1], a.x.v[2], a.x.v[3]);
  o[1] = make_uint4(a.x.v[4], a.x.v[5], a.x.v[6], a.x.v[7]);
  o[2] = make_uint4(a.y.v[0], a.y.v[1], a.y.v[2], a.y.v[3]);
  o[3] = make_uint4(a.y.v[4], a.y.v[5], a.y.v[6], a.y.v[7]);
  vtab_put_pt(a, i, vtab, n, true, nullptr);
}

// Montgomery-form bases that no other pass reads before the accumulate (no GLV table, host-fed)
__global__ void k_check_bases(const G1Aff* __restrict__ bases, uint32_t n, uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Aff a = load_aff(bases, i);
  if (!a.x.is_reduced() || !a.y.is_reduced()) atomicOr(err, 1u);
}

// ---- two-level counting sort of the n * W (point, digit) entries by bucket ------------------
// Bucket b = |digit| - 1 of window w splits into a coarse bin b >> FB (NBIN = 2^CB bins per window)
// and a fine index b & (2^FB - 1).  Pass 1 (k_bin_hist): per block of sort_chunk(c) points, every
// window's digits, LDS histogram of (window, bin).  Pass 2 (k_bin_scan_chunks, k_bin_scan): global
// offsets of every (window, bin, block) run.  Pass 3 (k_bin_scatter): the digits again (from the halves pass 1 stored), each
// entry appended to its block's run -> tmp (u64: fine << 32 | point | sign << 31); a block's runs
// are short contiguous spans, so writes merge in L2.  Pass 4 (k_fine_sort): one block per
// (window, bin) counting-sorts its ~n / NBIN entries by fine index inside that bin's region (L2
// resident), writes ent[], the global bucket offsets gst[] and the owner bucket tstart[t] of every
// accumulate chunk [tK, tK + K).  No per-(window, point) digit array is ever stored.
// points per block in passes 1 and 3: sort_chunk (msm_plan.hpp, with coarse_bits), 256 when the LDS
// staging of W digits per point would not fit (small c, many windows)
__host__ __device__ constexpr int ceil_log2(int x) { return x <= 1 ? 0 : 1 + ceil_log2((x + 1) / 2); }

// exclusive scan of x[0 .. N) in LDS by a 256-thread block (N <= 4096); returns the total
template <int N>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t* x, uint32_t* part) {
  constexpr int PER = (N + kBlock - 1) / kBlock;
  const int tid = threadIdx.x;
  uint32_t loc[PER];
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int k = tid * PER + j;
    loc[j] = k < N ? x[k] : 0u;
    sum += loc[j];
  }
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {
    const uint32_t u = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += u;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  const uint32_t total = part[kBlock - 1];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int k = tid * PER + j;
    if (k < N) x[k] = run;
    run += loc[j];
  }
  __syncthreads();
  return total;
}

// Coarse-binned entries (tmp[]): u64 fine << 32 | point | sign << 31, or -- when the virtual
// point index fits in 31 - FB bits (every size up to 2^22 points) -- packed into u32 as
// fine << (32 - FB) | sign << (31 - FB) | point, which halves the scatter's writes and the fine
// sort's reads.  The fine sort expands either form to the u64 layout in registers.
__device__ __forceinline__ uint32_t pack_entry32(uint32_t fine, uint32_t neg, uint32_t pt, uint32_t fb) {
  return (fb ? fine << (32 - fb) : 0u) | (neg << (31 - fb)) | pt;
}
__device__ __forceinline__ uint64_t load_entry(const uint64_t* __restrict__ tmp, uint32_t i, int e32, uint32_t fb) {
  if (!e32) return tmp[i];
  const uint32_t v = reinterpret_cast<const uint32_t*>(tmp)[i];
  const uint32_t fine = fb ? v >> (32 - fb) : 0u, neg = (v >> (31 - fb)) & 1u, pt = v & ((1u << (31 - fb)) - 1u);
  return ((uint64_t)fine << 32) | pt | (neg << 31);
}

// Logical block of the histogram / scatter passes.  Workgroups are dispatched round-robin over the
// 8 XCDs, so consecutive blocks sit on different L2s; both passes store per-block counts column-wise
// (bcnt[key * nblk + blk], 32 blocks per 128-B line) and runs of consecutive blocks side by side in
// tmp, and a line filled from 8 L2s is written back 8 times, partially.  xcd != 0 gives each XCD a
// contiguous range of logical blocks instead (a bijection; the tail n % 8 blocks keep their index).
__device__ __forceinline__ uint32_t sort_block(uint32_t b, uint32_t n, int xcd) {
  const uint32_t nfull = n & ~7u;
  if (!xcd || b >= nfull) return b;
  return (b & 7u) * (nfull >> 3) + (b >> 3);
}

// With GLV the pass also writes the beta-x table of its points (phix, see glv_phix).
template <int C, bool GLV>
__global__ void __launch_bounds__(kBlock) k_bin_hist(const Fr* __restrict__ scalars, uint32_t n, int mont_in,
                                                     uint32_t nblk, uint32_t* __restrict__ bcnt,
                                                     uint32_t* __restrict__ err, const G1Aff* __restrict__ bases,
                                                     uint4* __restrict__ phix, int phi64, int check_bases,
                                                     int xcd, int bm, uint32_t w0, uint32_t nw,
                                                     uint4* __restrict__ stored, int pf) {
  using D = Digits<C, GLV>;
  constexpr int W = D::W, LOGB = C - 1;
  constexpr int CB = coarse_bits(C, D::NB), FB = LOGB - CB, NBIN = 1 << CB;
  // windows [w0, w0 + nw) only (the MSM's window halves are sorted separately, see msm_run_impl):
  // keys (w - w0) * NBIN + bin
  const uint32_t nk = nw * NBIN;
  __shared__ uint32_t h[W * NBIN];
  for (int k = threadIdx.x; k < W * NBIN; k += kBlock) h[k] = 0;
  __syncthreads();
  constexpr uint32_t CH = sort_chunk(D::EP);
  const uint32_t blk = sort_block(blockIdx.x, gridDim.x, xcd);
  const uint32_t lo = blk * CH, hi = min(n, lo + CH);
  auto count = [&](const D& d) {
    d.each([&](int w, uint32_t mag, uint32_t, uint32_t) {
      if (mag && (uint32_t)w - w0 < nw) atomicAdd(&h[(w - w0) * NBIN + ((mag - 1) >> FB)], 1u);
    });
  };
  if (phix && phi64 == kPhiVtab && pf) {
    // Round 6: the 29-bit table path with the next point's scalar and base loaded one iteration
    // ahead (the pass is load-latency-bound: ~4 dependent iterations per thread at 4 waves/SIMD)
    uint32_t i = lo + threadIdx.x;
    const uint4* sp = reinterpret_cast<const uint4*>(scalars);
    const uint4* bp = reinterpret_cast<const uint4*>(bases);
    uint4 s0{}, s1{}, b0{}, b1{}, b2{}, b3{};
    if (i < hi) {
      s0 = sp[2 * (size_t)i], s1 = sp[2 * (size_t)i + 1];
      b0 = bp[4 * (size_t)i], b1 = bp[4 * (size_t)i + 1], b2 = bp[4 * (size_t)i + 2], b3 = bp[4 * (size_t)i + 3];
    }
    for (; i < hi; i += kBlock) {
      G1Aff a;
      a.x.v[0] = b0.x; a.x.v[1] = b0.y; a.x.v[2] = b0.z; a.x.v[3] = b0.w;
      a.x.v[4] = b1.x; a.x.v[5] = b1.y; a.x.v[6] = b1.z; a.x.v[7] = b1.w;
      a.y.v[0] = b2.x; a.y.v[1] = b2.y; a.y.v[2] = b2.z; a.y.v[3] = b2.w;
      a.y.v[4] = b3.x; a.y.v[5] = b3.y; a.y.v[6] = b3.z; a.y.v[7] = b3.w;
      const uint4 c0 = s0, c1 = s1;
      const uint32_t j = i + kBlock;
      if (j < hi) {
        s0 = sp[2 * (size_t)j], s1 = sp[2 * (size_t)j + 1];
        b0 = bp[4 * (size_t)j], b1 = bp[4 * (size_t)j + 1], b2 = bp[4 * (size_t)j + 2], b3 = bp[4 * (size_t)j + 3];
      }
      vtab_put_pt(a, i, phix, n, GLV, check_bases ? err : nullptr);
      D d;
      d.from(scalar_in(c0, c1, mont_in, err));
      if (stored) d.store(stored, i);
      count(d);
    }
  } else
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) {
    // Montgomery bases are checked here (canonical ones by k_to_mont_bases)
    if (phix && phi64 == kPhiVtab) {  // the 29-bit chain's table (n = nsplit on the device path)
      vtab_put(bases, i, phix, n, GLV, check_bases ? err : nullptr);
    } else if constexpr (GLV) {
      if (phix) glv_phix(bases, i, phix, phi64, check_bases ? err : nullptr);  // (null: bases not landed yet, k_glv_phix later)
    } else {
      if (check_bases) {
        const G1Aff a = load_aff(bases, i);
        if (!a.x.is_reduced() || !a.y.is_reduced()) atomicOr(err, 1u);
      }
    }
    D d;
    d.load(scalars, i, mont_in, err);
    if (stored) d.store(stored, i);
    count(d);
  }
  __syncthreads();
  // bm: block-major bcnt[blk * nk + key], one contiguous row per block (the scan reads it in
  // 32-key tiles); else key-major bcnt[key * nblk + blk] (round 2)
  for (uint32_t k = threadIdx.x; k < nk; k += kBlock)
    bcnt[bm ? (size_t)blk * nk + k : (size_t)k * nblk + blk] = h[k];
}

// one 256-thread block per (window, bin): exclusive scan over blocks in place, total -> btot
__global__ void __launch_bounds__(kBlock) k_bin_scan_chunks(uint32_t* __restrict__ bcnt, uint32_t nblk,
                                                            uint32_t* __restrict__ btot) {
  __shared__ uint32_t part[kBlock];
  uint32_t* c = bcnt + (size_t)blockIdx.x * nblk;
  const uint32_t tid = threadIdx.x, per = (nblk + kBlock - 1) / kBlock;
  const uint32_t lo = min(nblk, tid * per), hi = min(nblk, lo + per);
  uint32_t sum = 0;
  for (uint32_t b = lo; b < hi; b++) sum += c[b];
  part[tid] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < kBlock; off <<= 1) {
    const uint32_t u = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += u;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  for (uint32_t b = lo; b < hi; b++) {
    const uint32_t v = c[b];
    c[b] = run;
    run += v;
  }
  if (tid == kBlock - 1) btot[blockIdx.x] = part[kBlock - 1];
}

// Block-major counts (bcnt[blk * nk + key]): one 1024-thread block per 32 keys.  Thread (grp, kk)
// walks rows grp * per .. of key 32 tile + kk, so each row access of a wave reads or writes two whole
// 128-B lines; exclusive scan over blocks in place, total -> btot.
template <int KT>  // keys per tile (32 or 16): 1024 / KT row groups per block
__global__ void __launch_bounds__(1024) k_bin_scan_tiles(uint32_t* __restrict__ bcnt, uint32_t nblk, uint32_t nk,
                                                         uint32_t* __restrict__ btot) {
  constexpr int G = 1024 / KT;
  __shared__ uint32_t part[G][KT + 1];
  const uint32_t kk = threadIdx.x % KT, grp = threadIdx.x / KT, key = blockIdx.x * KT + kk;
  const uint32_t per = (nblk + G - 1) / G, lo = min(nblk, grp * per), hi = min(nblk, lo + per);
  const bool live = key < nk;
  uint32_t* c = bcnt + key;
  uint32_t sum = 0;
  if (live) {
#pragma unroll 8
    for (uint32_t b = lo; b < hi; b++) sum += c[(size_t)b * nk];
  }
  part[grp][kk] = sum;
  __syncthreads();
  if (threadIdx.x < KT) {  // per key: exclusive scan over the G row groups
    uint32_t run = 0;
    for (int g = 0; g < G; g++) {
      const uint32_t v = part[g][threadIdx.x];
      part[g][threadIdx.x] = run;
      run += v;
    }
    if (blockIdx.x * KT + threadIdx.x < nk) btot[blockIdx.x * KT + threadIdx.x] = run;
  }
  __syncthreads();
  if (live) {
    uint32_t run = part[grp][kk];
#pragma unroll 8
    for (uint32_t b = lo; b < hi; b++) {
      const uint32_t v = c[(size_t)b * nk];
      c[(size_t)b * nk] = run;
      run += v;
    }
  }
}

// one 1024-thread block: exclusive scan of btot over all (window, bin) -> bstart; bstart[nwb] = total
__global__ void __launch_bounds__(1024) k_bin_scan(const uint32_t* __restrict__ btot, uint32_t nwb,
                                                   uint32_t* __restrict__ bstart, uint32_t* __restrict__ gst_end) {
  __shared__ uint32_t part[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (nwb + 1023) / 1024;
  const uint32_t lo = min(nwb, tid * per), hi = min(nwb, lo + per);
  uint32_t s = 0;
  for (uint32_t k = lo; k < hi; k++) s += btot[k];
  part[tid] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - s;
  for (uint32_t k = lo; k < hi; k++) {
    bstart[k] = run;
    run += btot[k];
  }
  if (tid == 1023) {
    bstart[nwb] = part[1023];
    *gst_end = part[1023];  // gst[nbt]: the entry total (k_fine_sort writes the other bucket starts)
  }
}

// Pass 3: the block's entries are first placed in LDS grouped by (window, bin), then each group
// is copied to its global run with consecutive lanes writing consecutive addresses.  Entry point
// index: the virtual point's table record, p_off + i, or phi_off + i for a GLV k2 digit (0 and n
// for a table of this sort's own points; a resident base set's offset and phi stride otherwise).
// The block's own (window, bin) counts
// are not recounted: they are the differences of consecutive block offsets that k_bin_scan_chunks
// left in bcnt (btot for the last block), which halves the LDS atomics of the pass.
template <int C, bool GLV>
__global__ void __launch_bounds__(kBlock) k_bin_scatter(const Fr* __restrict__ scalars, uint32_t n, int mont_in,
                                                        uint32_t nblk, const uint32_t* __restrict__ bcnt,
                                                        const uint32_t* __restrict__ btot,
                                                        const uint32_t* __restrict__ bstart,
                                                        uint64_t* __restrict__ tmp, int e32, int xcd, int bm,
                                                        uint32_t w0, uint32_t nw, const uint4* __restrict__ stored,
                                                        uint32_t p_off, uint32_t phi_off) {
  using D = Digits<C, GLV>;
  constexpr int W = D::W, LOGB = C - 1;
  constexpr int CB = coarse_bits(C, D::NB), FB = LOGB - CB, NBIN = 1 << CB, NK = W * NBIN;
  const uint32_t nk = nw * NBIN;  // keys of windows [w0, w0 + nw), (w - w0) * NBIN + bin
  // staged entry: local point (LP bits) | half << LP | sign << (LP + 1) | fine << (LP + 2) | (window, bin) key << (LP + 2 + FB)
  constexpr int LP = ceil_log2((int)sort_chunk(D::EP));
  static_assert(LP + 2 + FB + ceil_log2(NK) <= 32, "staged entry overflows 32 bits");
  constexpr uint32_t FMASK = (1u << FB) - 1;
  constexpr uint32_t CH = sort_chunk(D::EP), PT = CH / kBlock;
  __shared__ uint32_t off[NK];   // local group offsets
  __shared__ uint32_t cur[NK];   // cursors
  __shared__ uint32_t part[kBlock];
  __shared__ uint32_t stage[CH * D::EP];  // see the layout above (no separate key array: 3 blocks per CU)
  const uint32_t blk = sort_block(blockIdx.x, gridDim.x, xcd), lo = blk * CH, hi = min(n, lo + CH);
  for (uint32_t k = threadIdx.x; k < NK; k += kBlock) {
    if (k >= nk) {
      off[k] = 0;
      continue;
    }
    const size_t at = bm ? (size_t)blk * nk + k : (size_t)k * nblk + blk;
    off[k] = (blk + 1 < nblk ? bcnt[bm ? at + nk : at + 1] : btot[k]) - bcnt[at];
  }
  D dg[PT];
#pragma unroll
  for (int j = 0; j < (int)PT; j++) {
    const uint32_t i = lo + threadIdx.x + j * kBlock;
    if (i < hi) {
      if (stored) dg[j].load_stored(stored, i);  // written by this sort's k_bin_hist
      else dg[j].load(scalars, i, mont_in, nullptr);
    }
  }
  __syncthreads();
  const uint32_t total = block_excl_scan<NK>(off, part);
  for (int k = threadIdx.x; k < NK; k += kBlock) cur[k] = off[k];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < (int)PT; j++) {
    const uint32_t li = threadIdx.x + j * kBlock;
    if (lo + li < hi) {
      dg[j].each([&](int w, uint32_t mag, uint32_t neg, uint32_t half) {
        if (mag && (uint32_t)w - w0 < nw) {
          const uint32_t b = mag - 1;
          const uint32_t k = (w - w0) * NBIN + (b >> FB);
          const uint32_t pos = atomicAdd(&cur[k], 1u);
          stage[pos] = li | (half << LP) | (neg << (LP + 1)) | ((b & FMASK) << (LP + 2)) | (k << (LP + 2 + FB));
        }
      });
    }
  }
  __syncthreads();
  // global position of local slot x = gbase[key] + x  (cur[] reused for gbase)
  for (uint32_t k = threadIdx.x; k < nk; k += kBlock)
    cur[k] = bstart[k] + bcnt[bm ? (size_t)blk * nk + k : (size_t)k * nblk + blk] - off[k];
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < total; x += kBlock) {
    const uint32_t e = stage[x];
    const uint32_t pt = lo + (e & ((1u << LP) - 1u)) + (((e >> LP) & 1u) ? phi_off : p_off);
    const uint32_t dst = cur[e >> (LP + 2 + FB)] + x, fine = (e >> (LP + 2)) & FMASK, neg = (e >> (LP + 1)) & 1u;
    if (e32) reinterpret_cast<uint32_t*>(tmp)[dst] = pack_entry32(fine, neg, pt, FB);
    else tmp[dst] = ((uint64_t)fine << 32) | pt | (neg << 31);
  }
}

// one block per (window, bin): counting sort by the fine index within the bin's region.
// Regions of up to kFineCap entries (every bin but the short top window's at n = 2^20) are read
// from tmp ONCE into registers and sorted into an LDS copy of the region, which is then written to
// ent[] with consecutive lanes on consecutive addresses: the direct scatter of 4-byte entries to
// global memory cost ~5x its bytes in partial-line write traffic (PMC WRITE_SIZE, r01).  Larger
// regions are processed in LDS chunks of the same size (below); the two cases are separate
// instantiations (BIG), each block leaving at once unless its region is of its kind, so the staged
// one keeps to <= 64 VGPRs (two 1024-thread blocks per CU).
static constexpr uint32_t kFineR = 18;                 // entries per thread held in registers
static constexpr uint32_t kFineCap = 1024 * kFineR;    // region entries staged in LDS
static constexpr uint32_t kChunkR = 12, kChunk = 1024 * kChunkR;  // large regions: LDS chunk
static constexpr size_t kFineLds = (512 + 1024 + (size_t)kFineCap) * 4;  // 78 KiB: 2 blocks per CU
// MODE 0: staged regions only, 1: large regions only, 2 (round 3, default): both kinds in ONE launch,
// blocks in reverse (window, bin) order -- the crowded regions are the top window's, and as the
// launch's first blocks they run beside the small regions instead of as a separate serial launch
// (two launches: 37 + 35 us at 2^20, the large one a tail of a few dozen long blocks).
// one region (window, bin) = wb: staged in LDS whole (STAGED) or in chunks
template <bool STAGED>
__device__ __forceinline__ void fine_region(const uint64_t* __restrict__ tmp, int e32, uint32_t wb, uint32_t s0,
                                            uint32_t s1, uint32_t FB, uint32_t K, uint32_t* __restrict__ gst,
                                            uint32_t* __restrict__ tstart, uint32_t* __restrict__ ent,
                                            uint32_t* fine_lds) {
  uint32_t* fc = fine_lds;           // [512] fine-bucket counters / cursors
  uint32_t* part = fine_lds + 512;   // [1024] scan partials
  uint32_t* out = fine_lds + 1536;   // [kFineCap] the sorted region
  const uint32_t tid = threadIdx.x, NF = 1u << FB, len = s1 - s0;
  for (uint32_t f = tid; f < NF; f += 1024) fc[f] = 0;
  __syncthreads();
  uint64_t x[kFineR];
  if constexpr (STAGED) {
#pragma unroll
    for (uint32_t r = 0; r < kFineR; r++) {
      const uint32_t i = tid + r * 1024;
      x[r] = i < len ? load_entry(tmp, s0 + i, e32, FB) : 0;
    }
#pragma unroll
    for (uint32_t r = 0; r < kFineR; r++)
      if (tid + r * 1024 < len) atomicAdd(&fc[(uint32_t)(x[r] >> 32)], 1u);
  } else {
    uint32_t e = s0 + tid;
    for (; e + 3 * 1024 < s1; e += 4 * 1024) {  // 4 loads in flight per thread
      const uint32_t f0 = (uint32_t)(load_entry(tmp, e, e32, FB) >> 32);
      const uint32_t f1 = (uint32_t)(load_entry(tmp, e + 1024, e32, FB) >> 32);
      const uint32_t f2 = (uint32_t)(load_entry(tmp, e + 2048, e32, FB) >> 32);
      const uint32_t f3 = (uint32_t)(load_entry(tmp, e + 3072, e32, FB) >> 32);
      atomicAdd(&fc[f0], 1u);
      atomicAdd(&fc[f1], 1u);
      atomicAdd(&fc[f2], 1u);
      atomicAdd(&fc[f3], 1u);
    }
    for (; e < s1; e += 1024) atomicAdd(&fc[(uint32_t)(load_entry(tmp, e, e32, FB) >> 32)], 1u);
  }
  __syncthreads();
  // exclusive scan of fc[0 .. NF) (NF <= 512)
  const uint32_t v = tid < NF ? fc[tid] : 0;
  part[tid] = v;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t u = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += u;
    __syncthreads();
  }
  if (tid < NF) {
    const uint32_t st = s0 + part[tid] - v, en = st + v;
    const uint32_t g = wb * NF + tid;  // global bucket = w * B + b
    gst[g] = st;
    fc[tid] = STAGED ? st - s0 : st;
    for (uint32_t t = (st + K - 1) / K; t * K < en; t++) tstart[t] = g;
  }
  __syncthreads();
  if constexpr (STAGED) {
#pragma unroll
    for (uint32_t r = 0; r < kFineR; r++)
      if (tid + r * 1024 < len) out[atomicAdd(&fc[(uint32_t)(x[r] >> 32)], 1u)] = (uint32_t)x[r];
    __syncthreads();
    for (uint32_t i = tid; i < len; i += 1024) ent[s0 + i] = out[i];
    return;
  }
  // Large region: chunks of kChunk entries (12 per thread: the instantiation stays <= 64 VGPRs), each counting-sorted in LDS (chunk-local counts lc,
  // starts ls) and written as one contiguous run per fine bucket at that bucket's global cursor fc.
  uint32_t* lc = part;  // chunk counts reuse the scan buffer's first 512 words ...
  uint32_t* ls = part + 512;  // ... and chunk-local starts its second half
  for (uint32_t c0 = s0; c0 < s1; c0 += kChunk) {
    const uint32_t clen = min(kChunk, s1 - c0);
    if (tid < NF) lc[tid] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kChunkR; r++) {
      const uint32_t i = tid + r * 1024;
      x[r] = i < clen ? load_entry(tmp, c0 + i, e32, FB) : 0;
      if (i < clen) atomicAdd(&lc[(uint32_t)(x[r] >> 32)], 1u);
    }
    __syncthreads();
    // exclusive scan of lc[0 .. NF) by one wave per 64 buckets + a serial pass over the 8 totals
    if (tid < NF) {
      uint32_t v2 = lc[tid], incl = v2;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o);
        if ((tid & 63) >= (uint32_t)o) incl += u;
      }
      ls[tid] = incl - v2;  // exclusive within the wave
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (uint32_t w = 0; w < NF; w += 64) {
        const uint32_t last = min(NF, w + 64) - 1;
        const uint32_t tot = ls[last] + lc[last];
        out[kFineCap - 8 + (w >> 6)] = run;  // per-wave offsets parked at the end of out[]
        run += tot;
      }
    }
    __syncthreads();
    uint32_t base_f = 0;
    if (tid < NF) base_f = ls[tid] + out[kFineCap - 8 + (tid >> 6)];
    __syncthreads();
    if (tid < NF) {
      ls[tid] = base_f;
      lc[tid] = base_f;  // lc becomes the chunk-local cursor
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kChunkR; r++)
      if (tid + r * 1024 < clen) out[atomicAdd(&lc[(uint32_t)(x[r] >> 32)], 1u)] = (uint32_t)x[r];
    __syncthreads();
    // 16 lanes per fine bucket run (a chunk holds ~kChunk / NF ~ 24 entries per bucket):
    // out[ls[f] .. lc[f]) -> ent[fc[f] ..), consecutive lanes on consecutive addresses
    for (uint32_t f = tid >> 4; f < NF; f += 64) {
      const uint32_t st = ls[f], cnt = lc[f] - st, dst = fc[f];
      for (uint32_t j = tid & 15; j < cnt; j += 16) ent[dst + j] = out[st + j];
    }
    __syncthreads();
    if (tid < NF) fc[tid] += lc[tid] - ls[tid];
    __syncthreads();
  }
}


// MODE 0: staged regions only, 1: large regions only, 2 (round 3, default): both kinds in ONE launch,
// blocks in reverse (window, bin) order -- the crowded regions are the top window's, and as the
// launch's first blocks they run beside the small regions instead of as a separate serial launch
// (two launches: 37 + 35 us at 2^20, the large one a tail of a few dozen long blocks).
template <int MODE>
__global__ void __launch_bounds__(1024) k_fine_sort(const uint64_t* __restrict__ tmp, int e32,
                                                    const uint32_t* __restrict__ bstart, uint32_t FB, uint32_t K,
                                                    uint32_t* __restrict__ gst, uint32_t* __restrict__ tstart,
                                                    uint32_t* __restrict__ ent) {
  extern __shared__ __attribute__((aligned(16))) uint32_t fine_lds[];
  const uint32_t wb = MODE == 2 ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const uint32_t s0 = bstart[wb], s1 = bstart[wb + 1];
  const bool big = s1 - s0 > kFineCap;  // block-uniform
  if (MODE != 1 && !big) fine_region<true>(tmp, e32, wb, s0, s1, FB, K, gst, tstart, ent, fine_lds);
  if (MODE != 0 && big) fine_region<false>(tmp, e32, wb, s0, s1, FB, K, gst, tstart, ent, fine_lds);
}

// Each thread: K consecutive sorted entries.  See file header.
// Bucket pieces: a bucket whose entries cross thread boundaries is split into an OWNER piece (the
// thread holding its first entry; always that thread's last segment) and HEAD pieces (a later
// thread's first segment).  A bucket of exactly two pieces inside one block -- nearly all of them
// for random scalars -- is joined here: the head goes to LDS, and after the barrier the owner adds
// it to the piece still in its registers (one extra addition per owner at the accumulate's full
// occupancy, no global round trip).  Every other crossing bucket keeps the global pieces
// (pfirst = a thread's first segment, plast = its last) and is queued for k_fixup.  Empty
// buckets are never written: k_wsum reads gst.
static constexpr uint32_t kFixSerial = 8;  // crossing buckets of more pieces: k_fixup's heavy blocks
__device__ __forceinline__ bool join_in_block(uint32_t gs, uint32_t ge, uint32_t K) {
  const uint32_t t0 = gs / K, t1 = (ge - 1) / K;
  return t1 == t0 + 1 && t0 / kBlock == t1 / kBlock;
}
// The accumulator of k_accumulate's chain.  R29 (default): 9 x 29-bit limbs (curve29.hpp; each
// partial product one v_mad_u64_u32 with no carry add, 125 VGPRs = 4 waves per SIMD), reading its
// points from a table already in its form (vtab_put: a limb split per load).  Its bucket sums are STORED in the
// chain's own Montgomery form, x R' as 8 words ("r29w": every coordinate is below 4p < 2^256), not
// converted to field.hpp's canonical x R: a segment end runs for the whole wave whenever one of its
// lanes ends a segment, so its work counts nearly every iteration (the conversion there cost ~70 us
// of a 1.39 ms accumulate).  The readers convert instead: k_fixup (loads and stores r29w, so bsum
// stays uniform for the next host-fed piece), bucket_at (k_wsum, k_wsum_tree<false>, once per
// bucket), and k_wsum_tree<true, true> runs its running sums in the same form (bucket_at29).
// SVGPU_ACC_R29=0 selects the 8 x 32-bit chain (xyzz_madd_2p_u), stored canonical.
#ifndef SV_ACC_MADD32
#define SV_ACC_MADD32 xyzz_madd_2p_u
#endif
template <bool R29>
struct AccChain;
template <>
struct AccChain<false> {
  using T = G1Xyzz;
  __device__ static T identity() { return G1Xyzz::identity(); }
  __device__ static T in(const G1Xyzz& a) { return a; }
  __device__ static G1Xyzz out(const T& a) { return xyzz_canon2p(a); }
  __device__ static T madd(const T& acc, const G1Aff& p, bool neg) {
    return SV_ACC_MADD32(acc, p.x, neg ? -p.y : p.y);
  }
};
template <>
struct AccChain<true> {
  using T = r29::Xyzz;
  __device__ static T identity() { return r29::identity(); }
  __device__ static T in(const G1Xyzz& a) {  // storage form: x R' as words (r29w_*)
    return {r29::from_words(a.X.v), r29::from_words(a.Y.v), r29::from_words(a.ZZ.v), r29::from_words(a.ZZZ.v)};
  }
  __device__ static G1Xyzz out(const T& a) {  // the chain's X may reach 8p: stored below 4p
    G1Xyzz r;
    r29::to_words(r29::csub<4>(a.X), r.X.v);
    r29::to_words(a.Y, r.Y.v);
    r29::to_words(a.ZZ, r.ZZ.v);
    r29::to_words(a.ZZZ, r.ZZZ.v);
    return r;
  }
  __device__ static G1Xyzz canonical(const T& a) {  // field.hpp's canonical x R form
    G1Xyzz r;
    r29::to_r32(r29::csub<4>(a.X), r.X.v);
    r29::to_r32(a.Y, r.Y.v);
    r29::to_r32(a.ZZ, r.ZZ.v);
    r29::to_r32(a.ZZZ, r.ZZZ.v);
    return r;
  }
  __device__ static T madd(const T& acc, const G1Aff& p, bool neg) {
    const r29::F x = r29::from_words(p.x.v), y = r29::from_words(p.y.v);  // the table's x R' words
    return r29::madd(acc, x, y, neg);
  }
};

// SV_ACC_MIN_BLOCKS / SV_ACC29_MIN_BLOCKS: resident 256-thread blocks per CU the register allocator
// must allow for the 8 x 32-bit / 29-bit chains (1: no constraint -- the 32-bit chain takes 144
// VGPRs = 3 waves per SIMD; 4: at most 128 VGPRs, which the 29-bit chain meets without spilling)
#ifndef SV_ACC_MIN_BLOCKS
#define SV_ACC_MIN_BLOCKS 1
#endif
#ifndef SV_ACC29_MIN_BLOCKS
#define SV_ACC29_MIN_BLOCKS 4
#endif
// NL (round 6, the 29-bit chain; the round-5 loop stays for the 32-bit chain only): the chain's state
// is never the identity -- a lane whose chain is empty (segment start, or after P + (-P)) takes its
// next point as the state in the loop's divergent segment-end block and skips that entry's madd, so
// the per-entry step is r29::madd_live with no identity test or identity-valued merge.
template <bool ADD, bool R29, int PF = SV_ACC_PREFETCH, bool NL = R29>  // (R29 implies NL)
__global__ void __launch_bounds__(kBlock, R29 ? SV_ACC29_MIN_BLOCKS : SV_ACC_MIN_BLOCKS) k_accumulate(
    const G1Aff* __restrict__ bases, const uint32_t* __restrict__ ent, const uint32_t* __restrict__ gst,
    const uint32_t* __restrict__ tstart, uint32_t nbt, uint32_t K, uint32_t T,
    G1Xyzz* __restrict__ bsum, G1Xyzz* __restrict__ pfirst, G1Xyzz* __restrict__ plast,
    uint32_t* __restrict__ multi, uint32_t* __restrict__ nmulti, uint32_t* __restrict__ heavy,
    uint32_t* __restrict__ nheavy, const uint4* __restrict__ phix, uint32_t nsplit, int phi64) {
  using A = AccChain<R29>;
  // head pieces for the in-block join: canonical G1Xyzz (32-bit chain) or 29-bit records (144 B)
  __shared__ G1Xyzz shead[R29 ? 1 : kBlock];
  __shared__ uint4 shead29[R29 ? 9 * kBlock : 1];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = gst[nbt];
  const uint32_t s0 = t * K;
  const bool active = t < T && s0 < m;
  // owner piece left in acc for the in-block join (g = its bucket), or none
  bool owner = false;
  uint32_t g = 0, gs = 0, ge = 0;
  G1Xyzz sum;  // the last segment's canonical sum (the owner piece's, for the join)
  typename A::T acc = A::identity();
  if (active) {
    const uint32_t e_end = min(s0 + K, m);
    g = tstart[t];
    gs = gst[g];
    ge = gst[g + 1];
    uint32_t seg_start = s0;
    bool first = true;
    // ADD (host-fed pieces after the first): a segment that starts its bucket -- the owner piece --
    // starts from the sum the earlier pieces left in bsum (identity-initialised) instead of the
    // identity, so every later join (in block, k_fixup) and store carries it: no extra addition
    bool empty = true;  // NL: the chain holds no point yet (acc is not read)
    if constexpr (ADD) {
      if (s0 == gs) {
        if constexpr (R29) {
          acc = ld_rec29(bsum, g);
          empty = r29::is_zero(acc.ZZ);
        } else {
          acc = A::in(load_xyzz(bsum, g));
        }
      }
    }
    uint32_t vnext = 0;
    if constexpr (PF >= 1) vnext = ent[s0];
    G1Aff pnext;
    if constexpr (PF >= 2) pnext = load_vpoint(bases, phix, vnext & 0x7fffffffu, nsplit, phi64);
    if constexpr (NL) {
      static_assert(R29 && PF == 1, "the restructured loop is the 29-bit chain's");
      (void)bases;
      (void)nsplit;
      (void)phi64;
      for (uint32_t e = s0; e < e_end; e++) {
        // the entry's point first: a segment starting here starts from it
        const uint32_t v = vnext;
        if (e + 1 < e_end) vnext = ent[e + 1];
        r29::F x, y;  // the table's limbs (the identity: kVtabIdentity in y's top limb)
        ld_rec29(reinterpret_cast<const uint2*>(phix) + (size_t)kVtabRec * (v & 0x7fffffffu), x, y);
        const bool live = (y.v[r29::L - 1] & kVtabIdentity) == 0, neg = (v & 0x80000000u) != 0;
        bool fresh = false;
        if (e >= ge || empty) {  // divergent: a segment ends here, or the chain is empty
          if (e >= ge) {  // segment [seg_start, ge) of bucket g ends inside this chunk
            // the state as it is (an empty chain has acc.ZZ == 0, set below / by madd_live's
            // cancellation: the identity)
            if (seg_start == gs) {
              st_rec29(bsum, g, acc);
            } else {  // head piece of a bucket owned by an earlier thread
              if (join_in_block(gs, ge, K)) st_rec29(reinterpret_cast<G1Xyzz*>(shead29), threadIdx.x, acc);
              else st_rec29(pfirst, t, acc);
            }
            first = false;
            do {
              g++;
              gs = ge;
              ge = gst[g + 1];
            } while (ge <= e);
            seg_start = e;
            empty = true;
            if constexpr (ADD) {
              acc = ld_rec29(bsum, g);
              empty = r29::is_zero(acc.ZZ);
            } else {
              acc.ZZ = r29::zero();
            }
          }
          if (empty && live) {
            acc = r29::start(x, y, neg);
            empty = false;
            fresh = true;
          }
        }
        if (live && !fresh) {
          int special = 0;
          acc = r29::madd_live(acc, x, y, neg, special);
          if (special) {  // rare, divergent: P + P, or P + (-P) (the chain restarts at its next point)
            if (special == 2) {
              acc = r29::dbl_start(x, y, neg);
            } else {
              acc.ZZ = r29::zero();  // a chain that ends empty stores the identity
              empty = true;
            }
          }
        }
      }
    } else
    for (uint32_t e = s0; e < e_end; e++) {
      if (e >= ge) {  // segment [seg_start, ge) of bucket g ends inside this chunk
        const G1Xyzz sum = A::out(acc);
        if (seg_start == gs) {
          store_xyzz(bsum, g, sum);
        } else {  // head piece of a bucket owned by an earlier thread
          if (join_in_block(gs, ge, K)) shead[threadIdx.x] = sum;
          else store_xyzz(pfirst, t, sum);
        }
        first = false;
        do {
          g++;
          gs = ge;
          ge = gst[g + 1];
        } while (ge <= e);
        seg_start = e;
        // the new segment starts bucket g (gs == e: entries are contiguous, empty buckets skipped)
        if constexpr (ADD) acc = A::in(load_xyzz(bsum, g));
        else acc = A::identity();
      }
      uint32_t v;
      G1Aff p;
      if constexpr (PF == 0) {
        v = ent[e];
        p = load_vpoint(bases, phix, v & 0x7fffffffu, nsplit, phi64);
      } else if constexpr (PF == 1) {
        v = vnext;
        if (e + 1 < e_end) vnext = ent[e + 1];
        p = load_vpoint(bases, phix, v & 0x7fffffffu, nsplit, phi64);
      } else {
        v = vnext;
        p = pnext;
        if (e + 1 < e_end) {  // next entry's point in flight during this addition
          vnext = ent[e + 1];
          pnext = load_vpoint(bases, phix, vnext & 0x7fffffffu, nsplit, phi64);
        }
      }
      if (!p.is_identity()) acc = A::madd(acc, p, (v & 0x80000000u) != 0);
    }
    if constexpr (!R29) sum = A::out(acc);
    if (seg_start == gs && e_end == ge) {
      if constexpr (R29) st_rec29(bsum, g, acc);
      else store_xyzz(bsum, g, sum);
    } else if (seg_start != gs) {  // first segment, bucket started earlier (it may also go on later)
      if constexpr (R29) {
        if (join_in_block(gs, ge, K)) st_rec29(reinterpret_cast<G1Xyzz*>(shead29), threadIdx.x, acc);
        else st_rec29(pfirst, t, acc);
      } else {
        if (join_in_block(gs, ge, K)) shead[threadIdx.x] = sum;
        else store_xyzz(pfirst, t, sum);
      }
    } else if (join_in_block(gs, ge, K)) {  // this thread owns a two-piece in-block bucket
      owner = true;
    } else {
      if constexpr (R29) st_rec29(first ? pfirst : plast, t, acc);
      else store_xyzz(first ? pfirst : plast, t, sum);
      multi[atomicAdd(nmulti, 1u)] = g;  // joined by k_fixup
      if ((ge - 1) / K - gs / K > kFixSerial) heavy[atomicAdd(nheavy, 1u)] = g;
    }
  }
  __syncthreads();
  if (owner) {
    if constexpr (R29)  // the two pieces added in the chain's own form (X below 8p in, and out: a record's bound)
      st_rec29(bsum, g, r29::add_x8(acc, ld_rec29(reinterpret_cast<const G1Xyzz*>(shead29), threadIdx.x + 1)));
    else
      store_xyzz(bsum, g, xyzz_add(sum, shead[threadIdx.x + 1]));
  }
}

// Queued crossing buckets (see k_accumulate): pieces pfirst/plast joined serially when the bucket
// spans at most kFixSerial + 1 threads; longer ones (skewed digits: all-equal scalars, a short top
// window) are queued by k_accumulate for k_fixup's heavy blocks instead of being walked serially.
__device__ __forceinline__ G1Xyzz fixup_head(const G1Xyzz* __restrict__ pfirst, const G1Xyzz* __restrict__ plast,
                                             uint32_t s, uint32_t t0, uint32_t K, int r29w) {
  return load_bucket((s == t0 * K) ? pfirst : plast, t0, r29w);
}

// One launch for both queues: blocks [0, gm) walk the multi queue (grid-stride, one bucket per
// thread, a serial chain of at most kFixSerial 2p-domain additions), blocks [gm, gridDim) take the
// heavy queue (one bucket per block: strided partial sums of the per-thread pieces + LDS tree).
// The two queues hold disjoint buckets (k_accumulate puts a bucket of more than kFixSerial + 1
// pieces in both; the multi walk skips it).
__global__ void __launch_bounds__(kBlock) k_fixup(const uint32_t* __restrict__ gst, uint32_t K,
                                                  const G1Xyzz* __restrict__ pfirst,
                                                  const G1Xyzz* __restrict__ plast,
                                                  const uint32_t* __restrict__ multi,
                                                  const uint32_t* __restrict__ nmulti,
                                                  const uint32_t* __restrict__ heavy,
                                                  const uint32_t* __restrict__ nheavy, uint32_t gm,
                                                  G1Xyzz* __restrict__ bsum, int r29w) {
  __shared__ G1Xyzz sh[kBlock];
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x < gm) {  // block-uniform
    // one bucket per QUAD of lanes (quad.hpp: lane c = coordinate c): the chain of at most
    // kFixSerial additions is latency-bound (a few waves per SIMD), so 4-level quad additions
    // shorten it 2-3x; every branch below is uniform within the quad
    const uint32_t nm = *nmulti;
    const int c = tid & 3;
    for (uint32_t h = (blockIdx.x * blockDim.x + tid) >> 2; h < nm; h += (gm * blockDim.x) >> 2) {
      const uint32_t g = multi[h];
      const uint32_t s = gst[g], e = gst[g + 1];
      const uint32_t t0 = s / K, t1 = (e - 1) / K;
      if (t1 - t0 > kFixSerial) continue;  // a heavy bucket: the other blocks' part
      // r29w (k_accumulate's 29-bit chain): pieces and the stored sum as 29-bit records
      const G1Xyzz* h0 = s == t0 * K ? pfirst : plast;
      Fq acc = r29w ? rec29_coord_canonical(rec_at(h0, t0, 1), c) : quad::ld(h0 + t0, c);
      for (uint32_t t = t0 + 1; t <= t1; t++) {
        const Fq v = r29w ? rec29_coord_canonical(rec_at(pfirst, t, 1), c) : quad::ld(pfirst + t, c);
        acc = quad::add_2p(acc, v, c);
      }
      acc = fe_canon2p(acc);
      if (r29w) rec29_coord_store(rec_at(bsum, g, 1), c, acc);
      else quad::st(bsum + g, c, acc);
    }
    return;
  }
  const uint32_t nh = *nheavy, gh = gridDim.x - gm;
  for (uint32_t h = blockIdx.x - gm; h < nh; h += gh) {
    const uint32_t g = heavy[h];
    const uint32_t s = gst[g], e = gst[g + 1];
    const uint32_t t0 = s / K, t1 = (e - 1) / K;
    G1Xyzz acc = G1Xyzz::identity();
    for (uint32_t t = t0 + 1 + tid; t <= t1; t += kBlock) acc = xyzz_add(acc, load_bucket(pfirst, t, r29w));
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t st = kBlock / 2; st > 0; st >>= 1) {
      if (tid < st) sh[tid] = xyzz_add(sh[tid], sh[tid + st]);
      __syncthreads();
    }
    if (tid == 0) {
      const G1Xyzz sum = xyzz_add(fixup_head(pfirst, plast, s, t0, K, r29w), sh[0]);
      store_bucket(bsum, g, xyzz_canon2p(sum), r29w);
    }
    __syncthreads();
  }
}

// Bucket i of one window (x, gs: that window's bucket sums and starts): false when empty.
// gs == null: every bucket was written (host-fed merge).  (Joining the crossing buckets here
// instead of in k_fixup was measured 155 -> 440 us for k_wsum at 2^20: ~7 % of buckets cross,
// so nearly every wave's iteration diverges into the join loop.)
__device__ __forceinline__ bool bucket_at(const G1Xyzz* __restrict__ x, const uint32_t* __restrict__ gs, uint32_t i,
                                          G1Xyzz& out, int r29w) {  // r29w: sums in the 29-bit chain's form
  if (gs && gs[i] == gs[i + 1]) return false;
  out = load_bucket(x, i, r29w);
  return true;
}

// bucket i in the 29-bit chain's own form (its record as stored: no conversion); false when empty
__device__ __forceinline__ bool bucket_at29(const G1Xyzz* __restrict__ x, const uint32_t* __restrict__ gs, uint32_t i,
                                            r29::Xyzz& out) {
  if (gs && gs[i] == gs[i + 1]) return false;
  out = ld_rec29(x, i);
  return true;
}

// One bucket-reduction level over `groups` groups of N elements, segments of L buckets:
//   acc[g][j] = sum_{i in seg j} (i - jL + base) X[g][i],  tot[g][j] = sum_{i in seg j} X[g][i]
// Empty buckets (gst[b] == gst[b + 1]) are never written by the accumulate pass and read as identity.
__global__ void __launch_bounds__(kBlock) k_wsum(const G1Xyzz* __restrict__ X, const uint32_t* __restrict__ gst,
                                                 uint32_t N, uint32_t J, uint32_t L, uint32_t groups, int base,
                                                 G1Xyzz* __restrict__ acc_out, G1Xyzz* __restrict__ tot_out,
                                                 int r29w) {
  uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= J * groups) return;
  uint32_t g = tid / J, j = tid % J;
  const G1Xyzz* x = rec_at(X, (size_t)g * N, r29w);
  const uint32_t* gs = gst ? gst + (size_t)g * N : nullptr;
  uint32_t lo = j * L;
  uint32_t hi = min(N, lo + L);
  G1Xyzz run = G1Xyzz::identity(), acc = G1Xyzz::identity();
  if (hi > lo) {
    // bucket i - 1 (and its emptiness) is loaded while bucket i is being added (A/B at 2^20:
    // reduce 0.404 -> 0.393 ms)
    uint32_t i = hi - 1;
    G1Xyzz nx = G1Xyzz::identity();
    bool ne = bucket_at(x, gs, i, nx, r29w);
    for (;;) {
      const G1Xyzz cur = nx;
      const bool cne = ne;
      const uint32_t ci = i;
      if (ci > lo) {
        i = ci - 1;
        ne = bucket_at(x, gs, i, nx, r29w);
      }
      if (cne) run = xyzz_add_2p(run, cur);
      if (base || ci > lo) acc = xyzz_add_2p(acc, run);
      if (ci == lo) break;
    }
  }
  store_xyzz(acc_out, tid, xyzz_canon2p(acc));
  if (tot_out) store_xyzz(tot_out, tid, xyzz_canon2p(run));
}

// Step 2 fused: P 512-thread blocks per (window, group) each sum a 1/P slice of the group's H
// members (strided, ~H/(512 P) serial adds per thread) and finish with an LDS tree (9 levels).
// With P > 1 the slices' sums go to part[] and the block that finishes last (device-scope counter
// cnt[gid], zeroed per call) adds them -> out[w*NG + q].  P = 2 whenever the groups alone would not
// give every CU a block (GLV at 2^20: 120 groups, 17 -> 13 dependent additions per chain).
static constexpr int kGroupBlock = 512;
// member m of group q of window w (see above)
__device__ __forceinline__ G1Xyzz group_member(const G1Xyzz* __restrict__ acc, const G1Xyzz* __restrict__ tot,
                                               uint32_t w, uint32_t q, uint32_t J, uint32_t H, uint32_t m) {
  if (q < 2) return load_xyzz(acc, w * J + q * H + m);
  const uint32_t k = q - 2;
  const uint32_t j = ((m >> k) << (k + 1)) | (1u << k) | (m & ((1u << k) - 1));
  return load_xyzz(tot, w * J + j);
}
// XYZZ value of one lane as 32 dwords: LDS in structure-of-arrays order (dword d of lane t at
// [d][t], conflict-free), and a wave-level shift down by `off` lanes
__device__ __forceinline__ void sh_put(uint32_t (*sh)[kGroupBlock], uint32_t t, const G1Xyzz& v) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < 32; k++) sh[k][t] = d[k];
}
__device__ __forceinline__ G1Xyzz sh_get(uint32_t (*sh)[kGroupBlock], uint32_t t) {
  G1Xyzz v;
  uint32_t* d = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < 32; k++) d[k] = sh[k][t];
  return v;
}
__device__ __forceinline__ G1Xyzz wave_down(const G1Xyzz& v, int off) {
  G1Xyzz r;
  const uint32_t* d = reinterpret_cast<const uint32_t*>(&v);
  uint32_t* o = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int k = 0; k < 32; k++) o[k] = __shfl_down(d[k], off);
  return r;
}
__global__ void __launch_bounds__(kGroupBlock) k_group_sum(const G1Xyzz* __restrict__ acc,
                                                           const G1Xyzz* __restrict__ tot, uint32_t J,
                                                           uint32_t logJ, uint32_t P, G1Xyzz* __restrict__ out,
                                                           G1Xyzz* __restrict__ part, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t sh[32][kGroupBlock];  // 64 KiB
  const uint32_t NG = 2 + logJ, H = J / 2;
  const uint32_t gid = blockIdx.x / P, pp = blockIdx.x % P, w = gid / NG, q = gid % NG, tid = threadIdx.x;
  const uint32_t m0 = (uint32_t)((uint64_t)H * pp / P), m1 = (uint32_t)((uint64_t)H * (pp + 1) / P);
  // strided members, two loads in flight per addition pair
  G1Xyzz s = G1Xyzz::identity();
  uint32_t m = m0 + tid;
  for (; m + kGroupBlock < m1; m += 2 * kGroupBlock) {
    const G1Xyzz x0 = group_member(acc, tot, w, q, J, H, m);
    const G1Xyzz x1 = group_member(acc, tot, w, q, J, H, m + kGroupBlock);
    s = xyzz_add_2p(s, x0);
    s = xyzz_add_2p(s, x1);
  }
  if (m < m1) s = xyzz_add_2p(s, group_member(acc, tot, w, q, J, H, m));
  // tree: three cross-wave levels through LDS, then six inside wave 0
  for (uint32_t st = kGroupBlock / 2; st >= 64; st >>= 1) {
    if (tid >= st && tid < 2 * st) sh_put(sh, tid, s);
    __syncthreads();
    if (tid < st) s = xyzz_add_2p(s, sh_get(sh, tid + st));
    __syncthreads();
  }
  if (tid >= 64) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const G1Xyzz o = wave_down(s, off);
    if ((int)tid < off) s = xyzz_add_2p(s, o);
  }
  if (tid != 0) return;
  if (P > 1) {
    store_xyzz(part, blockIdx.x, s);
    __threadfence();
    if (atomicAdd(&cnt[gid], 1u) != P - 1) return;
    __threadfence();
    for (uint32_t k = 0; k < P; k++)
      if (k != pp) s = xyzz_add_2p(s, load_xyzz(part, gid * P + k));
  }
  store_xyzz(out, gid, xyzz_canon2p(s));
}

// The same subset sums with every XYZZ addition split over a quad of lanes (quad.hpp: lane
// c = lane & 3 holds coordinate c; 4 product levels per addition instead of ~14 dependent products):
// the tree is latency-bound (one wave per SIMD, most lanes idle in its upper levels), so a 3-4x
// shorter addition shortens the whole kernel.  512-thread blocks: strided member sums with whole
// per-lane additions (4 per lane: throughput work), then the tree in quad form -- a 4 x 4 transpose
// turns each quad's four sums into quad-form points (two levels), then four in-wave levels (lane
// shifts of 32 .. 4) and three cross-wave levels through LDS: 9 quad-addition levels instead of 9
// whole-addition levels.
__global__ void __launch_bounds__(kGroupBlock) k_group_sum_q(const G1Xyzz* __restrict__ acc,
                                                             const G1Xyzz* __restrict__ tot, uint32_t J,
                                                             uint32_t logJ, uint32_t P, G1Xyzz* __restrict__ out,
                                                             G1Xyzz* __restrict__ part, uint32_t* __restrict__ cnt) {
  constexpr int kWaves = kGroupBlock / 64;
  __shared__ Fq sh[kWaves][4];
  const uint32_t NG = 2 + logJ, H = J / 2;
  const uint32_t gid = blockIdx.x / P, pp = blockIdx.x % P, w = gid / NG, g = gid % NG, tid = threadIdx.x;
  const int c = tid & 3, lane = tid & 63, wave = tid >> 6;
  const uint32_t m0 = (uint32_t)((uint64_t)H * pp / P), m1 = (uint32_t)((uint64_t)H * (pp + 1) / P);
  // strided member sums with whole additions per lane (throughput work: every lane busy), two loads
  // in flight per addition pair, as k_group_sum
  G1Xyzz ps = G1Xyzz::identity();
  uint32_t m = m0 + tid;
  for (; m + kGroupBlock < m1; m += 2 * kGroupBlock) {
    const G1Xyzz x0 = group_member(acc, tot, w, g, J, H, m);
    const G1Xyzz x1 = group_member(acc, tot, w, g, J, H, m + kGroupBlock);
    ps = xyzz_add_2p(ps, x0);
    ps = xyzz_add_2p(ps, x1);
  }
  if (m < m1) ps = xyzz_add_2p(ps, group_member(acc, tot, w, g, J, H, m));
  // the tree in quad form: transpose the quad's four points to coordinates, add them (two levels),
  // then quads across the wave and across waves
  Fq v[4] = {ps.X, ps.Y, ps.ZZ, ps.ZZZ};
  quad::transpose(v, c);
  Fq s = quad::add_2p(quad::add_2p(v[0], v[1], c), quad::add_2p(v[2], v[3], c), c);
#pragma unroll 1
  for (int off = 32; off >= 4; off >>= 1) {
    const Fq o = quad::down(s, off);
    if (lane < off) s = quad::add_2p(s, o, c);
  }
  if (lane < 4) sh[wave][c] = s;
  __syncthreads();
  if (wave != 0) return;
  if (lane < 4 * kWaves) s = sh[lane >> 2][c];
#pragma unroll 1
  for (int off = 2 * kWaves; off >= 4; off >>= 1) {
    const Fq o = quad::down(s, off);
    if (lane < off) s = quad::add_2p(s, o, c);
  }
  if (lane >= 4) return;
  if (P > 1) {
    quad::st(part + blockIdx.x, c, s);
    __threadfence();
    uint32_t prev = 0;
    if (lane == 0) prev = atomicAdd(&cnt[gid], 1u);
    prev = (uint32_t)__shfl((int)prev, 0);
    if (prev != P - 1) return;  // uniform over the quad
    __threadfence();
    for (uint32_t k = 0; k < P; k++)
      if (k != pp) s = quad::add_2p(s, quad::ld(part + gid * P + k, c), c);
  }
  quad::st(out + gid, c, fe_canon2p(s));
}

// ---- Round 3: the subset sums as a tree inside the running-sum kernel.  k_group_sum(_q) sums every
// group U_k = sum_{j : bit k of j} T_j from scratch: logJ groups of J/2 members, ~J logJ / 2 additions
// per window.  The tree shares them: with block sums BS_0 = T, BS_{l+1}[i] = BS_l[2i] + BS_l[2i+1],
// U_l = sum of the odd BS_l[i] -- ~2J additions per window (and A = sum_j acc_j).  k_wsum_tree runs
// the running sums of 256 consecutive segments per block (one per thread, as k_wsum) and then the
// tree of the block's 256 segments in LDS, in place: at level l the pair (2i, 2i+1) of 2^l-blocks
// merges BS into position 2i 2^l, leaves its right half's sum at (2i + 1) 2^l as U_l's partial, and
// merges the partials of every U_k, k < l, at offset 2^k of the two halves -- (2 + l) 2^(7-l) tasks
// (A, BS, U_0..U_(l-1)), reads only from right halves, writes only to left halves, so a level needs
// one barrier.  Level 0 runs in registers (lane pairs, whole additions); levels 1..7 in quad form.
// A block ends with 10 points: A, the block total CT and U_0..U_7's partials (positions 2^k).
// k_group_fin then sums them per window: A over the blocks (two halves, the A_lo / A_hi slots the
// host Horner expects), U_k (k < 8) over the blocks, U_k (k >= 8) over the blocks whose index has
// bit k - 8 set (their CT).
// kTreeN segments per block (= threads), kTreeOut per-block outputs: msm_plan.hpp
static constexpr int kTreeRS = kTreeN + 1;                  // LDS row stride in dwords (quads conflict-free)
static constexpr size_t kTreeRow = (size_t)32 * kTreeRS * 4;  // one row of 256 points, structure of arrays

// dword d of point p at row[d * kTreeRS + p]; the quad form reads coordinate c (dwords 8c .. 8c + 7)
__device__ __forceinline__ void tr_put(uint32_t* row, uint32_t p, const G1Xyzz& v) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < 32; k++) row[k * kTreeRS + p] = d[k];
}
__device__ __forceinline__ G1Xyzz tr_get(const uint32_t* row, uint32_t p) {
  G1Xyzz v;
  uint32_t* d = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < 32; k++) d[k] = row[k * kTreeRS + p];
  return v;
}
__device__ __forceinline__ Fq tr_getc(const uint32_t* row, uint32_t p, int c) {
  Fq r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.v[k] = row[(8 * c + k) * kTreeRS + p];
  return r;
}
__device__ __forceinline__ void tr_putc(uint32_t* row, uint32_t p, int c, const Fq& v) {
#pragma unroll
  for (int k = 0; k < 8; k++) row[(8 * c + k) * kTreeRS + p] = v.v[k];
}
__device__ __forceinline__ G1Xyzz xor1(const G1Xyzz& v) {  // the neighbour lane's point (DPP quad_perm)
  G1Xyzz r;
  const uint32_t* d = reinterpret_cast<const uint32_t*>(&v);
  uint32_t* o = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int k = 0; k < 32; k++) o[k] = (uint32_t)__builtin_amdgcn_mov_dpp((int)d[k], quad::qp(1, 0, 3, 2), 0xF, 0xF, false);
  return r;
}
// task tau of tree level l (pairs of 2^l-blocks, np pairs, A row first when RUN): its row and the
// left-half slot it merges into (the right half's slot is + 2^l)
template <bool RUN>
__device__ __forceinline__ uint32_t* tr_task(uint32_t tau, uint32_t np, uint32_t s, uint32_t* rowA, uint32_t* rowT,
                                             uint32_t& dst) {
  if (RUN && tau < np) {
    dst = 2 * tau * s;
    return rowA;
  }
  const uint32_t r = RUN ? tau - np : tau, kk = r / np, i = r % np;  // kk 0: BS, kk >= 1: U_(kk-1) at 2^(kk-1)
  dst = 2 * i * s + (kk ? 1u << (kk - 1) : 0u);
  return rowT;
}

// RUN: running sums over L-bucket segments, then the tree over the block's 256 segments (rows A and
// T; one block per CU at 2^20).  !RUN (round 3, L = 1): the tree straight over 256 buckets per block
// -- no running sums and no A row (A = the total), a quarter of the LDS, so four blocks share a CU
// and one block's latency-bound upper levels overlap another's wide lower ones; its wide levels
// 1 and 2 run as whole additions (one per lane), the rest in quad form.
template <bool RUN, bool R29 = false>
__global__ void __launch_bounds__(kTreeN) k_wsum_tree(const G1Xyzz* __restrict__ X, const uint32_t* __restrict__ gst,
                                                       uint32_t N, uint32_t J, uint32_t L,
                                                       G1Xyzz* __restrict__ blk_out, int r29w) {
  extern __shared__ uint32_t tr_lds[];
  uint32_t* rowT = tr_lds;
  uint32_t* rowA = tr_lds + 32 * kTreeRS;  // RUN only
  constexpr int kWhole = RUN ? 1 : 3;      // levels below this run as whole additions
  const uint32_t tid = threadIdx.x, bpw = J >> kTreeLog;
  const uint32_t g = blockIdx.x / bpw, j = (blockIdx.x % bpw) * kTreeN + tid;
  const G1Xyzz* x = rec_at(X, (size_t)g * N, r29w);
  const uint32_t* gs = gst ? gst + (size_t)g * N : nullptr;
  const bool odd = tid & 1;
  if constexpr (RUN) {
    // running sums over segment j of window g, exactly as k_wsum with base 1
    const uint32_t lo = j * L, hi = min(N, lo + L);
    G1Xyzz run = G1Xyzz::identity(), acc = G1Xyzz::identity();
    if constexpr (R29) {
      // the 29-bit chain's sums (r29w) read as they are stored, the running sums in the same form
      // (r29::add: no carry adds, no per-bucket conversion), converted once for the tree below
      r29::Xyzz run29 = r29::identity(), acc29 = r29::identity();
      if (hi > lo) {
        uint32_t i = hi - 1;
        r29::Xyzz nx = r29::identity();
        bool ne = bucket_at29(x, gs, i, nx);
        for (;;) {
          const r29::Xyzz cur = nx;
          const bool cne = ne;
          const uint32_t ci = i;
          if (ci > lo) {
            i = ci - 1;
            ne = bucket_at29(x, gs, i, nx);
          }
          if (cne) run29 = r29::add(run29, cur);
          acc29 = r29::add(acc29, run29);
          if (ci == lo) break;
        }
      }
      run = AccChain<true>::canonical(run29);
      acc = AccChain<true>::canonical(acc29);
    } else if (hi > lo) {
      uint32_t i = hi - 1;
      G1Xyzz nx = G1Xyzz::identity();
      bool ne = bucket_at(x, gs, i, nx, r29w);
      for (;;) {
        const G1Xyzz cur = nx;
        const bool cne = ne;
        const uint32_t ci = i;
        if (ci > lo) {
          i = ci - 1;
          ne = bucket_at(x, gs, i, nx, r29w);
        }
        if (cne) run = xyzz_add_2p(run, cur);
        acc = xyzz_add_2p(acc, run);
        if (ci == lo) break;
      }
    }
    // level 0 (lane pairs, one addition per lane): even lanes A[2i] + A[2i+1], odd lanes
    // T[2i] + T[2i+1]; the odd T stays where it is as U_0's partial
    const G1Xyzz oa = xor1(acc), ot = xor1(run);
    const G1Xyzz s0 = xyzz_add_2p(odd ? ot : acc, odd ? run : oa);
    if (odd) {
      tr_put(rowT, tid - 1, s0);
      tr_put(rowT, tid, run);
    } else {
      tr_put(rowA, tid, s0);
    }
  } else {
    // level 0 over the buckets themselves (odd lanes; an empty bucket is the identity)
    G1Xyzz t = G1Xyzz::identity();
    if (j < N) bucket_at(x, gs, j, t, r29w);
    const G1Xyzz ot = xor1(t);
    if (odd) {
      tr_put(rowT, tid - 1, xyzz_add_2p(ot, t));
      tr_put(rowT, tid, t);
    }
  }
  __syncthreads();
  const int c = tid & 3;
  const uint32_t qd = tid >> 2;
#pragma unroll 1
  for (int l = 1; l < kTreeLog; l++) {
    const uint32_t s = 1u << l, np = (uint32_t)kTreeN >> (l + 1), ntask = ((RUN ? 2 : 1) + l) * np;
    if (l < kWhole) {  // whole additions, one task per thread (ntask <= 256)
      if (tid < ntask) {
        uint32_t dst;
        uint32_t* row = tr_task<RUN>(tid, np, s, rowA, rowT, dst);
        const G1Xyzz a = tr_get(row, dst), b = tr_get(row, dst + s);
        tr_put(row, dst, xyzz_add_2p(a, b));
      }
    } else {  // quad form: a task per quad and round (tasks of one level touch disjoint slots)
#pragma unroll 1
      for (uint32_t tau = qd; tau < ntask; tau += kTreeN / 4) {
        uint32_t dst;
        uint32_t* row = tr_task<RUN>(tau, np, s, rowA, rowT, dst);
        const Fq a = tr_getc(row, dst, c), b = tr_getc(row, dst + s, c);
        tr_putc(row, dst, c, quad::add_2p(a, b, c));
      }
    }
    __syncthreads();
  }
  // [A,] CT, U_0 .. U_7 -> blk_out (2p domain; k_group_fin canonicalises)
  if (tid >= (RUN ? 0u : 4u) && tid < (uint32_t)kTreeOut * 4) {
    const uint32_t q = tid >> 2;
    const uint32_t* row = q == 0 ? rowA : rowT;
    const uint32_t p = q < 2 ? 0u : 1u << (q - 2);
    quad::st(blk_out + (size_t)blockIdx.x * kTreeOut + q, c, tr_getc(row, p, c));
  }
}

// One block of two waves per (window, output slot): up to 128 members (bpw = J / 256 <= 128), each
// wave's 64 transposed into quad form, two quad additions inside each quad, the in-wave levels that
// still hold members, then wave 1's sum added to wave 0's.  aslot: the per-block slot the A sums
// read (0: A with running sums, 1: the block total CT for the pure tree).
__global__ void __launch_bounds__(128) k_group_fin(const G1Xyzz* __restrict__ blk_out, uint32_t bpw, uint32_t NG,
                                                   uint32_t aslot, G1Xyzz* __restrict__ out) {
  __shared__ Fq sh[4];
  const uint32_t w = blockIdx.x / NG, q = blockIdx.x % NG, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 3;
  const G1Xyzz* bo = blk_out + (size_t)w * bpw * kTreeOut;
  uint32_t members, b = tid, slot;
  if (q < 2) {  // A over the first / second half of the window's blocks
    const uint32_t h = (bpw + 1) / 2;
    members = q == 0 ? h : bpw - h;
    b = (q == 0 ? 0 : h) + tid;
    slot = aslot;
  } else if (q - 2 < (uint32_t)kTreeLog) {  // U_k, k < 8: every block's partial
    members = bpw;
    slot = q;
  } else {  // U_k, k >= 8: the totals of the blocks with bit k - 8 set
    const uint32_t m = q - 2 - kTreeLog;
    members = bpw / 2;
    b = ((tid >> m) << (m + 1)) | (1u << m) | (tid & ((1u << m) - 1));
    slot = 1;
  }
  if (wv > 0 && wv * 64 >= members) return;  // wave 1 only when there are more than 64 (wave 0 always
                                              // stores, the identity for an empty slot)
  const G1Xyzz v = tid < members ? load_xyzz(bo, b * kTreeOut + slot) : G1Xyzz::identity();
  Fq t[4] = {v.X, v.Y, v.ZZ, v.ZZZ};
  quad::transpose(t, c);
  Fq s = quad::add_2p(quad::add_2p(t[0], t[1], c), quad::add_2p(t[2], t[3], c), c);
  const uint32_t wm = min(64u, members - wv * 64);
  const uint32_t live = (wm + 3) / 4 * 4;  // lanes whose quads hold members
#pragma unroll 1
  for (uint32_t off = 32; off >= 4; off >>= 1) {
    if (off >= live) continue;  // uniform: only identities above
    const Fq o = quad::down(s, off);
    if (lane < off) s = quad::add_2p(s, o, c);
  }
  if (members > 64) {
    if (wv == 1 && lane < 4) sh[c] = s;
    __syncthreads();
    if (wv == 1) return;
    const Fq o = sh[c];
    s = quad::add_2p(s, o, c);
  }
  if (lane < 4) quad::st(out + blockIdx.x, c, fe_canon2p(s));
}

// ---------------------------------------------------------------------------------------------
// host orchestration (the plan, the switches, the buffer layout and the event slots: msm_plan.hpp)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(Fr) == kFrBytes && sizeof(G1Aff) == kAffBytes && sizeof(G1Xyzz) == kXyzzBytes &&
                  sizeof(uint4) == 16,
              "msm_plan.hpp's element sizes");
static_assert(ev_slot::kCount <= Workspace::kEvents, "msm_plan.hpp's event slots");

static thread_local sv_msm_stats g_last_stats;

int msm_last_stats(sv_msm_stats* out) {
  *out = g_last_stats;
  return SV_OK;
}

#define SV_LAUNCH_LOGB(KERNEL, LOGB, GRID, BLOCK, ...)                          \
  switch (LOGB) {                                                              \
    case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 5: hipLaunchKernelGGL(KERNEL<5>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 6: hipLaunchKernelGGL(KERNEL<6>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 7: hipLaunchKernelGGL(KERNEL<7>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 8: hipLaunchKernelGGL(KERNEL<8>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 9: hipLaunchKernelGGL(KERNEL<9>, GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 10: hipLaunchKernelGGL(KERNEL<10>, GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 11: hipLaunchKernelGGL(KERNEL<11>, GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 12: hipLaunchKernelGGL(KERNEL<12>, GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 13: hipLaunchKernelGGL(KERNEL<13>, GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 14: hipLaunchKernelGGL(KERNEL<14>, GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 15: hipLaunchKernelGGL(KERNEL<15>, GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    default: break;                                                            \
  }

#define SV_LAUNCH_C1(KERNEL, G, C, GRID, BLOCK, ...)                                              \
  switch (C) {                                                                                   \
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<4, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 5: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<5, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 6: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<6, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 7: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<7, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 8: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<8, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 9: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<9, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break;   \
    case 10: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<10, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 11: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<11, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 12: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<12, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 13: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<13, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 14: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<14, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 15: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<15, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    case 16: hipLaunchKernelGGL(HIP_KERNEL_NAME(KERNEL<16, G>), GRID, BLOCK, 0, st, __VA_ARGS__); break; \
    default: break;                                                                              \
  }
// full scalars or GLV halves (split on the fly)
#define SV_LAUNCH_C(KERNEL, GLV, C, GRID, BLOCK, ...)              \
  if (GLV) {                                                       \
    SV_LAUNCH_C1(KERNEL, true, C, GRID, BLOCK, __VA_ARGS__)        \
  } else {                                                         \
    SV_LAUNCH_C1(KERNEL, false, C, GRID, BLOCK, __VA_ARGS__)       \
  }

// Host Horner over every exponent: the group sums of window w are A_lo, A_hi at 2^(c w) and U_k at
// 2^(c w + logL + k), k < logJ (logL + logJ = c - 1, so the windows' exponents never collide), so one
// chain of c (W - 1) + c - 2 doublings with each term added at its exponent computes the total --
// 126 doublings + 120 additions with GLV at 2^20 instead of 224 + 119 for a Horner per window
// followed by one over the windows.
static host::Xyzz host_combine(const MsmPlan& p, const host::Xyzz* A) {
  const int top = (int)((p.W - 1) * p.c + p.logL + p.logJ - 1);
  host::Xyzz acc = host::x_identity();
  for (int e = top; e >= 0; e--) {
    acc = host::x_dbl(acc);
    const uint32_t w = (uint32_t)e / p.c, r = (uint32_t)e % p.c;
    const host::Xyzz* a = A + w * p.NG;
    if (r == 0) acc = host::x_add(host::x_add(acc, a[0]), a[1]);
    // (the tree straight over the buckets has logL = 0: U_0 shares A's exponent)
    if (r >= p.logL && r - p.logL < p.logJ) acc = host::x_add(acc, a[2 + r - p.logL]);
  }
  return acc;
}

// Scratch of the sort / accumulate stages.  The sort's own buffers (bcnt, btot, bstart, tmp) are
// reused piece after piece on one stream; its outputs (SortOut) and the accumulate's crossing-bucket
// pieces and queues are per piece / per accumulate stream.
struct MsmScratch {
  uint32_t *err, *bcnt, *btot, *bstart, *heavy, *multi, *nheavy, *nmulti;
  uint64_t* tmp;
  G1Xyzz *pfirst, *plast;
};
struct SortOut {
  uint32_t* ent;     // the piece's sorted entries (virtual point | sign << 31)
  uint32_t* gst;     // bucket starts, nbt + 1 (gst[nbt] = the entry total)
  uint32_t* tstart;  // owner bucket of every accumulate chunk
  uint32_t K, T;     // entries per accumulate thread, accumulate threads
};

// One call: what every stage reads.  res (a resident base set, msm.hpp): the call's points are rows
// [res->off, res->off + n) of the set.  Nothing is converted, checked or tabulated per call: the
// sorts run on the scalars alone and emit the set's record indices (P at off + i, phi(P) at
// N + off + i), the accumulate reads the set's table, a host-fed call stages scalars only, and
// bases is not used.
struct MsmCall {
  Workspace* ws;
  int device;
  size_t n;
  int mont_in;
  const MsmFeed* feed;
  const MsmResident* res;
  MsmTuning t;
  MsmPlan p;
  MsmShape s;
  bool lean, detail;  // MsmTuning::msm_lean, msm_stats (lean wins)
  // a resident set's record indices: P_i of the call at r_off + i, phi(P_i) at r_phi + i
  uint32_t r_off, r_phi;
  const uint4* r_tab;
  // inputs (device pointers; host-fed: the staging buffer) and the workspace's buffers (MsmBuffers)
  const G1Aff* bases;
  const Fr* scalars;
  G1Aff* bases_m;
  uint4 *phix, *stored;
  G1Xyzz *ping, *bsum, *racc, *rtot, *gpart, *tree_out;
  uint32_t *gst_all, *ent_all, *tst_all;
  MsmScratch w;
  std::vector<SortOut> so;                            // per piece
  const uint32_t* half_gst[2] = {nullptr, nullptr};  // split: each window half's bucket starts

  hipEvent_t ev(int slot) const { return ws->ev[slot]; }
  hipEvent_t ev_if(bool on, int slot) const { return on ? ws->ev[slot] : nullptr; }
};

// Digits + two-level counting sort of points [0, m) (virtual points p_off + i and, with GLV,
// nsplit + i: nsplit = m and p_off = 0 for a table of these m points, a resident set's phi record
// base and offset otherwise) into so, on stream st.  With phix set (bases resident) k_bin_hist also
// writes the GLV table; check_bases: Montgomery bases checked to be reduced on the way.
struct SortArgs {
  const G1Aff* bases = nullptr;
  const Fr* scalars = nullptr;
  size_t m = 0;  // real points (GLV: 2 m virtual ones)
  uint4* phix = nullptr;
  uint32_t nsplit = ~0u, p_off = 0;
  int check_bases = 0;
  uint32_t w0 = 0, nw = 0;  // windows [w0, w0 + nw) (nw = 0: all); so's buckets are those windows' (w - w0) * B + b
  uint4* stored = nullptr;  // the histogram pass's digits source for the scatter (MsmTuning::sort_halves)
  hipStream_t st = nullptr;
  hipStream_t side = nullptr;  // MsmTuning::sort_fork: the large fine-sort regions' stream
  hipEvent_t ev_mid = nullptr, ev_fork = nullptr, ev_join = nullptr;
};
static int msm_sort(const MsmCall& c, const SortOut& so, const SortArgs& a) {
  const MsmPlan& p = c.p;
  const MsmTuning& t = c.t;
  const MsmScratch& w = c.w;
  hipStream_t st = a.st;
  const int LOGB = p.c - 1;
  const int nb = p.glv ? 128 : 255;
  const uint32_t CB = (uint32_t)coarse_bits(p.c, nb), FB = (uint32_t)LOGB - CB, NBIN = 1u << CB;
  const uint32_t w0 = a.w0, nw = a.nw ? a.nw : p.W;
  const uint32_t nwb = nw * NBIN;
  const uint32_t npts = (uint32_t)a.m;
  const uint32_t ep = p.glv ? 2 * p.W : p.W;
  const uint32_t nblk = cdiv(npts, sort_chunk((int)ep));
  // u32 entries when every virtual point index (below nsplit + m with GLV, p_off + m without) fits
  const uint64_t vmax = p.glv ? (uint64_t)a.nsplit + npts : (uint64_t)a.p_off + npts;
  const int e32 = vmax <= (uint64_t(1) << (31 - FB)) && t.sort_e32 ? 1 : 0;
  const int xcd = t.sort_xcd, bm = t.sort_bm, hist_pf = t.hist_pf;
  const int mont_in = c.mont_in;
  SV_LAUNCH_C(k_bin_hist, p.glv, p.c, dim3(nblk), dim3(kBlock), a.scalars, npts, mont_in, nblk, w.bcnt, w.err,
              a.bases, a.phix, p.r29 ? kPhiVtab : p.phi64, a.check_bases, xcd, bm, w0, nw, a.stored, hist_pf);
  SV_HIP(hipGetLastError());
  if (a.ev_mid) SV_HIP(hipEventRecord(a.ev_mid, st));
  if (bm) {
    if (t.scan_keys == 16)
      hipLaunchKernelGGL(k_bin_scan_tiles<16>, dim3(cdiv(nwb, 16)), dim3(1024), 0, st, w.bcnt, nblk, nwb, w.btot);
    else
      hipLaunchKernelGGL(k_bin_scan_tiles<32>, dim3(cdiv(nwb, 32)), dim3(1024), 0, st, w.bcnt, nblk, nwb, w.btot);
  } else {
    hipLaunchKernelGGL(k_bin_scan_chunks, dim3(nwb), dim3(kBlock), 0, st, w.bcnt, nblk, w.btot);
  }
  // (fusing this scan into k_bin_scan_chunks' last block -- device-scope fence + counter -- was
  // measured 12 -> 122 us for that kernel: the fence writes back the XCD's L2)
  hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, st, w.btot, nwb, w.bstart, so.gst + (size_t)nw * p.B);
  SV_LAUNCH_C(k_bin_scatter, p.glv, p.c, dim3(nblk), dim3(kBlock), a.scalars, npts, mont_in, nblk, w.bcnt, w.btot,
              w.bstart, w.tmp, e32, xcd, bm, w0, nw, a.stored, a.p_off, p.glv ? a.nsplit : 0u);
  static thread_local int fine_attr_dev = -1;  // the > 64 KiB dynamic-LDS opt-in, once per thread/device
  if (fine_attr_dev != c.device) {
    SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fine_sort<0>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFineLds));
    SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fine_sort<1>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFineLds));
    SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fine_sort<2>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFineLds));
    fine_attr_dev = c.device;
  }
  if (!t.fine_split && !a.side) {  // one launch for both region kinds
    hipLaunchKernelGGL(k_fine_sort<2>, dim3(nwb), dim3(1024), kFineLds, st, w.tmp, e32, w.bstart, FB, so.K, so.gst,
                       so.tstart, so.ent);
    SV_HIP(hipGetLastError());
    return SV_OK;
  }
  // the two instantiations touch disjoint regions: with a side stream the large-region one (a few
  // dozen blocks, the top windows' crowded bins) runs concurrently with the other
  hipStream_t big_st = a.side ? a.side : st;
  if (a.side) {
    SV_HIP(hipEventRecord(a.ev_fork, st));
    SV_HIP(hipStreamWaitEvent(a.side, a.ev_fork, 0));
  }
  hipLaunchKernelGGL(k_fine_sort<1>, dim3(nwb), dim3(1024), kFineLds, big_st, w.tmp, e32, w.bstart, FB, so.K,
                     so.gst, so.tstart, so.ent);
  hipLaunchKernelGGL(k_fine_sort<0>, dim3(nwb), dim3(1024), kFineLds, st, w.tmp, e32, w.bstart, FB, so.K, so.gst,
                     so.tstart, so.ent);
  if (a.side) {
    SV_HIP(hipEventRecord(a.ev_join, a.side));
    SV_HIP(hipStreamWaitEvent(st, a.ev_join, 0));
  }
  SV_HIP(hipGetLastError());
  return SV_OK;
}

// Bucket accumulation of a sorted piece + its crossing-bucket fixups into bsum, on stream st
// (add_into: the piece's bucket sums are added to what bsum holds -- k_accumulate<true> starts each
// bucket's owner segment from it; otherwise complete buckets are stored and empty ones left alone).
struct AccArgs {
  const G1Aff* bases = nullptr;
  const uint4* phix = nullptr;
  uint32_t nsplit = ~0u;
  int add_into = 0;
  G1Xyzz* bsum = nullptr;
  uint32_t nbt = 0;  // the buckets so covers (0: all; a window half: its windows' buckets)
  hipStream_t st = nullptr;
  hipEvent_t ev_acc_done = nullptr, ev_fix_mid = nullptr;
};
static int msm_acc(const MsmCall& c, const MsmScratch& w, const SortOut& so, const AccArgs& a) {
  const MsmPlan& p = c.p;
  hipStream_t st = a.st;
  const uint32_t nbt = a.nbt ? a.nbt : p.nbt;
  // (a point prefetch one entry ahead, k_accumulate<., ., 2>, measured no gain on the device path or
  // on the host-fed pieces' ~2 waves per SIMD: 2^20 host-fed 2.69-2.71 ms either way)
  const int r29 = p.r29;
  // with the 29-bit chain phix is its table of every virtual point (vtab_put): record idx
  const uint32_t nsplit = r29 ? ~0u : a.nsplit;
  auto kern = a.add_into ? (r29 ? k_accumulate<true, true> : k_accumulate<true, false>)
                         : (r29 ? k_accumulate<false, true> : k_accumulate<false, false>);
  hipLaunchKernelGGL(kern, dim3(cdiv(so.T, kBlock)), dim3(kBlock), 0, st, a.bases, so.ent, so.gst, so.tstart, nbt,
                     so.K, so.T, a.bsum, w.pfirst, w.plast, w.multi, w.nmulti, w.heavy, w.nheavy, a.phix, nsplit,
                     p.phi64);
  SV_HIP(hipGetLastError());
  if (a.ev_acc_done) SV_HIP(hipEventRecord(a.ev_acc_done, st));
  const uint32_t gm = std::min<uint32_t>(cdiv(nbt, kBlock), 1024);
  hipLaunchKernelGGL(k_fixup, dim3(gm + 256), dim3(kBlock), 0, st, so.gst, so.K, w.pfirst, w.plast, w.multi,
                     w.nmulti, w.heavy, w.nheavy, gm, a.bsum, r29);
  SV_HIP(hipGetLastError());
  if (a.ev_fix_mid) SV_HIP(hipEventRecord(a.ev_fix_mid, st));
  return SV_OK;
}

// the fixup queue counters of piece (or window half) k: err[1 + 2k], err[2 + 2k], zeroed with the
// error flag, so no per-piece memset sits between the accumulates
static MsmScratch scratch_of(const MsmCall& c, int k) {
  MsmScratch wk = c.w;
  wk.nheavy = c.w.err + 1 + 2 * k;
  wk.nmulti = c.w.err + 2 + 2 * k;
  return wk;
}

// MSMs of at most kSmallMsmTerms terms (MsmTuning::small_msm): a fed call's inputs are staged whole
static int run_small(Workspace* ws, const void* d_bases, const void* d_scalars, size_t n, int form, int device,
                     const MsmFeed* feed, const MsmResident* res, host::Xyzz* out) {
  hipStream_t st = ws->stream;
  g_last_stats = sv_msm_stats{};
  int bases_form = form;
  if (res) {  // the set's Montgomery rows
    d_bases = reinterpret_cast<const G1Aff*>(res->rows) + res->off;
    bases_form = SV_MONTGOMERY;
  }
  if (feed) {
    MsmLayout in;
    const size_t so = in.put("scalars", n, sizeof(Fr)), bo = in.put("bases", res ? 0 : n, sizeof(G1Aff));
    SV_TRY(ws->reserve_in(in.total));
    SV_TRY(feed->stage_scalars(0, n, ws->inbuf + so, st, ws->ev[ev_slot::kSmallScalars]));
    d_scalars = ws->inbuf + so;
    if (!res) {
      SV_TRY(feed->stage_bases(0, n, ws->inbuf + bo, st, ws->ev[ev_slot::kSmallBases]));
      d_bases = ws->inbuf + bo;
    }
  }
  return msm_batch_windows_host(d_bases, d_scalars, nullptr, 1, n, form, bases_form, device, st, out);
}

// Reserve the workspace and the staging buffer by the one layout and form every pointer from it
template <class T>
static T* buf_at(char* base, size_t off) {
  return off == MsmLayout::kAbsent ? nullptr : reinterpret_cast<T*>(base + off);
}
static int lay_out(MsmCall& c, const MsmMode& mode, const void* d_bases, const void* d_scalars) {
  Workspace* ws = c.ws;
  const MsmShape& s = c.s;
  const MsmBuffers b = msm_buffers(c.n, mode, c.p, s);
  SV_TRY(ws->reserve(b.ws.total));
  SV_TRY(ws->reserve_pinned(s.nfinal * sizeof(G1Xyzz) + 256));
  if (c.feed) {
    SV_TRY(ws->reserve_in(b.in.total));
    SV_TRY(ws->ensure_copy_stream());
    SV_TRY(ws->ensure_sort_stream());
    d_bases = buf_at<void>(ws->inbuf, b.in_bases);
    d_scalars = ws->inbuf + b.in_scalars;
  }
  c.bases = reinterpret_cast<const G1Aff*>(d_bases);
  c.scalars = reinterpret_cast<const Fr*>(d_scalars);
  char* base = ws->buf;
  c.bases_m = buf_at<G1Aff>(base, b.bases_m);
  c.phix = buf_at<uint4>(base, b.phix);
  c.stored = buf_at<uint4>(base, b.stored);
  c.ping = buf_at<G1Xyzz>(base, b.ping);
  c.bsum = buf_at<G1Xyzz>(base, b.bsum);
  c.racc = buf_at<G1Xyzz>(base, b.racc);
  c.rtot = buf_at<G1Xyzz>(base, b.rtot);
  c.gpart = buf_at<G1Xyzz>(base, b.gpart);
  c.tree_out = buf_at<G1Xyzz>(base, b.tree_out);
  c.gst_all = buf_at<uint32_t>(base, b.gst);
  c.ent_all = buf_at<uint32_t>(base, b.ent);
  c.tst_all = buf_at<uint32_t>(base, b.tstart);
  MsmScratch& w = c.w;
  w.err = buf_at<uint32_t>(base, b.err);
  w.bcnt = buf_at<uint32_t>(base, b.bcnt);
  w.btot = buf_at<uint32_t>(base, b.btot);
  w.bstart = buf_at<uint32_t>(base, b.bstart);
  w.tmp = buf_at<uint64_t>(base, b.tmp);
  w.pfirst = buf_at<G1Xyzz>(base, b.pfirst);
  w.plast = buf_at<G1Xyzz>(base, b.plast);
  w.heavy = buf_at<uint32_t>(base, b.heavy);
  w.multi = buf_at<uint32_t>(base, b.multi);
  w.nheavy = w.err + 1;  // zeroed with the error flag
  w.nmulti = w.err + 2;
  c.so.resize(s.pieces);
  uint64_t eo = 0, to = 0;
  for (int k = 0; k < s.pieces; k++) {
    c.so[k] = {c.ent_all + eo, c.gst_all + (size_t)k * (c.p.nbt + 1), c.tst_all + to, s.K[k], s.T[k]};
    eo += (uint64_t)(s.pb[k + 1] - s.pb[k]) * s.ep;
    to += (uint64_t)s.T[k] + 1;
  }
  return SV_OK;
}

// Device inputs: canonical bases into the workspace's Montgomery copy (checked on the way)
static const G1Aff* device_bases(const MsmCall& c) {
  if (!c.s.conv) return c.bases;
  hipLaunchKernelGGL(k_to_mont_bases, dim3(cdiv(c.n, kBlock)), dim3(kBlock), 0, c.ws->stream, c.bases, c.bases_m,
                     (uint32_t)c.n, c.w.err);
  return c.bases_m;
}

// Device inputs, a resident set included: one sort, one accumulate, on the compute stream
static int run_device(MsmCall& c) {
  namespace ev = ev_slot;
  const MsmPlan& p = c.p;
  Workspace* ws = c.ws;
  hipStream_t st = ws->stream;
  const bool res = c.res != nullptr;
  const G1Aff* bases = res ? nullptr : device_bases(c);
  hipStream_t side = nullptr;
  if (!res && c.t.sort_fork) {
    SV_TRY(ws->ensure_copy_stream());  // idle on the device path
    side = ws->copy_stream;
  }
  const uint32_t nsplit = p.glv ? (res ? c.r_phi : (uint32_t)c.n) : ~0u;
  SV_TRY(msm_sort(c, c.so[0], {.bases = bases, .scalars = c.scalars, .m = c.n, .phix = res ? nullptr : c.phix,
                               .nsplit = nsplit, .p_off = c.r_off, .check_bases = res ? 0 : c.mont_in,
                               .stored = c.stored, .st = st, .side = side, .ev_mid = c.ev_if(c.detail, ev::kSortMid),
                               .ev_fork = c.ev(ev::kSortFork), .ev_join = c.ev(ev::kSortJoin)}));
  SV_HIP(hipEventRecord(c.ev(ev::kAccBegin), st));
  return msm_acc(c, c.w, c.so[0], {.bases = bases, .phix = res ? c.r_tab : c.phix, .nsplit = res ? ~0u : nsplit,
                                   .bsum = c.bsum, .st = st, .ev_acc_done = c.ev(ev::kAccEnd),
                                   .ev_fix_mid = c.ev_if(c.detail, ev::kFixEnd)});
}

// MsmTuning::msm_split: half A on the compute stream, half B on the sort stream beside A's accumulate
static int run_device_split(MsmCall& c) {
  namespace ev = ev_slot;
  const MsmPlan& p = c.p;
  const MsmShape& s = c.s;
  Workspace* ws = c.ws;
  hipStream_t st = ws->stream;
  const G1Aff* bases = device_bases(c);
  const uint32_t nsplit = p.glv ? (uint32_t)c.n : ~0u;
  SV_TRY(ws->ensure_sort_stream());
  hipStream_t ss = ws->sort_stream;
  const uint32_t nbt_a = s.nwh[0] * p.B;  // half A's buckets
  SortOut sh[2];
  MsmScratch wh[2] = {scratch_of(c, 0), scratch_of(c, 1)};
  for (int h = 0; h < 2; h++) {
    sh[h].K = p.K;
    sh[h].T = s.Th[h];
    sh[h].ent = c.ent_all + (h ? (size_t)p.npts * s.nwh[0] : 0);  // at most npts entries per window
    sh[h].gst = c.gst_all + (h ? (size_t)nbt_a + 1 : 0);
    sh[h].tstart = c.tst_all + (h ? s.Th[0] + 1 : 0);
    wh[h].pfirst = rec_at(c.w.pfirst, h ? s.Th[0] : 0, p.r29);
    wh[h].plast = rec_at(c.w.plast, h ? s.Th[0] : 0, p.r29);
    wh[h].heavy = c.w.heavy + (h ? nbt_a : 0);
    wh[h].multi = c.w.multi + (h ? nbt_a : 0);
    c.half_gst[h] = sh[h].gst;
  }
  G1Xyzz* bsum_b = rec_at(c.bsum, (size_t)nbt_a, p.r29);
  // half A: sort (with the GLV table and the base check), accumulate
  SV_TRY(msm_sort(c, sh[0], {.bases = bases, .scalars = c.scalars, .m = c.n, .phix = c.phix, .nsplit = nsplit,
                             .check_bases = c.mont_in, .w0 = 0, .nw = s.nwh[0], .st = st,
                             .ev_mid = c.ev_if(c.detail, ev::kSortMid)}));
  SV_HIP(hipEventRecord(c.ev(ev::kAccBegin), st));
  SV_HIP(hipStreamWaitEvent(ss, c.ev(ev::kAccBegin), 0));  // the sort scratch is free, the GLV table written
  SV_TRY(msm_acc(c, wh[0], sh[0], {.bases = bases, .phix = c.phix, .nsplit = nsplit, .bsum = c.bsum, .nbt = nbt_a,
                                   .st = st, .ev_acc_done = c.ev(ev::kAccEnd),
                                   .ev_fix_mid = c.ev_if(c.detail, ev::kFixEnd)}));
  // half B
  SV_TRY(msm_sort(c, sh[1], {.bases = bases, .scalars = c.scalars, .m = c.n, .nsplit = nsplit, .w0 = s.nwh[0],
                             .nw = s.nwh[1], .st = ss}));
  SV_HIP(hipEventRecord(c.ev(ev::kHalfBAccBegin), ss));
  SV_TRY(msm_acc(c, wh[1], sh[1], {.bases = bases, .phix = c.phix, .nsplit = nsplit, .bsum = bsum_b,
                                   .nbt = s.nwh[1] * p.B, .st = ss, .ev_acc_done = c.ev(ev::kHalfBAccEnd)}));
  SV_HIP(hipEventRecord(c.ev(ev::kHalfBEnd), ss));
  return SV_OK;
}

// The host-fed call's feeder.  The workspace's helper thread stages the pieces back to back (a
// pageable copy blocks the thread that issues it: queueing each piece's ~12 launches from that same
// thread left the copy engine idle ~30 us per burst, rocprof trace); the calling thread queues a
// piece's sort / accumulate as soon as the feeder has recorded the piece's events.  staged = stages
// done (2k + 1: piece k's scalars, 2k + 2: its bases), -1 once the feeder failed.
// Piece 0's scalars are staged by the CALLING thread, right after the helper is woken: the helper's
// wake-up (a condition variable, tens of us) then overlaps that first copy instead of delaying it,
// and the helper takes over from piece 0's bases (it spins until the scalars are issued, so the
// copy stream keeps the scalars-then-bases order).
class Feeder {
 public:
  explicit Feeder(const MsmCall& c) : c_(c) {}
  ~Feeder() {  // on every exit: stop the helper after its current stage, then wait for it
    if (!started_) return;
    stop_.store(1);
    c_.ws->wait_helper();
  }
  static int scalars_of(int k) { return 2 * k + 1; }
  static int bases_of(int k) { return 2 * k + 2; }

  int start() {
    SV_TRY(c_.ws->run_helper([this] { feed_pieces(); }));
    started_ = true;
    // an exception leaving stage_scalars (host-pool allocation) unwinds through the destructor, whose
    // stop releases the helper's wait; SV_GUARD then turns it into the call's error code
    const std::vector<size_t>& pb = c_.s.pb;
    const int rc0 = c_.feed->stage_scalars(pb[0], pb[1], const_cast<Fr*>(c_.scalars) + pb[0], c_.ws->copy_stream,
                                           c_.ev(ev_slot::piece_scalars(0)));
    if (rc0 != SV_OK) {
      fail(rc0);  // the helper, spinning on staged, exits
      return rc0;
    }
    staged_.store(scalars_of(0), std::memory_order_release);
    return SV_OK;
  }
  // block until `stage` (scalars_of / bases_of a piece) has been issued; the feeder's error if it failed
  int wait(int stage) {
    int x;
    while ((x = staged_.load(std::memory_order_acquire)) >= 0 && x < stage) std::this_thread::yield();
    if (x < 0) {
      set_error("%s", err_.c_str());
      return rc_;
    }
    return SV_OK;
  }

 private:
  void fail(int rc) {
    rc_ = rc;
    err_ = sv::last_error();
    staged_.store(-1, std::memory_order_release);
  }
  void feed_pieces() {  // on the helper thread
    const MsmFeed* feed = c_.feed;
    const std::vector<size_t>& pb = c_.s.pb;
    hipStream_t cs = c_.ws->copy_stream;
    int rc = SV_OK;
    // the helper thread has no SV_GUARD: an exception here (std::function / vector allocation in
    // the host pool) becomes the call's SV_ERR_DEVICE instead of std::terminate
    try {
      int st0;
      // also leave when the caller stops before staging piece 0 (its copy failed or threw)
      while ((st0 = staged_.load(std::memory_order_acquire)) == 0 && !stop_.load(std::memory_order_relaxed))
        std::this_thread::yield();
      for (int k = 0; st0 > 0 && k < c_.s.pieces && !stop_.load(std::memory_order_relaxed); k++) {
        const size_t lo = pb[k], hi = pb[k + 1];
        if (k > 0) {
          rc = feed->stage_scalars(lo, hi, const_cast<Fr*>(c_.scalars) + lo, cs, c_.ev(ev_slot::piece_scalars(k)));
          if (rc != SV_OK) break;
          staged_.store(scalars_of(k), std::memory_order_release);
        }
        if (!c_.res)
          rc = feed->stage_bases(lo, hi, const_cast<G1Aff*>(c_.bases) + lo, cs, c_.ev(ev_slot::piece_bases(k)));
        if (rc != SV_OK) break;
        staged_.store(bases_of(k), std::memory_order_release);
      }
    } catch (const std::exception& e) {
      set_error("host-fed MSM feeder: %s", e.what());
      rc = SV_ERR_DEVICE;
    } catch (...) {
      set_error("host-fed MSM feeder: unknown exception");
      rc = SV_ERR_DEVICE;
    }
    if (rc != SV_OK) fail(rc);
  }

  const MsmCall& c_;
  std::atomic<int> staged_{0}, stop_{0};
  int rc_ = SV_OK;
  std::string err_;
  bool started_ = false;
};

// Piece k's landed bases (points [lo, lo + m)) made ready for its accumulate: conversion / check and
// the piece's table, on the sort stream behind the piece's sort (MsmTuning::fed_prep) or on the
// compute stream; `sorted` is recorded on the sort stream behind whatever ran there.  Returns the
// bases the accumulate reads.
static int prepare_piece(const MsmCall& c, Feeder& feeder, int k, uint4* phix_k, const G1Aff** pbases) {
  const MsmPlan& p = c.p;
  const size_t lo = c.s.pb[k], m = c.s.pb[k + 1] - lo;
  hipStream_t st = c.ws->stream, ss = c.ws->sort_stream;
  hipEvent_t sorted = c.ev(ev_slot::piece_sorted(k));
  const bool conv = c.s.conv;
  G1Aff* db = const_cast<G1Aff*>(c.bases) + lo;
  if (!c.t.fed_prep) SV_HIP(hipEventRecord(sorted, ss));
  SV_TRY(feeder.wait(Feeder::bases_of(k)));
  hipStream_t ps = c.t.fed_prep ? ss : st;
  SV_HIP(hipStreamWaitEvent(ps, c.ev(ev_slot::piece_bases(k)), 0));
  *pbases = conv ? c.bases_m + lo : db;
  if (conv)  // canonical bases converted (and checked) once they have landed
    hipLaunchKernelGGL(k_to_mont_bases, dim3(cdiv(m, kBlock)), dim3(kBlock), 0, ps, db, c.bases_m + lo, (uint32_t)m,
                       c.w.err);
  if (p.r29)  // the piece's table (29-bit chain) from the landed (converted) bases, checked
    hipLaunchKernelGGL(k_vtab, dim3(cdiv(m, kBlock)), dim3(kBlock), 0, ps, *pbases, (uint32_t)m, phix_k,
                       p.glv ? 1 : 0, conv ? nullptr : c.w.err);
  else if (!p.glv)
    hipLaunchKernelGGL(k_check_bases, dim3(cdiv(m, kBlock)), dim3(kBlock), 0, ps, db, (uint32_t)m, c.w.err);
  if (!p.r29 && p.glv)  // the piece's phi table from the landed (converted) bases; Montgomery ones checked
    hipLaunchKernelGGL(k_glv_phix, dim3(cdiv(m, kBlock)), dim3(kBlock), 0, ps, *pbases, (uint32_t)m, phix_k, p.phi64,
                       conv ? nullptr : c.w.err);
  SV_HIP(hipGetLastError());
  if (c.t.fed_prep) SV_HIP(hipEventRecord(sorted, ss));
  return SV_OK;
}

// Host-fed.  Piece k: the copy stream stages its scalars, then its bases; the sort stream sorts the
// piece once its scalars have landed, beside the previous piece's accumulate, and prepares the
// landed bases; the compute stream accumulates the piece into the one bucket set
// (identity-initialised; pieces after the first add into it).  With a resident set there are no
// bases to wait for: the piece's accumulate is gated on its sort alone and reads the set's table at
// the piece's records.
static int run_fed(MsmCall& c) {
  namespace ev = ev_slot;
  const MsmPlan& p = c.p;
  const MsmShape& s = c.s;
  Workspace* ws = c.ws;
  hipStream_t st = ws->stream, cs = ws->copy_stream, ss = ws->sort_stream;
  const bool res = c.res != nullptr;
  if (s.pieces > 1) SV_HIP(hipMemsetAsync(c.bsum, 0, (size_t)p.nbt * s.rec_bytes, st));
  SV_HIP(hipEventRecord(c.ev(ev::kFedFork), st));
  SV_HIP(hipStreamWaitEvent(cs, c.ev(ev::kFedFork), 0));
  SV_HIP(hipStreamWaitEvent(ss, c.ev(ev::kFedFork), 0));
  Feeder feeder(c);
  SV_TRY(feeder.start());
  for (int k = 0; k < s.pieces; k++) {
    const size_t lo = s.pb[k], m = s.pb[k + 1] - lo;
    const uint32_t lo32 = (uint32_t)lo;
    hipEvent_t sorted = c.ev(ev::piece_sorted(k));
    // GLV: piece-local virtual points (i, m + i) over the piece's bases and its slice of the table;
    // a resident set: its records
    const uint32_t nsplit = p.glv ? (res ? c.r_phi + lo32 : (uint32_t)m) : ~0u;
    uint4* phix_k = s.tab4 ? c.phix + s.tab4 * lo : nullptr;
    SV_TRY(feeder.wait(Feeder::scalars_of(k)));
    SV_HIP(hipStreamWaitEvent(ss, c.ev(ev::piece_scalars(k)), 0));
    SV_TRY(msm_sort(c, c.so[k], {.scalars = c.scalars + lo, .m = m, .nsplit = nsplit,
                                 .p_off = res ? c.r_off + lo32 : 0u, .st = ss}));
    const G1Aff* pbases = nullptr;
    if (res) SV_HIP(hipEventRecord(sorted, ss));
    else SV_TRY(prepare_piece(c, feeder, k, phix_k, &pbases));
    SV_HIP(hipStreamWaitEvent(st, sorted, 0));
    if (k == 0) SV_HIP(hipEventRecord(c.ev(ev::kAccBegin), st));
    SV_TRY(msm_acc(c, scratch_of(c, k), c.so[k],
                   {.bases = pbases, .phix = res ? c.r_tab : phix_k, .nsplit = res ? ~0u : nsplit,
                    .add_into = k > 0 ? 1 : 0, .bsum = c.bsum, .st = st,
                    .ev_acc_done = c.ev_if(k == s.pieces - 1, ev::kAccEnd)}));
  }
  return SV_OK;
}

// Bucket reduction: running sums over segments of 2^logL buckets, then the subset sums (with
// several host-fed pieces every bucket of bsum holds a value: no emptiness table).  (Reducing the top
// windows first to overlap the host Horner with the lower ones was measured slower: each half-size
// launch of these occupancy-bound kernels takes nearly as long as the whole -- reduce 0.40 -> 0.67 ms.)
static int reduce_buckets(const MsmCall& c) {
  const MsmPlan& p = c.p;
  const MsmShape& s = c.s;
  hipStream_t st = c.ws->stream;
  const uint32_t* gst = s.pieces > 1 ? nullptr : c.so[0].gst;
  if (p.tree == 0) {
    hipLaunchKernelGGL(k_wsum, dim3(cdiv((uint64_t)p.J * p.W, kBlock)), dim3(kBlock), 0, st, c.bsum, gst, p.B, p.J,
                       1u << p.logL, p.W, 1, c.racc, c.rtot, p.r29);
    auto group_sum = c.t.group_quad ? k_group_sum_q : k_group_sum;
    hipLaunchKernelGGL(group_sum, dim3(p.NG * p.W * s.gparts), dim3(kGroupBlock), 0, st, c.racc, c.rtot, p.J, p.logJ,
                       s.gparts, c.ping, c.gpart, c.w.err + 64);
    SV_HIP(hipGetLastError());
    return SV_OK;
  }
  static thread_local int tree_attr_dev = -1;  // the > 64 KiB dynamic-LDS opt-in, once per thread/device
  if (tree_attr_dev != c.device) {
    SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wsum_tree<true, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * kTreeRow)));
    SV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wsum_tree<true, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * kTreeRow)));
    tree_attr_dev = c.device;
  }
  // windows [w0, w0 + nw) of the bucket sums xb (starts gs: empty buckets skipped) -> ping rows
  // running sums on the 29-bit chain when the bucket sums are stored in its form
  auto tree_run = p.r29 ? k_wsum_tree<true, true> : k_wsum_tree<true, false>;
  auto reduce_windows = [&](const G1Xyzz* xb, const uint32_t* gs, uint32_t w0, uint32_t nw) {
    if (p.tree == 2)
      hipLaunchKernelGGL(k_wsum_tree<false>, dim3(p.J / kTreeN * nw), dim3(kTreeN), kTreeRow, st, xb, gs, p.B, p.J,
                         1u, c.tree_out, p.r29);
    else
      hipLaunchKernelGGL(tree_run, dim3(p.J / kTreeN * nw), dim3(kTreeN), 2 * kTreeRow, st, xb, gs, p.B, p.J,
                         1u << p.logL, c.tree_out, p.r29);
    hipLaunchKernelGGL(k_group_fin, dim3(nw * p.NG), dim3(128), 0, st, c.tree_out, p.J / kTreeN, p.NG,
                       p.tree == 2 ? 1u : 0u, c.ping + (size_t)w0 * p.NG);
  };
  if (s.split) {
    reduce_windows(c.bsum, c.half_gst[0], 0, s.nwh[0]);  // beside half B's accumulate
    SV_HIP(hipStreamWaitEvent(st, c.ev(ev_slot::kHalfBEnd), 0));
    reduce_windows(rec_at(c.bsum, (size_t)s.nwh[0] * p.B, p.r29), c.half_gst[1], s.nwh[0], s.nwh[1]);
  } else {
    reduce_windows(c.bsum, gst, 0, p.W);
  }
  SV_HIP(hipGetLastError());
  return SV_OK;
}

// a host-fed call that fails part-way leaves copies (and sorts) queued on its other streams: drain
// them before the lease returns the staging buffers to the pool
struct Drain {
  Workspace* ws;
  bool armed;
  ~Drain() {
    if (armed) (void)ws->quiesce();
  }
};

// The group sums and the error word to the host, the host Horner, the call's stats
static int finish(const MsmCall& c, Drain& drain, host::Xyzz* out) {
  namespace ev = ev_slot;
  const MsmPlan& p = c.p;
  Workspace* ws = c.ws;
  hipStream_t st = ws->stream;
  const size_t nfinal = c.s.nfinal;
  SV_HIP(hipMemcpyAsync(ws->pinned, c.ping, nfinal * sizeof(G1Xyzz) + 4, hipMemcpyDeviceToHost, st));
  SV_HIP(hipStreamSynchronize(st));
  drain.armed = false;  // the copy and sort streams' work all precedes the compute stream's end
  uint32_t errv;
  memcpy(&errv, ws->pinned + nfinal * sizeof(G1Xyzz), 4);
  if (errv) {
    set_error("invalid input: %s%s", (errv & 1) ? "base coordinate not reduced mod p; " : "",
              (errv & 2) ? "scalar not reduced mod r" : "");
    return SV_ERR_ARG;
  }
  auto t0 = std::chrono::steady_clock::now();
  *out = host_combine(p, reinterpret_cast<const host::Xyzz*>(ws->pinned));
  auto t1 = std::chrono::steady_clock::now();

  sv_msm_stats& s = g_last_stats;
  auto span = [&](int from, int to) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c.ev(from), c.ev(to));
    return ms;
  };
  if (c.detail && !c.feed) {
    s.digits_ms = span(ev::kStart, ev::kSortMid);  // digits + coarse histogram (digits never stored; the GLV halves are)
    s.sort_ms = span(ev::kSortMid, ev::kAccBegin);
    s.fixup_ms = span(ev::kAccEnd, ev::kFixEnd);
    s.reduce_ms = span(ev::kFixEnd, ev::kEnd);
  } else if (c.lean) {
    s.digits_ms = s.sort_ms = s.fixup_ms = s.reduce_ms = -1.0f;  // not measured
  } else {  // digits folded into sort_ms, fixup into reduce_ms
    s.digits_ms = 0;
    s.sort_ms = span(ev::kStart, ev::kAccBegin);
    s.fixup_ms = 0;
    s.reduce_ms = span(ev::kAccEnd, ev::kEnd);
  }
  // host-fed: "accumulate" spans the first piece's accumulate to the last piece's (transfers included);
  // split: the two halves' accumulate launches, each from its own start to its own end (they may
  // overlap in time), and accumulate_span_ms from the first start to the last end
  const float ms = span(ev::kAccBegin, ev::kAccEnd);
  s.accumulate_ms = ms;
  s.accumulate_span_ms = ms;
  s.accumulate_launches = 1;
  if (c.s.split) {
    const float mb = span(ev::kHalfBAccBegin, ev::kHalfBAccEnd), mspan = span(ev::kAccBegin, ev::kHalfBAccEnd);
    s.accumulate_ms = ms + mb;
    s.accumulate_span_ms = std::max(ms, mspan);
    s.accumulate_launches = 2;
  }
  s.host_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
  s.total_ms = c.lean ? -1.0f : span(ev::kStart, ev::kEnd) + s.host_ms;
  s.window_bits = p.c;
  s.num_windows = p.W;
  s.accumulate_launch_units = cdiv((uint64_t)p.npts * p.W, p.K);
  s.entries = (uint64_t)p.npts * p.W;
  return SV_OK;
}

// Every single-MSM entry point: validate, the small route, plan, lay out, dispatch, reduce, finish
static int msm_run_impl(const void* d_bases, const void* d_scalars, size_t n, int form, int device,
                        hipStream_t user_stream, const MsmFeed* feed, host::Xyzz* out,
                        const MsmResident* res = nullptr) {
  if (n == 0) {
    set_error("pairs should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > (size_t(1) << 26)) {
    set_error("n = %zu exceeds the per-device limit 2^26 (shard across devices/calls)", n);
    return SV_ERR_LEN;
  }
  if (form != SV_CANONICAL && form != SV_MONTGOMERY) {
    set_error("bad form %d", form);
    return SV_ERR_ARG;
  }
  WsLease lease(device, user_stream);
  if (!lease.ok()) return SV_ERR_DEVICE;
  MsmCall c;
  c.ws = lease.get();
  c.t = msm_tuning();
  if (n <= kSmallMsmTerms && c.t.small_msm) return run_small(c.ws, d_bases, d_scalars, n, form, device, feed, res, out);
  c.device = device;
  c.n = n;
  c.mont_in = form == SV_MONTGOMERY ? 1 : 0;
  c.feed = feed;
  c.res = res;
  c.p = msm_plan(n, c.t);
  if (res) c.p.r29 = 1;
  MsmMode mode;
  mode.canonical = form == SV_CANONICAL;
  mode.fed = feed != nullptr;
  mode.resident = res != nullptr;
  if (feed) mode.pieces = feed->pieces, mode.split = feed->split;
  c.s = msm_shape(n, mode, c.p, c.t);
  c.lean = c.t.msm_lean;
  c.detail = c.t.msm_stats && !c.lean;
  c.r_off = res ? (uint32_t)res->off : 0u;
  c.r_phi = res ? (uint32_t)(res->N + res->off) : 0u;
  c.r_tab = res ? reinterpret_cast<const uint4*>(res->vtab) : nullptr;
  SV_TRY(lay_out(c, mode, d_bases, d_scalars));

  hipStream_t st = c.ws->stream;
  Drain drain{c.ws, feed != nullptr || c.s.split};
  if (!c.lean) SV_HIP(hipEventRecord(c.ev(ev_slot::kStart), st));
  SV_HIP(hipMemsetAsync(c.w.err, 0, c.s.nerr * 4, st));
  SV_TRY(feed ? run_fed(c) : c.s.split ? run_device_split(c) : run_device(c));
  SV_TRY(reduce_buckets(c));
  if (!c.lean) SV_HIP(hipEventRecord(c.ev(ev_slot::kEnd), st));
  return finish(c, drain, out);
}

int msm_run_device(const void* d_bases, const void* d_scalars, size_t n, int form, int device,
                   hipStream_t user_stream, host::Xyzz* out) {
  return msm_run_impl(d_bases, d_scalars, n, form, device, user_stream, nullptr, out);
}

int msm_run_fed(size_t n, int form, int device, const MsmFeed& feed, host::Xyzz* out) {
  return msm_run_impl(nullptr, nullptr, n, form, device, nullptr, &feed, out);
}

int msm_resident_prepare(const void* d_rows, size_t n, int form, int device, hipStream_t user_stream,
                         void* d_rows_m, void* d_vtab) {
  WsLease lease(device, user_stream);
  if (!lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = lease.get();
  hipStream_t st = ws->stream;
  SV_TRY(ws->reserve(256));
  SV_TRY(ws->reserve_pinned(256));
  uint32_t* err = ws->carve<uint32_t>(1);
  SV_HIP(hipMemsetAsync(err, 0, 4, st));
  hipLaunchKernelGGL(k_resident_prepare, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, st,
                     reinterpret_cast<const G1Aff*>(d_rows), reinterpret_cast<G1Aff*>(d_rows_m), (uint32_t)n,
                     form == SV_MONTGOMERY ? 1 : 0, reinterpret_cast<uint4*>(d_vtab), err);
  SV_HIP(hipGetLastError());
  SV_HIP(hipMemcpyAsync(ws->pinned, err, 4, hipMemcpyDeviceToHost, st));
  SV_HIP(hipStreamSynchronize(st));
  uint32_t errv;
  memcpy(&errv, ws->pinned, 4);
  if (errv) {
    set_error("invalid input: base coordinate not reduced mod p");
    return SV_ERR_ARG;
  }
  return SV_OK;
}

int msm_run_resident_device(const MsmResident& set, const void* d_scalars, size_t n, int form, int device,
                            hipStream_t user_stream, host::Xyzz* out) {
  return msm_run_impl(nullptr, d_scalars, n, form, device, user_stream, nullptr, out, &set);
}

int msm_run_resident_fed(const MsmResident& set, size_t n, int form, int device, const MsmFeed& feed,
                         host::Xyzz* out) {
  return msm_run_impl(nullptr, nullptr, n, form, device, nullptr, &feed, out, &set);
}

}  // namespace sv
