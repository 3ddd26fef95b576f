// Synthetic division of p(X) = sum_{i<n} a_i X^i over BN254 Fr by (X - z): the quotient of a KZG
// opening and the evaluation p(z), for coefficients that are already in HBM.
//
// With the suffix Horner values h_i = a_i + z h_{i+1} (h_n = 0): p(z) = h_0 and q_i = h_{i+1}.  The
// recurrence is a linear suffix scan under (h_L, z^len_L) o h_R = h_L + z^len_L h_R, run in three
// launches that never wait for another block (no look-back: a grid that depends on the order in
// which blocks are scheduled can hang on a shared device):
//   1. k_div_reduce    each block reduces its span of kDivSpan coefficients to one total
//                      B_b = sum_k a_{b S + k} z^k, and checks that every coefficient is below r;
//   2. k_div_carries   one block scans the totals with the weight z^S: carry_b = h_{(b+1) S}, and
//                      p(z) = B_0 + z^S carry_0;
//   3. k_div_quotient  each block rescans its span from its carry and writes q.
// Inside a block every thread walks kDivPer consecutive coefficients (a local Horner), and the 256
// thread values are combined by a Hillis-Steele suffix scan in LDS whose weight doubles its exponent
// per level (z^T, z^2T, ...).  No power of z is computed on the device: the host squares z into a
// per-call table of two dozen weights (DivWeights, CarryWeights: ~40 host products, 2 us) that
// travels in the kernel arguments, so every weight is wave-uniform.  All arithmetic is field.hpp's
// Montgomery Fr; canonical inputs are converted on load, outputs on store.  A block's error flag is
// a plain store beside its total, and phase 2 folds the flags: nothing has to be zeroed per call.
//
// Memory: a thread's coefficients are 32 T consecutive bytes, so direct loads would touch 64
// separate 16-B pieces per wave instruction.  A block's span goes through LDS instead: 16 B per
// lane, consecutive lanes consecutive addresses, into an image padded by 16 B per thread chunk
// (chunk stride 36 dwords for T = 4: the 16 lanes of a ds_read_b128 group land on 16 different
// 4-bank slots); phase 3 stages the quotient the same way back.  The image (36 KiB) is reused for
// the scan's two buffers, so four blocks fit a CU.  Traffic: the coefficients are read twice and
// the quotient written once, 96 B per coefficient.
//
// Several polynomials at one point (a GWC19 point set: c = sum_j v^j p_j, e_j = p_j(z), one witness
// for c) take one more pass in front of the division, in two launches of the same kind:
//   k_batch_pass   block b walks the m polynomials over its span: per polynomial a Horner per
//                  thread and a weighted TREE over the block (an evaluation needs a reduction, not
//                  a scan: 1.25 products per coefficient against the scan's 3) into a per-block
//                  total, and c's span accumulated in registers (one product per coefficient),
//                  written once at the end.  Every polynomial is read once;
//   k_batch_fold   block j folds polynomial j's totals with the weight z^S into e_j.
// The polynomials' pointers, lengths and the powers of v are a per-call table in pooled scratch (one
// H2D copy), not kernel arguments; z's weights are the division's.  Lengths may differ: N = the
// longest, a shorter polynomial is zero past its end (inside a span) and skipped in the spans behind
// it.  Traffic: (m + 1) x 32 B per coefficient.
//
// Several polynomials at several points (a SHPLONK set: e_jk = p_j(x_k)) take the same pass with K
// trees folded between one pair of barriers (k_points_pass, k_points_fold: up to kPointsPerLaunch
// points per launch, their weights in the per-call table), and the quotient by several roots is K
// runs of the division (poly_div_roots_enqueue).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "field.hpp"
#include "kzg_open.hpp"
#include "runtime.hpp"

namespace sv {

namespace {

constexpr int kT = (int)kDivPer;             // coefficients per thread
constexpr int kNT = (int)kDivThreads;        // threads per block
constexpr int kChunkQ = 2 * kT + 1;          // uint4 per thread chunk of the LDS image (16 B of padding)
constexpr int kImageQ = kNT * kChunkQ;       // uint4 in the image
constexpr int kScanQ = 2 * kNT;              // uint4 in one scan buffer
static_assert(kDivSpan == kDivThreads * kDivPer, "span = threads x coefficients per thread");
static_assert((kDivSpan & (kDivSpan - 1)) == 0 && (kDivPer & (kDivPer - 1)) == 0, "z^S and z^T by squaring");
static_assert(2 * kScanQ <= kImageQ, "the scan's two buffers live in the image");

constexpr int ilog2(uint32_t v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

__device__ __forceinline__ Fr ld_fr(const uint4* q) {
  const uint4 a = q[0], b = q[1];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_fr(uint4* q, const Fr& v) {
  q[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  q[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

constexpr int kLevels = ilog2(kDivThreads);  // levels of the block scan
static_assert((1u << kLevels) == kDivThreads, "the block scan doubles its stride per level");

// The per-call weights, by value in the kernel arguments (wave-uniform: scalar loads).
struct DivWeights {    // phases 1 and 3
  Fr z;                // Montgomery
  Fr step[kLevels];    // level l of the block scan: z^(T 2^l)
};
struct CarryWeights {  // phase 2
  Fr W;                // z^S, one block total's weight
  Fr step[kLevels];    // level l of its scan: W^(c 2^l), c totals per thread
};

// slot of the span's q-th uint4 in the padded image
__device__ __forceinline__ int image_slot(int q) { return (q / (2 * kT)) * kChunkQ + (q % (2 * kT)); }

// the span's uint4 [q0, q0 + 2 S) of src into the image, zeros past qn (the polynomial's end)
__device__ __forceinline__ void load_span(uint4* sm, const uint4* __restrict__ src, uint64_t q0, uint64_t qn) {
  uint4 v[2 * kT];
#pragma unroll
  for (int k = 0; k < 2 * kT; k++) {
    const uint64_t g = q0 + threadIdx.x + k * kNT;
    v[k] = g < qn ? src[g] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < 2 * kT; k++) sm[image_slot((int)threadIdx.x + k * kNT)] = v[k];
}

// Inclusive suffix scan over the block's threads: returns sum_{u >= t} w^(u - t) v_u for thread t,
// w = step[0] the weight of one thread step and step[l] = w^(2^l).  Every thread's result is also
// left in the returned buffer (two uint4 per thread); the caller synchronises before it overwrites sm.
__device__ __forceinline__ Fr block_suffix_scan(uint4* sm, Fr v, const Fr (&step)[kLevels], const uint4** result) {
  const int t = (int)threadIdx.x;
  uint4* cur = sm;
  uint4* nxt = sm + kScanQ;
  st_fr(cur + 2 * t, v);
  __syncthreads();
#pragma unroll
  for (int l = 0; l < kLevels; l++) {  // unrolled: step[l] is then a fixed kernel-argument offset
    const int d = 1 << l;
    if (t + d < kNT) v = v + step[l] * ld_fr(cur + 2 * (t + d));
    st_fr(nxt + 2 * t, v);
    __syncthreads();  // one barrier per level: the level after this one writes the buffer read here
    uint4* s = cur;
    cur = nxt, nxt = s;
  }
  *result = cur;
  return v;
}

__global__ void __launch_bounds__(kNT) k_div_reduce(const uint4* __restrict__ coeffs, uint64_t n, const DivWeights w,
                                                     int mont, Fr* __restrict__ totals, uint32_t* __restrict__ flags) {
  __shared__ uint4 sm[kImageQ];
  const int t = (int)threadIdx.x;
  load_span(sm, coeffs, (uint64_t)blockIdx.x * (2 * kDivSpan), 2 * n);
  __syncthreads();
  Fr acc = Fr::zero();
  bool bad = false;
#pragma unroll
  for (int k = kT - 1; k >= 0; k--) {
    Fr a = ld_fr(sm + t * kChunkQ + 2 * k);
    bad |= !a.is_reduced();
    if (!mont) a = fe_to_mont(a);
    acc = k == kT - 1 ? a : a + w.z * acc;
  }
  const int any_bad = __syncthreads_or(bad);  // also: the image is consumed, the scan reuses it
  const uint4* res;
  acc = block_suffix_scan(sm, acc, w.step, &res);
  if (t == 0) {
    totals[blockIdx.x] = acc;
    flags[blockIdx.x] = any_bad ? 1u : 0u;
  }
}

// One block over the nb block totals, c = ceil(nb / kNT) consecutive totals per thread:
// carries[b] = h_{(b + 1) S} = sum_{u > b} (z^S)^(u - b - 1) B_u, *eval = h_0, *err = any block's flag.
__global__ void __launch_bounds__(kNT) k_div_carries(const Fr* __restrict__ totals, const uint32_t* __restrict__ flags,
                                                      uint32_t nb, const CarryWeights w, int mont,
                                                      Fr* __restrict__ carries, Fr* __restrict__ eval,
                                                      uint32_t* __restrict__ err) {
  __shared__ uint4 sm[2 * kScanQ];
  const int t = (int)threadIdx.x;
  const uint32_t c = (nb + kNT - 1) / kNT;
  const uint32_t lo = (uint32_t)t * c;
  Fr acc = Fr::zero();
  uint32_t bad = 0;
  for (uint32_t k = c; k-- > 0;)
    if (lo + k < nb) {  // totals past nb are zero, and come first
      acc = totals[lo + k] + w.W * acc;
      bad |= flags[lo + k];
    }
  const int any_bad = __syncthreads_or((int)bad);
  const uint4* res;
  (void)block_suffix_scan(sm, acc, w.step, &res);
  // a thread whose chunk reaches past nb has nothing to its right, so its carry is zero and the
  // skipped (zero) totals would leave it zero
  acc = t + 1 < kNT ? ld_fr(res + 2 * (t + 1)) : Fr::zero();
  for (uint32_t k = c; k-- > 0;)
    if (lo + k < nb) {
      carries[lo + k] = acc;
      acc = totals[lo + k] + w.W * acc;
    }
  if (t == 0) {
    *eval = mont ? acc : fe_from_mont(acc);
    *err = any_bad ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(kNT) k_div_quotient(const uint4* __restrict__ coeffs, uint64_t n, const DivWeights w,
                                                       int mont, const Fr* __restrict__ carries, int q_mont,
                                                       uint4* __restrict__ quot) {
  __shared__ uint4 sm[kImageQ];
  const int t = (int)threadIdx.x;
  const uint64_t q0 = (uint64_t)blockIdx.x * (2 * kDivSpan);
  load_span(sm, coeffs, q0, 2 * n);
  __syncthreads();
  Fr a[kT];
#pragma unroll
  for (int k = 0; k < kT; k++) {
    a[k] = ld_fr(sm + t * kChunkQ + 2 * k);
    if (!mont) a[k] = fe_to_mont(a[k]);
  }
  // the block's carry enters at its last thread, so the scan gives the true h at every thread's start
  const Fr block_carry = t == kNT - 1 ? carries[blockIdx.x] : Fr::zero();
  Fr acc = block_carry;
#pragma unroll
  for (int k = kT - 1; k >= 0; k--) acc = a[k] + w.z * acc;
  __syncthreads();  // the image is consumed: the scan reuses it
  const uint4* res;
  (void)block_suffix_scan(sm, acc, w.step, &res);
  acc = t + 1 < kNT ? ld_fr(res + 2 * (t + 1)) : block_carry;  // h at the next thread's start
  __syncthreads();  // the scan's buffers are read: the image is written again
  // q_{t0 + k} = h_{t0 + k + 1}
#pragma unroll
  for (int k = kT - 1; k >= 0; k--) {
    st_fr(sm + t * kChunkQ + 2 * k, q_mont ? acc : fe_from_mont(acc));
    if (k > 0) acc = a[k] + w.z * acc;
  }
  __syncthreads();
  const uint64_t qn = 2 * (n - 1);
#pragma unroll
  for (int k = 0; k < 2 * kT; k++) {
    const int q = t + k * kNT;
    if (q0 + q < qn) quot[q0 + q] = sm[image_slot(q)];
  }
}

// ---- several polynomials at one point (poly_combine_eval_enqueue) ----
// The weighted sum sum_t w^t v_t over the block's threads, w = step[0] and step[l] = w^(2^l): a tree
// whose level l folds neighbouring pairs of the 256 >> l values left by the level before, with the
// working threads packed at the front (128, 64, 32, ... of them, so 9 wave products instead of the
// suffix scan's 32).  Thread 0 returns the sum; the last barrier comes after every read of sm, so
// the caller may overwrite sm at once.
__device__ __forceinline__ Fr block_weighted_sum(uint4* sm, Fr v, const Fr (&step)[kLevels]) {
  const int t = (int)threadIdx.x;
  uint4* cur = sm;
  uint4* nxt = sm + kScanQ;
  st_fr(cur + 2 * t, v);
  __syncthreads();
#pragma unroll
  for (int l = 0; l < kLevels; l++) {
    if (t < (kNT >> (l + 1))) {
      v = ld_fr(cur + 4 * t) + step[l] * ld_fr(cur + 4 * t + 2);
      st_fr(nxt + 2 * t, v);
    }
    __syncthreads();
    uint4* s = cur;
    cur = nxt, nxt = s;
  }
  return v;
}

// load_span in two halves, so that the next polynomial's loads are in flight during this one's
// products: the span's uint4 [q0, q0 + 2 S) of src into registers, zeros past qn ...
__device__ __forceinline__ void fetch_span(uint4 (&v)[2 * kT], const uint4* __restrict__ src, uint64_t q0, uint64_t qn) {
#pragma unroll
  for (int k = 0; k < 2 * kT; k++) {
    const uint64_t g = q0 + threadIdx.x + k * kNT;
    v[k] = g < qn ? src[g] : make_uint4(0, 0, 0, 0);
  }
}
// ... and from there into the padded image
__device__ __forceinline__ void store_span(uint4* sm, const uint4 (&v)[2 * kT]) {
#pragma unroll
  for (int k = 0; k < 2 * kT; k++) sm[image_slot((int)threadIdx.x + k * kNT)] = v[k];
}

// Block b walks the m polynomials over its span [b S, (b + 1) S): per polynomial the span's total
// B_jb = sum_k a_j[b S + k] z^k (a Horner per thread, then the tree) into totals[j nb + b], and the
// span of c = sum_j v^j a_j in registers (kCombine), stored once at the end.  A polynomial that ends
// before the span is skipped (its totals there are never read); one that ends inside it is zero
// past its end.  Every raw coefficient is checked below r; the block's flag is a plain store.
// (The form is a template parameter: with a run-time branch around the conversion inside the loop
// the compiler kept both versions of the four products alive to the loop's end, 300 registers.)
template <bool kCombine, bool kMont>
__global__ void __launch_bounds__(kNT) k_batch_pass(const BatchRow* __restrict__ table, uint32_t m, uint64_t N,
                                                     const DivWeights w, int c_mont,
                                                     uint4* __restrict__ combined, Fr* __restrict__ totals,
                                                     uint32_t* __restrict__ flags) {
  __shared__ uint4 sm[kImageQ];
  const int t = (int)threadIdx.x;
  const uint32_t nb = gridDim.x;
  const uint64_t first = (uint64_t)blockIdx.x * kDivSpan;  // the span's first coefficient
  const uint64_t q0 = 2 * first;
  Fr c[kT];
#pragma unroll
  for (int k = 0; k < kT; k++) c[k] = Fr::zero();
  bool bad = false;
  uint4 v[2 * kT];
  fetch_span(v, static_cast<const uint4*>(table[0].coeffs), q0, 2 * table[0].len);
  for (uint32_t j = 0; j < m; j++) {
    const bool live = table[j].len > first;  // the same for the whole block
    if (live) {
      store_span(sm, v);
      __syncthreads();
    }
    if (j + 1 < m) fetch_span(v, static_cast<const uint4*>(table[j + 1].coeffs), q0, 2 * table[j + 1].len);
    if (!live) continue;
    Fr vp;
    if (kCombine) memcpy(vp.v, table[j].vpow.l, sizeof vp.v);
    Fr acc = Fr::zero();
#pragma unroll
    for (int k = kT - 1; k >= 0; k--) {
      Fr a = ld_fr(sm + t * kChunkQ + 2 * k);
      bad |= !a.is_reduced();
      if (!kMont) a = fe_to_mont(a);
      acc = k == kT - 1 ? a : a + w.z * acc;
      if (kCombine) {
        c[k] = c[k] + vp * a;
        // pin the sum here: left alone, the compiler sinks the four additions to the loop's end and
        // keeps the four products alive across the tree (300 registers, one wave per SIMD)
#pragma unroll
        for (int i = 0; i < 8; i++) asm volatile("" : "+v"(c[k].v[i]));
      }
    }
    __syncthreads();  // the image is consumed: the tree reuses it
    acc = block_weighted_sum(sm, acc, w.step);
    if (t == 0) totals[(uint64_t)j * nb + blockIdx.x] = acc;
  }
  const int any_bad = __syncthreads_or(bad);
  if (t == 0) flags[blockIdx.x] = any_bad ? 1u : 0u;
  if (kCombine) {
#pragma unroll
    for (int k = 0; k < kT; k++) st_fr(sm + t * kChunkQ + 2 * k, c_mont ? c[k] : fe_from_mont(c[k]));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * kT; k++) {
      const int q = t + k * kNT;
      if (q0 + q < 2 * N) combined[q0 + q] = sm[image_slot(q)];
    }
  }
}

// Block j folds polynomial j's totals: e_j = sum_b (z^S)^b B_jb over its ceil(len_j / S) spans, with
// c = ceil(nb / kNT) consecutive totals per thread (the call's c, whatever the polynomial's length,
// so one set of weights serves every block) and the tree over the threads.  Block 0 also folds
// the flags.
__global__ void __launch_bounds__(kNT) k_batch_fold(const BatchRow* __restrict__ table, uint32_t nb,
                                                     const CarryWeights w, int mont, const Fr* __restrict__ totals,
                                                     const uint32_t* __restrict__ flags, Fr* __restrict__ evals,
                                                     uint32_t* __restrict__ err) {
  __shared__ uint4 sm[2 * kScanQ];
  const int t = (int)threadIdx.x;
  const uint32_t j = blockIdx.x;
  const uint32_t nbj = (uint32_t)((table[j].len + kDivSpan - 1) / kDivSpan);
  const uint32_t c = (nb + kNT - 1) / kNT;
  const uint32_t lo = (uint32_t)t * c;
  const Fr* mine = totals + (uint64_t)j * nb;
  Fr acc = Fr::zero();
  uint32_t bad = 0;
  for (uint32_t k = c; k-- > 0;) {
    if (lo + k < nbj) acc = mine[lo + k] + w.W * acc;  // totals past nbj are zero, and come first
    if (j == 0 && lo + k < nb) bad |= flags[lo + k];
  }
  const int any_bad = __syncthreads_or((int)bad);
  acc = block_weighted_sum(sm, acc, w.step);
  if (t == 0) {
    evals[j] = mont ? acc : fe_from_mont(acc);
    if (j == 0) *err = any_bad ? 1u : 0u;
  }
}

// ---- several polynomials at several points (poly_eval_points_enqueue) ----
// One point's row of the per-call table: the weights make_weights gives for it.
struct PointRow {
  DivWeights dw;
  CarryWeights cw;
};
static_assert(sizeof(PointRow) == kPointRowBytes, "the table's point row");

constexpr int kKP = (int)kPointsPerLaunch;  // points per launch
constexpr int kTreeAQ = kKP * kScanQ;       // uint4 of the trees' wide buffer: kKP x 256 values
constexpr int kTreeBQ = kKP * kScanQ / 2;   // ... and of the narrow one: kKP x 128 values
constexpr int kTreesQ = kTreeAQ + kTreeBQ > kImageQ ? kTreeAQ + kTreeBQ : kImageQ;  // the image shares them
constexpr int kStepsQ = kKP * kLevels * 2;  // the points' tree weights, staged once per block

// k_batch_pass without the combination and with K <= kKP points: block b walks the m polynomials
// over its span, and per polynomial every thread runs one Horner per point over the same four
// coefficients (read from the image once).  The K x 256 thread values lie one tree behind the other
// in one array, so a tree level is ONE fold of neighbouring pairs over the whole array between one
// pair of barriers -- K trees' worth of working lanes per barrier (K x 128, K x 64, ... K) where K
// passes would run K trees in sequence.  Pair i of level l belongs to tree i >> (7 - l) and takes
// that point's step[l]; below 64 pairs per tree a wave holds pairs of several trees, so the weights
// are read per lane from an LDS copy of the table's rows, not from scalar registers.  The last
// level's K pairs are the totals: totals[(j K + k) nb + b].  Flags and skipped spans as in
// k_batch_pass.
template <bool kMont>
__global__ void __launch_bounds__(kNT) k_points_pass(const BatchRow* __restrict__ table, uint32_t m,
                                                      const PointRow* __restrict__ points, uint32_t K,
                                                      Fr* __restrict__ totals, uint32_t* __restrict__ flags) {
  __shared__ uint4 sm[kTreesQ + kStepsQ];
  uint4* steps = sm + kTreesQ;  // point k's step[l] at steps + 2 (k kLevels + l)
  const int t = (int)threadIdx.x;
  const uint32_t nb = gridDim.x;
  const uint64_t first = (uint64_t)blockIdx.x * kDivSpan;
  const uint64_t q0 = 2 * first;
  for (int i = t; i < (int)K * 2 * kLevels; i += kNT)  // visible after the first live polynomial's barriers
    steps[i] = reinterpret_cast<const uint4*>(points[i / (2 * kLevels)].dw.step)[i % (2 * kLevels)];
  bool bad = false;
  uint4 v[2 * kT];
  fetch_span(v, static_cast<const uint4*>(table[0].coeffs), q0, 2 * table[0].len);
  for (uint32_t j = 0; j < m; j++) {
    const bool live = table[j].len > first;  // the same for the whole block
    if (live) {
      store_span(sm, v);
      __syncthreads();
    }
    if (j + 1 < m) fetch_span(v, static_cast<const uint4*>(table[j + 1].coeffs), q0, 2 * table[j + 1].len);
    if (!live) continue;
    Fr a[kT];
#pragma unroll
    for (int k = 0; k < kT; k++) {
      a[k] = ld_fr(sm + t * kChunkQ + 2 * k);
      bad |= !a[k].is_reduced();
      if (!kMont) a[k] = fe_to_mont(a[k]);
    }
    __syncthreads();  // the image is consumed: the trees reuse it
    for (uint32_t p = 0; p < K; p++) {
      const Fr z = points[p].dw.z;  // wave-uniform
      Fr acc = a[kT - 1];
#pragma unroll
      for (int k = kT - 2; k >= 0; k--) acc = a[k] + z * acc;
      st_fr(sm + 2 * ((int)p * kNT + t), acc);
    }
    __syncthreads();
    uint4* cur = sm;
    uint4* nxt = sm + kTreeAQ;
#pragma unroll
    for (int l = 0; l < kLevels; l++) {
      const int pairs = (int)K * (kNT >> (l + 1));
      for (int i = t; i < pairs; i += kNT) {
        const int p = i >> (kLevels - 1 - l);
        const Fr r = ld_fr(cur + 4 * i) + ld_fr(steps + 2 * (p * kLevels + l)) * ld_fr(cur + 4 * i + 2);
        if (l == kLevels - 1) totals[((uint64_t)j * K + (uint32_t)i) * nb + blockIdx.x] = r;  // i = the point
        else st_fr(nxt + 2 * i, r);
      }
      __syncthreads();  // also behind the last level: the next polynomial's image overwrites what it read
      uint4* s = cur;
      cur = nxt, nxt = s;
    }
  }
  const int any_bad = __syncthreads_or(bad);
  if (t == 0) flags[blockIdx.x] = any_bad ? 1u : 0u;
}

// Block j K + k folds polynomial j's totals at point k: k_batch_fold with the point's weights from
// the table.  evals is the call's array behind the points of earlier launches, stride = the call's
// number of points.  Block 0 also folds the flags.
__global__ void __launch_bounds__(kNT) k_points_fold(const BatchRow* __restrict__ table, uint32_t nb,
                                                      const PointRow* __restrict__ points, uint32_t K, int mont,
                                                      const Fr* __restrict__ totals, const uint32_t* __restrict__ flags,
                                                      Fr* __restrict__ evals, uint32_t stride,
                                                      uint32_t* __restrict__ err) {
  __shared__ uint4 sm[2 * kScanQ];
  const int t = (int)threadIdx.x;
  const uint32_t j = blockIdx.x / K, p = blockIdx.x % K;
  const CarryWeights& w = points[p].cw;
  const uint32_t nbj = (uint32_t)((table[j].len + kDivSpan - 1) / kDivSpan);
  const uint32_t c = (nb + kNT - 1) / kNT;
  const uint32_t lo = (uint32_t)t * c;
  const Fr* mine = totals + (uint64_t)blockIdx.x * nb;
  Fr acc = Fr::zero();
  uint32_t bad = 0;
  for (uint32_t k = c; k-- > 0;) {
    if (lo + k < nbj) acc = mine[lo + k] + w.W * acc;  // totals past nbj are zero, and come first
    if (blockIdx.x == 0 && lo + k < nb) bad |= flags[lo + k];
  }
  const int any_bad = __syncthreads_or((int)bad);
  acc = block_weighted_sum(sm, acc, w.step);
  if (t == 0) {
    evals[(uint64_t)j * stride + p] = mont ? acc : fe_from_mont(acc);
    if (blockIdx.x == 0) *err = any_bad ? 1u : 0u;
  }
}

// x^e by square and multiply (host: the per-call weights)
Fr pow_u32(const Fr& x, uint32_t e) {
  Fr r = Fr::one();
  for (int bit = 31; bit >= 0; bit--) {
    r = fe_sqr(r);
    if ((e >> bit) & 1u) r = r * x;
  }
  return r;
}

// the weights of a call over nb spans: z^T, squared per level up to z^(T 2^kLevels) = z^S, then
// (z^S)^c and its squares, c = ceil(nb / threads) totals per thread
void make_weights(const sv_fe& z, int mont, uint32_t nb, DivWeights* dw, CarryWeights* cw) {
  memcpy(dw->z.v, z.l, sizeof dw->z.v);
  if (!mont) dw->z = fe_to_mont(dw->z);
  Fr x = dw->z;
  for (int i = 0; i < ilog2(kDivPer); i++) x = fe_sqr(x);
  for (int l = 0; l < kLevels; l++) {
    dw->step[l] = x;
    x = fe_sqr(x);
  }
  cw->W = x;
  x = pow_u32(x, (nb + kDivThreads - 1) / kDivThreads);
  for (int l = 0; l < kLevels; l++) {
    cw->step[l] = x;
    x = fe_sqr(x);
  }
}

}  // namespace

size_t poly_div_scratch_bytes(size_t n) {
  const size_t nb = (n + kDivSpan - 1) / kDivSpan;
  return kDivHeadBytes + nb * (2 * sizeof(Fr) + sizeof(uint32_t));
}

int poly_div_linear_enqueue(const void* d_coeffs, size_t n, const sv_fe& z, int form, int q_form, void* d_quotient,
                            void* d_scratch, hipStream_t st) {
  static_assert(sizeof(Fr) == sizeof(sv_fe), "Fr is the ABI's element");
  if (n == 0 || n > (size_t(1) << 26)) {
    set_error("poly_div: n = %zu out of range", n);
    return SV_ERR_LEN;
  }
  const uint32_t nb = (uint32_t)((n + kDivSpan - 1) / kDivSpan);
  char* scratch = static_cast<char*>(d_scratch);
  Fr* eval = reinterpret_cast<Fr*>(scratch + kDivEvalOffset);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kDivErrOffset);
  Fr* totals = reinterpret_cast<Fr*>(scratch + kDivHeadBytes);
  Fr* carries = totals + nb;
  uint32_t* flags = reinterpret_cast<uint32_t*>(carries + nb);
  const int mont = form == SV_MONTGOMERY ? 1 : 0;
  DivWeights dw;
  CarryWeights cw;
  make_weights(z, mont, nb, &dw, &cw);
  const uint4* c = static_cast<const uint4*>(d_coeffs);
  hipLaunchKernelGGL(k_div_reduce, dim3(nb), dim3(kNT), 0, st, c, (uint64_t)n, dw, mont, totals, flags);
  hipLaunchKernelGGL(k_div_carries, dim3(1), dim3(kNT), 0, st, totals, flags, nb, cw, mont, carries, eval, err);
  if (d_quotient && n > 1)
    hipLaunchKernelGGL(k_div_quotient, dim3(nb), dim3(kNT), 0, st, c, (uint64_t)n, dw, mont, carries,
                       q_form == SV_MONTGOMERY ? 1 : 0, static_cast<uint4*>(d_quotient));
  SV_HIP(hipGetLastError());
  return SV_OK;
}

sv_fe poly_fr_to_mont(const sv_fe& canonical) {
  Fr x;
  memcpy(x.v, canonical.l, sizeof x.v);
  x = fe_to_mont(x);
  sv_fe out;
  memcpy(out.l, x.v, sizeof x.v);
  return out;
}

void poly_batch_fill_table_weights(BatchRow* rows, const sv_fe* const* d_polys, const uint64_t* lens, size_t m,
                                   const sv_fe* weights, int form) {
  for (size_t j = 0; j < m; j++) {
    rows[j].coeffs = d_polys[j];
    rows[j].len = lens[j];
    rows[j].vpow = form == SV_MONTGOMERY ? weights[j] : poly_fr_to_mont(weights[j]);
  }
}

void poly_batch_fill_table(BatchRow* rows, const sv_fe* const* d_polys, const uint64_t* lens, size_t m, const sv_fe& v,
                           int form) {
  Fr vm;
  memcpy(vm.v, v.l, sizeof vm.v);
  if (form != SV_MONTGOMERY) vm = fe_to_mont(vm);
  std::vector<sv_fe> pw(m);
  Fr p = Fr::one();
  for (size_t j = 0; j < m; j++) {
    memcpy(pw[j].l, p.v, sizeof p.v);
    p = p * vm;
  }
  poly_batch_fill_table_weights(rows, d_polys, lens, m, pw.data(), SV_MONTGOMERY);
}

size_t poly_batch_scratch_bytes(size_t m, size_t N) {
  const size_t nb = (N + kDivSpan - 1) / kDivSpan;
  return poly_batch_head_bytes(m) + m * nb * sizeof(Fr) + nb * sizeof(uint32_t);
}

int poly_combine_eval_enqueue(const BatchRow* d_table, size_t m, size_t N, const sv_fe& z, int form, int c_form,
                              void* d_combined, void* d_scratch, hipStream_t st) {
  if (m == 0 || m > SV_OPEN_BATCH_MAX || N == 0 || N > (size_t(1) << 26)) {
    set_error("poly_combine_eval: m = %zu, N = %zu out of range", m, N);
    return SV_ERR_LEN;
  }
  const uint32_t nb = (uint32_t)((N + kDivSpan - 1) / kDivSpan);
  char* scratch = static_cast<char*>(d_scratch);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kBatchErrOffset);
  Fr* evals = reinterpret_cast<Fr*>(scratch + kBatchEvalsOffset);
  Fr* totals = evals + m;
  uint32_t* flags = reinterpret_cast<uint32_t*>(totals + m * (size_t)nb);
  const int mont = form == SV_MONTGOMERY ? 1 : 0;
  const int c_mont = c_form == SV_MONTGOMERY ? 1 : 0;
  DivWeights dw;
  CarryWeights cw;
  make_weights(z, mont, nb, &dw, &cw);
  auto pass = d_combined ? (mont ? k_batch_pass<true, true> : k_batch_pass<true, false>)
                         : (mont ? k_batch_pass<false, true> : k_batch_pass<false, false>);
  hipLaunchKernelGGL(pass, dim3(nb), dim3(kNT), 0, st, d_table, (uint32_t)m, (uint64_t)N, dw, c_mont,
                     static_cast<uint4*>(d_combined), totals, flags);
  hipLaunchKernelGGL(k_batch_fold, dim3((uint32_t)m), dim3(kNT), 0, st, d_table, nb, cw, mont, totals, flags, evals,
                     err);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

void poly_points_fill_rows(void* rows, const sv_fe* points, size_t K, int form, size_t N) {
  const uint32_t nb = (uint32_t)((N + kDivSpan - 1) / kDivSpan);
  PointRow* r = static_cast<PointRow*>(rows);
  for (size_t k = 0; k < K; k++) make_weights(points[k], form == SV_MONTGOMERY ? 1 : 0, nb, &r[k].dw, &r[k].cw);
}

size_t poly_points_scratch_bytes(size_t m, size_t K, size_t N) {
  const size_t nb = (N + kDivSpan - 1) / kDivSpan;
  const size_t kc = K < kPointsPerLaunch ? K : kPointsPerLaunch;
  return poly_points_head_bytes(m, K) + m * kc * nb * sizeof(Fr) + nb * sizeof(uint32_t);
}

int poly_eval_points_enqueue(const BatchRow* d_table, size_t m, size_t N, const void* d_points, const void* h_points,
                             size_t K, int form, void* d_scratch, hipStream_t st) {
  if (m == 0 || m > SV_OPEN_BATCH_MAX || K == 0 || K > SV_EVAL_POINTS_MAX || N == 0 || N > (size_t(1) << 26)) {
    set_error("poly_eval_points: m = %zu, K = %zu, N = %zu out of range", m, K, N);
    return SV_ERR_LEN;
  }
  const uint32_t nb = (uint32_t)((N + kDivSpan - 1) / kDivSpan);
  const size_t kc = K < kPointsPerLaunch ? K : kPointsPerLaunch;
  char* scratch = static_cast<char*>(d_scratch);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kPointsErrOffset);
  Fr* evals = reinterpret_cast<Fr*>(scratch + kPointsEvalsOffset);
  Fr* totals = evals + m * K;
  uint32_t* flags = reinterpret_cast<uint32_t*>(totals + m * kc * (size_t)nb);
  const int mont = form == SV_MONTGOMERY ? 1 : 0;
  const PointRow* points = static_cast<const PointRow*>(d_points);
  if (K == 1) {
    // one point is the evaluate-only k_batch_pass, whose weights are scalar registers: at 2^20
    // coefficients it is 7 % faster than the multi-point pass with one tree (0.584 against 0.623 ms
    // at m = 16; equal within the spread at 2^16 and 2^18).  Same totals, same head.
    const PointRow& w = *static_cast<const PointRow*>(h_points);
    auto one = mont ? k_batch_pass<false, true> : k_batch_pass<false, false>;
    hipLaunchKernelGGL(one, dim3(nb), dim3(kNT), 0, st, d_table, (uint32_t)m, (uint64_t)N, w.dw, 0,
                       static_cast<uint4*>(nullptr), totals, flags);
    hipLaunchKernelGGL(k_batch_fold, dim3((uint32_t)m), dim3(kNT), 0, st, d_table, nb, w.cw, mont, totals, flags, evals,
                       err);
    SV_HIP(hipGetLastError());
    return SV_OK;
  }
  auto pass = mont ? k_points_pass<true> : k_points_pass<false>;
  // the launches share the totals and the flags (every launch checks every coefficient): stream order
  for (size_t k0 = 0; k0 < K; k0 += kPointsPerLaunch) {
    const uint32_t kn = (uint32_t)(K - k0 < kPointsPerLaunch ? K - k0 : kPointsPerLaunch);
    hipLaunchKernelGGL(pass, dim3(nb), dim3(kNT), 0, st, d_table, (uint32_t)m, points + k0, kn, totals, flags);
    hipLaunchKernelGGL(k_points_fold, dim3((uint32_t)m * kn), dim3(kNT), 0, st, d_table, nb, points + k0, kn, mont,
                       totals, flags, evals + k0, (uint32_t)K, err);
  }
  SV_HIP(hipGetLastError());
  return SV_OK;
}

namespace {
size_t div_scratch_aligned(size_t n) { return (poly_div_scratch_bytes(n) + 255) & ~size_t(255); }
}  // namespace

size_t poly_div_roots_scratch_bytes(size_t n, size_t K) { return (K > 1 ? 2 : 1) * div_scratch_aligned(n); }

int poly_div_roots_enqueue(const void* d_coeffs, size_t n, const sv_fe* roots, size_t K, int form, int q_form,
                           void* d_quotient, void* const d_tmp[2], void* d_scratch, hipStream_t st) {
  if (K == 0 || n <= K) {
    set_error("poly_div_roots: n = %zu coefficients, K = %zu roots", n, K);
    return SV_ERR_ARG;
  }
  const void* src = d_coeffs;
  int src_form = form;
  for (size_t k = 0; k < K; k++) {
    const bool last = k + 1 == K;
    void* dst = last ? d_quotient : d_tmp[k & 1];
    // a root goes in the form of the coefficients it divides: the call's, then Montgomery
    const sv_fe x = src_form == form || form == SV_MONTGOMERY ? roots[k] : poly_fr_to_mont(roots[k]);
    char* scratch = static_cast<char*>(d_scratch) + (k == 0 ? 0 : div_scratch_aligned(n));
    const int rc = poly_div_linear_enqueue(src, n - k, x, src_form, last ? q_form : SV_MONTGOMERY, dst, scratch, st);
    if (rc != SV_OK) return rc;
    src = dst;
    src_form = SV_MONTGOMERY;
  }
  return SV_OK;
}

namespace {
Fr fr_in(const sv_fe& a) {
  Fr x;
  memcpy(x.v, a.l, sizeof x.v);
  return x;
}
sv_fe fr_out(const Fr& x) {
  sv_fe a;
  memcpy(a.l, x.v, sizeof x.v);
  return a;
}
}  // namespace

sv_fe poly_fr_mul(const sv_fe& a, const sv_fe& b) { return fr_out(fr_in(a) * fr_in(b)); }
sv_fe poly_fr_sub(const sv_fe& a, const sv_fe& b) { return fr_out(fr_in(a) - fr_in(b)); }
sv_fe poly_fr_inv(const sv_fe& a) { return fr_out(fe_inv(fr_in(a))); }
sv_fe poly_fr_one() { return fr_out(Fr::one()); }

}  // namespace sv
