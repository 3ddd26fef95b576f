// A stable sort of a BN254 Fr column by canonical value, and halo2's permute_expression_pair on top
// of it: the permuted columns A', S' of a lookup argument, for columns that are already in HBM.
//
// The sort is a least-significant-digit radix sort, keys only, over the canonical 256-bit value in
// 32 digits of 8 bits.  Every phase is a launch of its own on the call's stream and no block ever
// waits for another block (kzg_open.hip's division has the reason: no look-back on a shared device):
//   k_lp_first    reads the column once: Montgomery data becomes canonical with one multiplication,
//                 every element is tested below r (the error flag), the canonical image is written,
//                 and ALL 32 digit histograms are built at once: 32 x 256 counters in LDS per block
//                 (32 KiB), folded into global memory with one atomic per non-empty bin;
//   k_lp_plan     one block: a digit whose histogram has a single non-empty bin moves nothing, so
//                 its pass is dead; the live passes get the image they read (ping-pong parity), the
//                 histograms become the digits' global bases, and the image that holds the result
//                 is recorded.  The host never learns which passes are live: all 32 are enqueued and
//                 a dead pass's three launches return at their first instruction;
//   per pass      k_lp_count    per-block digit counts (LDS atomics), stored digit-major;
//                 k_lp_offsets  one block per digit scans that digit's counts over the blocks into
//                               global offsets (base of the digit + the blocks before);
//                 k_lp_scatter  the STABLE scatter: a wave matches its 64 keys' digits with eight
//                               ballots, so a key's rank among equal digits in its wave is a popcount
//                               of the lanes below it; the runs' counts go through LDS, where one
//                               thread per digit turns them into positions in run order, which is
//                               input order;
//   k_lp_finish   converts the final image back to `form` into the destination, whatever the parity
//                 of the number of live passes (zero included: n == 1, all keys equal).
//
// The permutation sorts A into image pair 0 and S into image pair 1 (T = sorted S), writes A' from
// the first, and then:
//   k_lp_leaders  row i of A' is a leader if i == 0 or A'[i] != A'[i - 1]; a leader takes the lower
//                 bound p of its value in T and marks used[p] if T[p] is that value (the FIRST copy of
//                 it in T), or folds its row into the missing-row word (an atomicMax of UINT64_MAX -
//                 row, so the smallest row wins); the others are the repeats;
//   k_lp_totals, k_lp_carries, k_lp_lists
//                 the exclusive scans over `repeat` and over `!used` in the block / carries pattern of
//                 grand_product.hip (block totals, one block over the totals, blocks again with their
//                 carries): rep_row[k] = the k-th repeated row, un_pos[j] = the j-th unused position
//                 of T, i.e. L[j] = T[un_pos[j]] without materialising L; m = the number of repeats;
//   k_lp_write    S'[i] = A'[i] at a leader, and for k < m S'[rep_row[k]] = T[un_pos[m - 1 - k]]: the
//                 smallest leftover goes to the last repeated row, as halo2's pop() does.
// Comparisons are on the canonical images; the outputs are converted to `form` where they are written.
//
// Every kernel's work is a __device__ body (lp_*) with two entry kernels around it.  k_lp_* are the
// single calls' entries, with the pointers of their one column as kernel parameters: a sort is 99
// launches, a permutation 202, its two sorts one after the other.  k_lpb_* are the batch call's
// entries with a column dimension, blockIdx.y: a call's columns are its lookups' inputs and, after
// them, its distinct tables (csrc/lp_batch_plan.hpp names them); each sorted column has its own state,
// image pair and per-block counts, and each lookup its own head, flag and list arrays, totals and
// carries, and an entry finds its column's pointers in the by-value LpGeom.  One set of launches
// serves every column: the blocks of a column for which a pass is dead return at their first
// instruction while the other columns' blocks run: 104 kernels whatever the number of lookups.  A table
// the caller has sorted skips the radix sort: k_lpb_table converts it into its one image and checks
// T[i - 1] <= T[i] (one more launch, 105).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "field.hpp"
#include "lookup_permute.hpp"
#include "lp_batch_plan.hpp"
#include "runtime.hpp"

namespace sv {

namespace {

constexpr int kNT = (int)kLpThreads;
constexpr int kPer = (int)kLpPer;
constexpr int kWave = 64;
constexpr int kRuns = (int)kLpTile / kWave;  // runs of 64 consecutive keys per tile
constexpr uint32_t kFirstBlocksMax = 256;    // k_lp_first strides over the tiles: bounds its global atomics
static_assert(kLpTile == kLpThreads * kLpPer, "tile = threads x keys per thread");
static_assert(kLpThreads == 256, "one thread per digit value");
static_assert(kLpThreads % kWave == 0, "whole waves");

// Per sorted column: the histograms (after k_lp_plan: the digits' exclusive bases), the plan of
// every pass (bit 0: live, bit 1: the image it reads) and the image that holds the sorted keys.
struct LpState {
  uint32_t hist[kLpDigits][256];
  uint32_t plan[kLpDigits];
  uint32_t final_image;
  uint32_t pad[31];
};
static_assert(sizeof(LpState) % 256 == 0, "regions stay 256-byte aligned");

struct LpHead {
  uint32_t err, pad0;
  unsigned long long missing;  // UINT64_MAX - row, 0 = none
  uint32_t repeats, pad1;      // m
  uint32_t pad2[10];           // a batch has one head per lookup, kLpHeadBytes apart
};
static_assert(sizeof(LpHead) == kLpHeadBytes && offsetof(LpHead, missing) == kLpMissingOffset, "head layout");
constexpr uint32_t kErrNotReduced = kLpErrNotReduced, kErrNotSorted = kLpErrNotSorted;  // bits of heads[0].err

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
__device__ __forceinline__ bool key_less(const Fr& a, const Fr& b) {
  bool lt = false;
#pragma unroll
  for (int i = 0; i < 8; i++) lt = a.v[i] != b.v[i] ? a.v[i] < b.v[i] : lt;  // the highest differing limb decides
  return lt;
}
__device__ __forceinline__ uint32_t key_digit(const Fr& a, uint32_t pass) {
  return (a.v[pass >> 2] >> ((pass & 3u) * 8)) & 255u;
}

// Exclusive prefix sums of a and of b over the block's threads (Hillis-Steele in LDS, one barrier
// per level); ta and tb take the block's totals.  sm: 4 * kNT words, free again on return.
__device__ __forceinline__ void block_exscan2(uint32_t* sm, uint32_t& a, uint32_t& b, uint32_t& ta, uint32_t& tb) {
  const int t = (int)threadIdx.x;
  uint32_t* cur = sm;
  uint32_t* nxt = sm + 2 * kNT;
  const uint32_t a0 = a, b0 = b;
  cur[t] = a, cur[kNT + t] = b;
  __syncthreads();
#pragma unroll 1
  for (int d = 1; d < kNT; d <<= 1) {
    if (t >= d) a += cur[t - d], b += cur[kNT + t - d];
    nxt[t] = a, nxt[kNT + t] = b;
    __syncthreads();
    uint32_t* x = cur;
    cur = nxt, nxt = x;
  }
  ta = cur[kNT - 1], tb = cur[2 * kNT - 1];
  a -= a0, b -= b0;
  __syncthreads();
}

// ---- the bodies ------------------------------------------------------------------------------------

template <bool kMont>
__device__ __forceinline__ void lp_first(const uint4* __restrict__ in, uint4* __restrict__ image, uint32_t n, uint32_t nb,
                                         LpState* __restrict__ state, LpHead* __restrict__ head) {
  __shared__ uint32_t h[kLpDigits * 256];
  const int t = (int)threadIdx.x;
  for (int e = t; e < (int)kLpDigits * 256; e += kNT) h[e] = 0;
  __syncthreads();
  bool bad = false;
  for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < kPer; j++) {
      const uint32_t i = tile * kLpTile + (uint32_t)(j * kNT + t);
      if (i < n) {
        Fr a = ld_fr(in + 2 * (size_t)i);
        bad |= !a.is_reduced();
        if (kMont) a = fe_from_mont(a);
        st_fr(image + 2 * (size_t)i, a);
#pragma unroll
        for (uint32_t p = 0; p < kLpDigits; p++) atomicAdd(&h[p * 256 + key_digit(a, p)], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* g = &state->hist[0][0];
  for (int e = t; e < (int)kLpDigits * 256; e += kNT)
    if (h[e]) atomicAdd(g + e, h[e]);
  if (bad) atomicOr(&head->err, kErrNotReduced);
}

// A table the caller has sorted: the one pass that reads it.  The canonical image is written, every
// element is tested below r, and element i is compared with element i - 1 (read and converted again:
// a tile's first element has its predecessor in another block).
template <bool kMont>
__device__ __forceinline__ void lp_table(const uint4* __restrict__ in, uint4* __restrict__ image, uint32_t n, uint32_t nb,
                                         LpHead* __restrict__ head) {
  const int t = (int)threadIdx.x;
  bool bad = false, unsorted = false;
  for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < kPer; j++) {
      const uint32_t i = tile * kLpTile + (uint32_t)(j * kNT + t);
      if (i < n) {
        Fr a = ld_fr(in + 2 * (size_t)i);
        bad |= !a.is_reduced();
        if (kMont) a = fe_from_mont(a);
        st_fr(image + 2 * (size_t)i, a);
        if (i > 0) {
          Fr b = ld_fr(in + 2 * (size_t)(i - 1));
          if (kMont) b = fe_from_mont(b);
          unsorted |= key_less(a, b);
        }
      }
    }
  }
  if (bad) atomicOr(&head->err, kErrNotReduced);
  if (unsorted) atomicOr(&head->err, kErrNotSorted);
}

__device__ __forceinline__ void lp_plan(LpState* __restrict__ state) {
  __shared__ uint32_t sm[4 * kNT];
  const int t = (int)threadIdx.x;
  uint32_t image = 0;
  for (uint32_t p = 0; p < kLpDigits; p++) {
    uint32_t v = state->hist[p][t], one = v != 0, tv, bins;
    block_exscan2(sm, v, one, tv, bins);
    state->hist[p][t] = v;
    const uint32_t live = bins > 1;
    if (t == 0) state->plan[p] = live | (image << 1);
    image ^= live;
  }
  if (t == 0) state->final_image = image;
}

__device__ __forceinline__ void lp_count(const LpState* __restrict__ state, uint32_t pass, const uint32_t* __restrict__ img0,
                                         const uint32_t* __restrict__ img1, uint32_t n, uint32_t* __restrict__ counts) {
  const uint32_t pw = state->plan[pass];
  if (!(pw & 1u)) return;
  __shared__ uint32_t h[256];
  const int t = (int)threadIdx.x;
  const uint32_t* src = (pw & 2u) ? img1 : img0;
  h[t] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t i = blockIdx.x * kLpTile + (uint32_t)(j * kNT + t);
    if (i < n) atomicAdd(&h[(src[8 * (size_t)i + (pass >> 2)] >> ((pass & 3u) * 8)) & 255u], 1u);
  }
  __syncthreads();
  counts[(size_t)t * gridDim.x + blockIdx.x] = h[t];
}

// Block d: the counts of digit d over the nb blocks, c = ceil(nb / kNT) consecutive ones per thread,
// become the positions at which the blocks' keys of that digit start.
__device__ __forceinline__ void lp_offsets(const LpState* __restrict__ state, uint32_t pass, uint32_t nb,
                                           uint32_t* __restrict__ counts) {
  if (!(state->plan[pass] & 1u)) return;
  __shared__ uint32_t sm[4 * kNT];
  const int t = (int)threadIdx.x;
  uint32_t* row = counts + (size_t)blockIdx.x * nb;
  const uint32_t c = (nb + kNT - 1) / kNT;
  const uint32_t lo = (uint32_t)t * c;
  uint32_t s = 0, z = 0, ts, tz;
  for (uint32_t k = 0; k < c; k++)
    if (lo + k < nb) s += row[lo + k];
  block_exscan2(sm, s, z, ts, tz);
  s += state->hist[pass][blockIdx.x];
  for (uint32_t k = 0; k < c; k++)
    if (lo + k < nb) {
      const uint32_t v = row[lo + k];
      row[lo + k] = s;
      s += v;
    }
}

__device__ __forceinline__ void lp_scatter(const LpState* __restrict__ state, uint32_t pass, uint4* __restrict__ img0,
                                           uint4* __restrict__ img1, uint32_t n, const uint32_t* __restrict__ offsets) {
  const uint32_t pw = state->plan[pass];
  if (!(pw & 1u)) return;
  __shared__ uint32_t cnt[kRuns * 256];
  const int t = (int)threadIdx.x;
  const int lane = t % kWave, wave = t / kWave;
  const uint4* src = (pw & 2u) ? img1 : img0;
  uint4* dst = (pw & 2u) ? img0 : img1;
  for (int e = t; e < kRuns * 256; e += kNT) cnt[e] = 0;
  __syncthreads();
  Fr key[kPer];
  uint32_t dig[kPer], rank[kPer];
  bool ok[kPer];
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const int run = wave * kPer + j;
    const uint32_t i = blockIdx.x * kLpTile + (uint32_t)(run * kWave + lane);
    ok[j] = i < n;
    key[j] = ok[j] ? ld_fr(src + 2 * (size_t)i) : Fr::zero();
    dig[j] = key_digit(key[j], pass);
    unsigned long long same = __ballot(ok[j]);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (dig[j] >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    rank[j] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (ok[j] && rank[j] == 0) cnt[run * 256 + dig[j]] = (uint32_t)__popcll(same);
  }
  __syncthreads();
  {
    uint32_t at = offsets[(size_t)t * gridDim.x + blockIdx.x];  // thread t: digit t, runs in input order
    for (int run = 0; run < kRuns; run++) {
      const uint32_t v = cnt[run * 256 + t];
      cnt[run * 256 + t] = at;
      at += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const int run = wave * kPer + j;
    if (ok[j]) st_fr(dst + 2 * (size_t)(cnt[run * 256 + dig[j]] + rank[j]), key[j]);
  }
}

__device__ __forceinline__ const uint4* final_image(const LpState* state, const uint4* img0, const uint4* img1) {
  return state->final_image ? img1 : img0;
}

// src: the image that holds the sorted keys
template <bool kMont>
__device__ __forceinline__ void lp_finish(const uint4* __restrict__ src, uint32_t n, uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  const Fr a = ld_fr(src + 2 * (size_t)i);
  st_fr(out + 2 * (size_t)i, kMont ? fe_to_mont(a) : a);
}

// A = the sorted input, T = the sorted table
__device__ __forceinline__ void lp_leaders(const uint4* A, const uint4* T, uint32_t n, uint32_t* __restrict__ repeat,
                                           uint32_t* __restrict__ used, LpHead* __restrict__ head) {
  const uint32_t i = blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  const Fr a = ld_fr(A + 2 * (size_t)i);
  const bool leader = i == 0 || ld_fr(A + 2 * (size_t)(i - 1)) != a;
  repeat[i] = leader ? 0u : 1u;
  if (!leader) return;
  uint32_t lo = 0, hi = n;  // the lower bound of a in T: the first p with T[p] >= a, n when there is none
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (key_less(ld_fr(T + 2 * (size_t)mid), a)) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n && ld_fr(T + 2 * (size_t)lo) == a) used[lo] = 1u;
  else atomicMax(&head->missing, ~0ull - (unsigned long long)i);
}

// This thread's kPer consecutive rows of the two flag columns: repeat, and !used.
__device__ __forceinline__ void load_flags(const uint32_t* repeat, const uint32_t* used, uint32_t n, uint32_t (&r)[kPer],
                                           uint32_t (&u)[kPer]) {
  const uint32_t row0 = blockIdx.x * kLpTile + threadIdx.x * kLpPer;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const bool live = row0 + k < n;
    r[k] = live ? repeat[row0 + k] : 0u;
    u[k] = live ? 1u - used[row0 + k] : 0u;
  }
}

__device__ __forceinline__ void lp_totals(const uint32_t* __restrict__ repeat, const uint32_t* __restrict__ used, uint32_t n,
                                          uint32_t* __restrict__ totals) {
  __shared__ uint32_t sm[4 * kNT];
  uint32_t r[kPer], u[kPer], a = 0, b = 0, ta, tb;
  load_flags(repeat, used, n, r, u);
#pragma unroll
  for (int k = 0; k < kPer; k++) a += r[k], b += u[k];
  block_exscan2(sm, a, b, ta, tb);
  if (threadIdx.x == 0) totals[blockIdx.x] = ta, totals[gridDim.x + blockIdx.x] = tb;
}

// One block over the nb pairs of block totals, c = ceil(nb / kNT) consecutive pairs per thread.
__device__ __forceinline__ void lp_carries(const uint32_t* __restrict__ totals, uint32_t nb, uint32_t* __restrict__ carries,
                                           LpHead* __restrict__ head) {
  __shared__ uint32_t sm[4 * kNT];
  const int t = (int)threadIdx.x;
  const uint32_t c = (nb + kNT - 1) / kNT;
  const uint32_t lo = (uint32_t)t * c;
  uint32_t a = 0, b = 0, ta, tb;
  for (uint32_t k = 0; k < c; k++)
    if (lo + k < nb) a += totals[lo + k], b += totals[nb + lo + k];
  block_exscan2(sm, a, b, ta, tb);
  for (uint32_t k = 0; k < c; k++)
    if (lo + k < nb) {
      carries[lo + k] = a, carries[nb + lo + k] = b;
      a += totals[lo + k], b += totals[nb + lo + k];
    }
  if (t == 0) head->repeats = ta;
}

__device__ __forceinline__ void lp_lists(const uint32_t* __restrict__ repeat, const uint32_t* __restrict__ used, uint32_t n,
                                         const uint32_t* __restrict__ carries, uint32_t* __restrict__ rep_row,
                                         uint32_t* __restrict__ un_pos) {
  __shared__ uint32_t sm[4 * kNT];
  uint32_t r[kPer], u[kPer], a = 0, b = 0, ta, tb;
  load_flags(repeat, used, n, r, u);
#pragma unroll
  for (int k = 0; k < kPer; k++) a += r[k], b += u[k];
  block_exscan2(sm, a, b, ta, tb);
  a += carries[blockIdx.x], b += carries[gridDim.x + blockIdx.x];
  const uint32_t row0 = blockIdx.x * kLpTile + threadIdx.x * kLpPer;
#pragma unroll
  for (int k = 0; k < kPer; k++) {  // a flag is 0 past the last row, and a and b stay below n
    if (r[k]) rep_row[a++] = row0 + k;
    if (u[k]) un_pos[b++] = row0 + k;
  }
}

template <bool kMont>
__device__ __forceinline__ void lp_write(const uint4* A, const uint4* T, uint32_t n, const uint32_t* __restrict__ repeat,
                                         const uint32_t* __restrict__ rep_row, const uint32_t* __restrict__ un_pos,
                                         const LpHead* __restrict__ head, uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  if (!repeat[i]) {
    const Fr a = ld_fr(A + 2 * (size_t)i);
    st_fr(out + 2 * (size_t)i, kMont ? fe_to_mont(a) : a);
  }
  const uint32_t m = head->repeats;  // a failed lookup has more unused positions than repeats: still in range
  if (i < m) {
    const Fr l = ld_fr(T + 2 * (size_t)un_pos[m - 1 - i]);
    st_fr(out + 2 * (size_t)rep_row[i], kMont ? fe_to_mont(l) : l);
  }
}

// ---- the single calls' entries: one column, its pointers as kernel parameters ---------------------

template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lp_first(const uint4* __restrict__ in, uint4* __restrict__ image, uint32_t n,
                                                  uint32_t nb, LpState* __restrict__ state, LpHead* __restrict__ head) {
  lp_first<kMont>(in, image, n, nb, state, head);
}

__global__ void __launch_bounds__(kNT) k_lp_plan(LpState* __restrict__ state) { lp_plan(state); }

__global__ void __launch_bounds__(kNT) k_lp_count(const LpState* __restrict__ state, uint32_t pass,
                                                  const uint32_t* __restrict__ img0, const uint32_t* __restrict__ img1,
                                                  uint32_t n, uint32_t* __restrict__ counts) {
  lp_count(state, pass, img0, img1, n, counts);
}

__global__ void __launch_bounds__(kNT) k_lp_offsets(const LpState* __restrict__ state, uint32_t pass, uint32_t nb,
                                                    uint32_t* __restrict__ counts) {
  lp_offsets(state, pass, nb, counts);
}

__global__ void __launch_bounds__(kNT) k_lp_scatter(const LpState* __restrict__ state, uint32_t pass,
                                                    uint4* __restrict__ img0, uint4* __restrict__ img1, uint32_t n,
                                                    const uint32_t* __restrict__ offsets) {
  lp_scatter(state, pass, img0, img1, n, offsets);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lp_finish(const LpState* __restrict__ state, const uint4* __restrict__ img0,
                                                   const uint4* __restrict__ img1, uint32_t n, uint4* __restrict__ out) {
  lp_finish<kMont>(final_image(state, img0, img1), n, out);
}

// The images of the permutation: A' = the final image of pair a, T = that of pair s.
struct LpImages {
  const LpState* sa;
  const LpState* ss;
  const uint4 *a0, *a1, *s0, *s1;
};

__global__ void __launch_bounds__(kNT) k_lp_leaders(const LpImages im, uint32_t n, uint32_t* __restrict__ repeat,
                                                    uint32_t* __restrict__ used, LpHead* __restrict__ head) {
  lp_leaders(final_image(im.sa, im.a0, im.a1), final_image(im.ss, im.s0, im.s1), n, repeat, used, head);
}

__global__ void __launch_bounds__(kNT) k_lp_totals(const uint32_t* __restrict__ repeat, const uint32_t* __restrict__ used,
                                                   uint32_t n, uint32_t* __restrict__ totals) {
  lp_totals(repeat, used, n, totals);
}

__global__ void __launch_bounds__(kNT) k_lp_carries(const uint32_t* __restrict__ totals, uint32_t nb,
                                                    uint32_t* __restrict__ carries, LpHead* __restrict__ head) {
  lp_carries(totals, nb, carries, head);
}

__global__ void __launch_bounds__(kNT) k_lp_lists(const uint32_t* __restrict__ repeat, const uint32_t* __restrict__ used,
                                                  uint32_t n, const uint32_t* __restrict__ carries,
                                                  uint32_t* __restrict__ rep_row, uint32_t* __restrict__ un_pos) {
  lp_lists(repeat, used, n, carries, rep_row, un_pos);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lp_write(const LpImages im, uint32_t n, const uint32_t* __restrict__ repeat,
                                                  const uint32_t* __restrict__ rep_row, const uint32_t* __restrict__ un_pos,
                                                  const LpHead* __restrict__ head, uint4* __restrict__ out) {
  lp_write<kMont>(final_image(im.sa, im.a0, im.a1), final_image(im.ss, im.s0, im.s1), n, repeat, rep_row, un_pos, head, out);
}

// ---- the batch call's entries: a column dimension ------------------------------------------------

// What every batch kernel is given by value.  A call has columns: the lookups' inputs are columns
// [0, lookups), the tables come after them.  The first sorted_cols columns go through the radix sort
// and have a state, a block of per-block counts and an image pair; a column past them is a table the
// caller has sorted, with one image.  A sort launch covers the columns blockIdx.y; lookup j of the
// permutation's kernels is blockIdx.y.  The per-lookup arrays are strided by lookup.
struct LpGeom {
  LpHead* heads;     // lookup j: heads[j]; heads[0].err is the whole call's
  LpState* states;   // column c < sorted_cols
  uint4* images;     // column c < sorted_cols: images 2c, 2c + 1; past them one each
  uint32_t* counts;  // column c < sorted_cols
  uint32_t *repeat, *used, *rep_row, *un_pos, *totals, *carries;
  size_t image_stride, counts_stride, flag_stride, tot_stride;  // in uint4, u32, u32, u32
  uint32_t n, nb;
  uint32_t sorted_cols;
  uint8_t table_col[kLpbMax];  // the column of lookup j's table
};
struct LpIn {
  const uint4* p[2 * kLpbMax];  // by column of the launch
};
struct LpOut {
  uint4* p[kLpbMax];
};

__device__ __forceinline__ uint4* image_of(const LpGeom& g, uint32_t c, uint32_t parity) {
  const size_t k = c < g.sorted_cols ? 2 * (size_t)c + parity : 2 * (size_t)g.sorted_cols + (c - g.sorted_cols);
  return g.images + k * g.image_stride;
}
// the image that holds column c's sorted keys
__device__ __forceinline__ const uint4* sorted_image(const LpGeom& g, uint32_t c) {
  return image_of(g, c, c < g.sorted_cols ? g.states[c].final_image : 0u);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lpb_first(const LpIn ins, const LpGeom g) {
  const uint32_t c = blockIdx.y;
  lp_first<kMont>(ins.p[c], image_of(g, c, 0), g.n, g.nb, g.states + c, g.heads);
}

// the table slots: columns col0 + blockIdx.y, past the sorted ones
template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lpb_table(const LpIn tabs, const LpGeom g, uint32_t col0) {
  lp_table<kMont>(tabs.p[blockIdx.y], image_of(g, col0 + blockIdx.y, 0), g.n, g.nb, g.heads);
}

__global__ void __launch_bounds__(kNT) k_lpb_plan(const LpGeom g) { lp_plan(g.states + blockIdx.y); }

__global__ void __launch_bounds__(kNT) k_lpb_count(const LpGeom g, uint32_t pass) {
  const uint32_t c = blockIdx.y;
  lp_count(g.states + c, pass, reinterpret_cast<const uint32_t*>(image_of(g, c, 0)),
           reinterpret_cast<const uint32_t*>(image_of(g, c, 1)), g.n, g.counts + c * g.counts_stride);
}

__global__ void __launch_bounds__(kNT) k_lpb_offsets(const LpGeom g, uint32_t pass) {
  const uint32_t c = blockIdx.y;
  lp_offsets(g.states + c, pass, g.nb, g.counts + c * g.counts_stride);
}

__global__ void __launch_bounds__(kNT) k_lpb_scatter(const LpGeom g, uint32_t pass) {
  const uint32_t c = blockIdx.y;
  lp_scatter(g.states + c, pass, image_of(g, c, 0), image_of(g, c, 1), g.n, g.counts + c * g.counts_stride);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lpb_finish(const LpOut outs, const LpGeom g) {
  lp_finish<kMont>(sorted_image(g, blockIdx.y), g.n, outs.p[blockIdx.y]);
}

// Lookup j = blockIdx.y reads A' = the sorted image of column j and T = that of column table_col[j].
__global__ void __launch_bounds__(kNT) k_lpb_leaders(const LpGeom g) {
  const uint32_t j = blockIdx.y;
  lp_leaders(sorted_image(g, j), sorted_image(g, g.table_col[j]), g.n, g.repeat + j * g.flag_stride,
             g.used + j * g.flag_stride, g.heads + j);
}

__global__ void __launch_bounds__(kNT) k_lpb_totals(const LpGeom g) {
  const uint32_t j = blockIdx.y;
  lp_totals(g.repeat + j * g.flag_stride, g.used + j * g.flag_stride, g.n, g.totals + j * g.tot_stride);
}

__global__ void __launch_bounds__(kNT) k_lpb_carries(const LpGeom g) {
  const uint32_t j = blockIdx.y;
  lp_carries(g.totals + j * g.tot_stride, g.nb, g.carries + j * g.tot_stride, g.heads + j);
}

__global__ void __launch_bounds__(kNT) k_lpb_lists(const LpGeom g) {
  const uint32_t j = blockIdx.y;
  lp_lists(g.repeat + j * g.flag_stride, g.used + j * g.flag_stride, g.n, g.carries + j * g.tot_stride,
           g.rep_row + j * g.flag_stride, g.un_pos + j * g.flag_stride);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT) k_lpb_write(const LpOut outs, const LpGeom g) {
  const uint32_t j = blockIdx.y;
  lp_write<kMont>(sorted_image(g, j), sorted_image(g, g.table_col[j]), g.n, g.repeat + j * g.flag_stride,
                  g.rep_row + j * g.flag_stride, g.un_pos + j * g.flag_stride, g.heads + j, outs.p[j]);
}

constexpr size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

struct LpLayout {
  size_t state[2], counts, image[4], repeat, used, rep_row, un_pos, totals, carries, total;
};

LpLayout layout(size_t n, bool permute) {
  const size_t nb = (n + kLpTile - 1) / kLpTile;
  LpLayout l{};
  size_t at = align256(kLpHeadBytes);
  for (int s = 0; s < (permute ? 2 : 1); s++) l.state[s] = at, at += sizeof(LpState);
  l.counts = at, at += align256(256 * nb * sizeof(uint32_t));
  for (int k = 0; k < (permute ? 4 : 2); k++) l.image[k] = at, at += align256(n * sizeof(Fr));
  if (permute) {
    l.repeat = at, at += align256(n * sizeof(uint32_t));
    l.used = at, at += align256(n * sizeof(uint32_t));
    l.rep_row = at, at += align256(n * sizeof(uint32_t));
    l.un_pos = at, at += align256(n * sizeof(uint32_t));
    l.totals = at, at += align256(2 * nb * sizeof(uint32_t));
    l.carries = at, at += align256(2 * nb * sizeof(uint32_t));
  }
  l.total = at;
  return l;
}

// One column: d_in -> sorted canonical keys in img0 or img1 (state->final_image says which).
void enqueue_sort(const sv_fe* d_in, bool mont, uint32_t n, uint32_t nb, LpState* state, LpHead* head, uint4* img0,
                  uint4* img1, uint32_t* counts, hipStream_t st) {
  const uint4* in = reinterpret_cast<const uint4*>(d_in);
  const uint32_t first = std::min(nb, kFirstBlocksMax);
  if (mont) hipLaunchKernelGGL(k_lp_first<true>, dim3(first), dim3(kNT), 0, st, in, img0, n, nb, state, head);
  else hipLaunchKernelGGL(k_lp_first<false>, dim3(first), dim3(kNT), 0, st, in, img0, n, nb, state, head);
  hipLaunchKernelGGL(k_lp_plan, dim3(1), dim3(kNT), 0, st, state);
  for (uint32_t pass = 0; pass < kLpDigits; pass++) {
    hipLaunchKernelGGL(k_lp_count, dim3(nb), dim3(kNT), 0, st, state, pass, reinterpret_cast<const uint32_t*>(img0),
                       reinterpret_cast<const uint32_t*>(img1), n, counts);
    hipLaunchKernelGGL(k_lp_offsets, dim3(256), dim3(kNT), 0, st, state, pass, nb, counts);
    hipLaunchKernelGGL(k_lp_scatter, dim3(nb), dim3(kNT), 0, st, state, pass, img0, img1, n, counts);
  }
}

void enqueue_finish(bool mont, uint32_t n, const LpState* state, const uint4* img0, const uint4* img1, sv_fe* d_out,
                    hipStream_t st) {
  const uint32_t rows = (n + kNT - 1) / kNT;
  uint4* out = reinterpret_cast<uint4*>(d_out);
  if (mont) hipLaunchKernelGGL(k_lp_finish<true>, dim3(rows), dim3(kNT), 0, st, state, img0, img1, n, out);
  else hipLaunchKernelGGL(k_lp_finish<false>, dim3(rows), dim3(kNT), 0, st, state, img0, img1, n, out);
}

template <class T>
T* at(void* scratch, size_t offset) {
  return reinterpret_cast<T*>(static_cast<char*>(scratch) + offset);
}

}  // namespace

size_t lookup_permute_scratch_bytes(size_t n, bool permute) { return layout(n, permute).total; }

int lookup_permute_enqueue(const LpCall& call, void* d_scratch, hipStream_t st) {
  static_assert(sizeof(Fr) == sizeof(sv_fe), "Fr is the ABI's element");
  if (call.n == 0 || call.n > kLpMaxRows) {
    set_error("lookup permute: n = %zu out of range", call.n);
    return SV_ERR_LEN;
  }
  const bool mont = call.form == SV_MONTGOMERY;
  const uint32_t n = (uint32_t)call.n;
  const uint32_t nb = (n + kLpTile - 1) / kLpTile;
  const LpLayout l = layout(call.n, call.permute);
  char* scratch = static_cast<char*>(d_scratch);
  LpHead* head = reinterpret_cast<LpHead*>(scratch);
  LpState* sa = reinterpret_cast<LpState*>(scratch + l.state[0]);
  uint32_t* counts = reinterpret_cast<uint32_t*>(scratch + l.counts);
  uint4* img[4];
  for (int k = 0; k < 4; k++) img[k] = reinterpret_cast<uint4*>(scratch + l.image[k]);
  // the head and the histograms start at zero
  SV_HIP(hipMemsetAsync(scratch, 0, l.counts, st));
  enqueue_sort(call.d_in, mont, n, nb, sa, head, img[0], img[1], counts, st);
  enqueue_finish(mont, n, sa, img[0], img[1], call.d_out, st);
  if (call.permute) {
    LpState* ss = reinterpret_cast<LpState*>(scratch + l.state[1]);
    uint32_t* repeat = reinterpret_cast<uint32_t*>(scratch + l.repeat);
    uint32_t* used = reinterpret_cast<uint32_t*>(scratch + l.used);
    uint32_t* rep_row = reinterpret_cast<uint32_t*>(scratch + l.rep_row);
    uint32_t* un_pos = reinterpret_cast<uint32_t*>(scratch + l.un_pos);
    uint32_t* totals = reinterpret_cast<uint32_t*>(scratch + l.totals);
    uint32_t* carries = reinterpret_cast<uint32_t*>(scratch + l.carries);
    SV_HIP(hipMemsetAsync(used, 0, (size_t)n * sizeof(uint32_t), st));
    enqueue_sort(call.d_table, mont, n, nb, ss, head, img[2], img[3], counts, st);
    const LpImages im{sa, ss, img[0], img[1], img[2], img[3]};
    const uint32_t rows = (n + kNT - 1) / kNT;
    uint4* out = reinterpret_cast<uint4*>(call.d_out_table);
    hipLaunchKernelGGL(k_lp_leaders, dim3(rows), dim3(kNT), 0, st, im, n, repeat, used, head);
    hipLaunchKernelGGL(k_lp_totals, dim3(nb), dim3(kNT), 0, st, repeat, used, n, totals);
    hipLaunchKernelGGL(k_lp_carries, dim3(1), dim3(kNT), 0, st, totals, nb, carries, head);
    hipLaunchKernelGGL(k_lp_lists, dim3(nb), dim3(kNT), 0, st, repeat, used, n, carries, rep_row, un_pos);
    if (mont) hipLaunchKernelGGL(k_lp_write<true>, dim3(rows), dim3(kNT), 0, st, im, n, repeat, rep_row, un_pos, head, out);
    else hipLaunchKernelGGL(k_lp_write<false>, dim3(rows), dim3(kNT), 0, st, im, n, repeat, rep_row, un_pos, head, out);
  }
  SV_HIP(hipGetLastError());
  return SV_OK;
}

// Every column of the batch in one set of launches: 104 kernels (105 with tables the caller has
// sorted) and two memsets, whatever the number of lookups.
int lookup_permute_batch_enqueue(const LpBatchCall& call, void* d_scratch, hipStream_t st) {
  static_assert(sizeof(LpState) == kLpbStateBytes && kLpHeadBytes == kLpbHeadBytes && kLpTile == kLpbTile &&
                    kLpMaxRows == kLpbMaxRows && sizeof(sv_fe) == kLpbElem,
                "lp_batch_plan.hpp lays out this file's scratch");
  static_assert(kLpbMax == SV_LOOKUP_BATCH_MAX && kLpbTablesSorted == SV_LOOKUP_TABLES_SORTED &&
                    kLpbCanonical == SV_CANONICAL && kLpbMontgomery == SV_MONTGOMERY,
                "lp_batch_plan.hpp's numbers are the header's");
  const LpBatchPlan& p = *call.plan;
  if (p.rule != kLpbOk || p.count == 0 || p.count > kLpbMax || p.slots == 0 || p.slots > p.count || call.n == 0 ||
      call.n > kLpMaxRows) {
    set_error("lookup permute batch: not a plan of an accepted call");
    return SV_ERR_ARG;
  }
  const bool mont = call.form == SV_MONTGOMERY;
  const bool presorted = p.sorted_cols == p.count;
  LpGeom g{};
  g.n = (uint32_t)call.n;
  g.nb = (g.n + kLpTile - 1) / kLpTile;
  g.sorted_cols = p.sorted_cols;
  g.heads = at<LpHead>(d_scratch, p.heads);
  g.states = at<LpState>(d_scratch, p.states);
  g.counts = at<uint32_t>(d_scratch, p.counts);
  g.images = at<uint4>(d_scratch, p.images);
  g.repeat = at<uint32_t>(d_scratch, p.repeat);
  g.used = at<uint32_t>(d_scratch, p.used);
  g.rep_row = at<uint32_t>(d_scratch, p.rep_row);
  g.un_pos = at<uint32_t>(d_scratch, p.un_pos);
  g.totals = at<uint32_t>(d_scratch, p.totals);
  g.carries = at<uint32_t>(d_scratch, p.carries);
  g.image_stride = p.image_stride / sizeof(uint4);
  g.counts_stride = p.counts_stride / sizeof(uint32_t);
  g.flag_stride = p.flag_stride / sizeof(uint32_t);
  g.tot_stride = p.tot_stride / sizeof(uint32_t);
  LpIn ins{}, tabs{};
  LpOut out_a{}, out_s{};
  for (uint32_t j = 0; j < p.count; j++) {
    ins.p[j] = reinterpret_cast<const uint4*>(call.d_inputs[j]);
    out_a.p[j] = reinterpret_cast<uint4*>(call.d_out_inputs[j]);
    out_s.p[j] = reinterpret_cast<uint4*>(call.d_out_tables[j]);
    g.table_col[j] = (uint8_t)(p.count + p.slot[j]);
  }
  for (uint32_t s = 0; s < p.slots; s++) {
    tabs.p[s] = reinterpret_cast<const uint4*>(p.table[s]);
    if (!presorted) ins.p[p.count + s] = tabs.p[s];
  }
  const uint32_t cols = p.sorted_cols, lookups = p.count;
  const uint32_t first = std::min(g.nb, kFirstBlocksMax), rows = (g.n + kNT - 1) / kNT;
  // the heads and the histograms start at zero, and every lookup's used flags
  SV_HIP(hipMemsetAsync(d_scratch, 0, p.zeroed, st));
  SV_HIP(hipMemsetAsync(g.used, 0, p.count * p.flag_stride, st));
  if (presorted) {
    if (mont) hipLaunchKernelGGL(k_lpb_table<true>, dim3(first, p.slots), dim3(kNT), 0, st, tabs, g, p.count);
    else hipLaunchKernelGGL(k_lpb_table<false>, dim3(first, p.slots), dim3(kNT), 0, st, tabs, g, p.count);
  }
  if (mont) hipLaunchKernelGGL(k_lpb_first<true>, dim3(first, cols), dim3(kNT), 0, st, ins, g);
  else hipLaunchKernelGGL(k_lpb_first<false>, dim3(first, cols), dim3(kNT), 0, st, ins, g);
  hipLaunchKernelGGL(k_lpb_plan, dim3(1, cols), dim3(kNT), 0, st, g);
  for (uint32_t pass = 0; pass < kLpDigits; pass++) {
    hipLaunchKernelGGL(k_lpb_count, dim3(g.nb, cols), dim3(kNT), 0, st, g, pass);
    hipLaunchKernelGGL(k_lpb_offsets, dim3(256, cols), dim3(kNT), 0, st, g, pass);
    hipLaunchKernelGGL(k_lpb_scatter, dim3(g.nb, cols), dim3(kNT), 0, st, g, pass);
  }
  if (mont) hipLaunchKernelGGL(k_lpb_finish<true>, dim3(rows, lookups), dim3(kNT), 0, st, out_a, g);
  else hipLaunchKernelGGL(k_lpb_finish<false>, dim3(rows, lookups), dim3(kNT), 0, st, out_a, g);
  hipLaunchKernelGGL(k_lpb_leaders, dim3(rows, lookups), dim3(kNT), 0, st, g);
  hipLaunchKernelGGL(k_lpb_totals, dim3(g.nb, lookups), dim3(kNT), 0, st, g);
  hipLaunchKernelGGL(k_lpb_carries, dim3(1, lookups), dim3(kNT), 0, st, g);
  hipLaunchKernelGGL(k_lpb_lists, dim3(g.nb, lookups), dim3(kNT), 0, st, g);
  if (mont) hipLaunchKernelGGL(k_lpb_write<true>, dim3(rows, lookups), dim3(kNT), 0, st, out_s, g);
  else hipLaunchKernelGGL(k_lpb_write<false>, dim3(rows, lookups), dim3(kNT), 0, st, out_s, g);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

}  // namespace sv
