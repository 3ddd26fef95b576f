// NTT over BN254 Fr for data that is already in HBM: out[j] = sum_i in[i] (g omega^j)^i (forward),
// its exact inverse, natural order on both sides, `count` transforms back to back.
//
// Decomposition (ntt_plan.hpp has the algebra and every index map): the k index bits are cut into
// ceil(k / T) digits, one launch per digit, decimation in frequency from the top digit down.  A pass
// runs the 2^w-point DFT of its digit for every column and multiplies frequency f by the twiddle
// omega_n^(f 2^H lo) on the way out.  No block waits for another block: the passes are separate
// launches in stream order.  Passes before the last write where they read; the last one (contiguous
// rows) stores digit-reversed, so the result is in natural order.  With one pass the data goes
// d_in -> d_out directly; with more, every pass but the last writes an image in pooled scratch and
// every pass but the first reads it: the input is only read, and in place costs nothing extra.
//
// A block (512 threads) holds 2^11 elements in LDS (64 KiB, two blocks per CU): the 2^w entries of
// C = 2^(11 - w) NEIGHBOURING columns (at most 128), element x = entry x / C of column x % C.  The
// strided side of every pass has its columns at consecutive addresses, so the block's global loads
// and stores are 16 B per lane along runs of C x 32 B (256 B at w = 8, 64 B at w = 10); a pass reads
// each element once and writes it once.  In LDS an element is split into its two 16-B halves, one
// plane each (the second plane 128 B off the bank phase of the first): consecutive threads read
// consecutive 16-B slots of a plane, which is conflict-free for ds_read_b128 whatever the lane
// grouping, and the global staging, whose lanes alternate between the planes, hits all 64 banks.
// Between barriers every thread runs two radix-2 butterflies of one stage (Gentleman-Sande: sum,
// and difference times omega_{2d}^j); the w stages leave frequency f at entry bitrev(f), which the
// way out undoes through registers.
//
// Roots: two tables per direction and device, hi[e >> 13] and lo[e & 8191] of the root of order
// 2^26 (omega_26^e = hi lo; 4 x 8192 x 32 B = 1 MiB per device, whatever k), built on the host at a
// device's first call under a lock and kept.  A smaller domain's omega_k^e is omega_26^(e 2^(26-k));
// a stage's omega_{2d}^j has a multiple of 2^13 as exponent and is one entry of hi.  The coset
// factors (g^i on the first load, g^-i / n on the last store) and the form conversions are folded
// into one per-element factor on either side: a constant (Montgomery conversion, 1 / n) or the
// constant times a power of g, which a thread builds from the host's seed powers g^(2^b) (in the
// kernel arguments) for its first element and steps by one more seed for the next.
//
// An element not below r is found in the first pass; a block's flag is a plain store and one small
// launch folds the flags: nothing is zeroed per call.
//
// The extended-domain round trip (ext_plan.hpp has its predicates) runs the same passes.  k_ntt_pass
// is a template over the mode; kNtt is the transform above and compiles to what it was.
//   kLde   pass 0 of a coset LDE: n = 2^k coefficients into the plan of K = k + e.  An input index
//          >= n is a zero that is never loaded (no padded copy exists in HBM), the way-in factor
//          goes to live elements only, a block whose columns are all padding stores zeros and
//          leaves, and in the first min(e, w_0) stages the upper partner of a butterfly is a known
//          zero: sum = p stays where it is, difference = p omega^j, and a pair whose lower partner
//          is padding too is skipped.  Passes 1 .. are kNtt.
//   kQuot  the first and the last pass of the quotient's inverse coset transform: the way-in factor
//          is table[i mod 2^e] = c / t(g omega_K^i) (c the conversion constant, folded in on the
//          host; at most 256 entries at the head of the call's scratch), and the digit-reversed
//          store of the last pass skips every destination index >= pieces n.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "field.hpp"
#include "ext_plan.hpp"
#include "ntt.hpp"
#include "runtime.hpp"

namespace sv {

namespace {

constexpr uint32_t kTL = kNttThreadsLog;
constexpr uint32_t kNT = 1u << kTL;               // threads per block
constexpr uint32_t kElems = 1u << kNttBlockLog;   // elements in the block's image
constexpr uint32_t kPer = kElems / kNT;           // elements per thread
static_assert(kNttBlockColsMaxLog < kTL && kPer >= 2, "a thread's 16-B units all lie in one column");
constexpr uint32_t kPlane = kElems + 8;           // uint4 between the planes: 128 B off phase
constexpr uint32_t kRootLog = 26;                 // the tables' root
constexpr uint32_t kTabLog = 13;                  // entries per table (log2)
constexpr uint32_t kTabMask = (1u << kTabLog) - 1u;
static_assert(kNttMaxLog <= kRootLog && kRootLog == 2 * kTabLog, "omega_26^e = hi[e >> 13] lo[e & 8191]");

enum : int { kNone = 0, kConst = 1, kPowers = 2, kTable = 3 };  // the per-element factor of a side
enum : int { kNtt = 0, kLde = 1, kQuot = 2 };                        // k_ntt_pass's modes

struct PassArgs {
  const uint4* src;
  uint4* dst;
  const Fr* tab_hi;      // the direction's tables
  const Fr* tab_lo;
  uint32_t* flags;       // per-block flags; the first pass only, else NULL
  uint64_t total_cols;   // count << (k - w)
  NttPlan plan;
  uint32_t pass;
  int in_mode, out_mode;
  Fr in_c, out_c;        // the constant of either side
  Fr pw[kNttMaxLog];     // g^(2^b) (forward) or g^-(2^b) (inverse), Montgomery
  // kLde, kQuot only
  uint32_t live_log;     // kLde: input indices below 2^live_log are coefficients, the rest zeros
  uint32_t ext_log;      // e
  uint64_t keep;         // kQuot: destination indices below it are stored
  const Fr* table;       // kQuot: c / t_i, 2^e entries
};

__device__ __forceinline__ Fr ld_el(const uint4* sm, uint32_t x) {
  const uint4 a = sm[x], b = sm[kPlane + x];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_el(uint4* sm, uint32_t x, const Fr& v) {
  sm[x] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  sm[kPlane + x] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

// c g^e from the seeds g^(2^b), b < k
__device__ __forceinline__ Fr pow_seeds(const Fr& c, const Fr (&pw)[kNttMaxLog], uint32_t e, uint32_t k) {
  Fr r = c;
  for (uint32_t b = 0; b < k; b++)
    if ((e >> b) & 1u) r = r * pw[b];
  return r;
}

template <int kMode>
__global__ void __launch_bounds__(kNT) k_ntt_pass(const PassArgs a) {
  __shared__ uint4 sm[kPlane + kElems];
  const uint32_t t = threadIdx.x;
  const uint32_t s = a.pass, k = a.plan.k;
  const uint32_t w = ntt_width(a.plan, s);
  const uint32_t c = ntt_block_cols_log(a.plan, s);
  const uint32_t cl = ntt_cols_log(a.plan, s);
  const uint32_t elems = 1u << (w + c);
  const uint32_t sl = ntt_src_stride_log(a.plan, s), dl = ntt_dst_stride_log(a.plan, s);
  const uint32_t cmask = (1u << c) - 1u;
  const uint64_t g0 = (uint64_t)blockIdx.x << c;  // the block's first column, counted over the batch

  // the column of this thread's 16-B units (staging) ...
  const uint32_t half = t & 1u;
  const uint32_t qu = (t >> 1) & cmask;
  const uint64_t gu = g0 + qu;
  const bool live_u = gu < a.total_cols;
  const uint32_t col_u = (uint32_t)(gu & ((1ull << cl) - 1ull));
  const uint64_t first_u = (gu >> cl) << k;  // its transform's first element
  // kLde reads polynomial gu >> cl of 2^live_log coefficients
  const uint64_t src_first_u = kMode == kLde ? (gu >> cl) << a.live_log : first_u;
  const uint32_t mu0 = t >> (c + 1), mu_step = kNT >> (c + 1);
  // ... and of its whole elements (arithmetic)
  const uint32_t qe = t & cmask;
  const uint32_t col_e = (uint32_t)((g0 + qe) & ((1ull << cl) - 1ull));
  const uint32_t m0 = t >> c, m_step = kNT >> c;

  if (kMode == kLde) {
    // a block of padding: zeros in the image, a clean flag
    if (__syncthreads_and(ext_col_dead(a.plan, col_e, a.live_log))) {
      if (live_u) {
        const uint64_t base = first_u + ntt_dst_base(a.plan, s, col_u);
#pragma unroll
        for (uint32_t r = 0; r < 2 * kPer; r++) {
          const uint32_t m = mu0 + r * mu_step;
          if (t + r * kNT < 2 * elems) a.dst[2 * (base + ((uint64_t)m << dl)) + half] = make_uint4(0, 0, 0, 0);
        }
      }
      if (t == 0) a.flags[blockIdx.x] = 0u;
      return;
    }
  }

  {
    const uint32_t sb = ntt_src_base(a.plan, s, col_u);
    const uint64_t base = src_first_u + sb;
    uint4 v[2 * kPer];
#pragma unroll
    for (uint32_t r = 0; r < 2 * kPer; r++) {
      const uint32_t m = mu0 + r * mu_step;
      bool ld = live_u && t + r * kNT < 2 * elems;
      if (kMode == kLde) ld = ld && ext_live(sb + (m << sl), a.live_log);
      v[r] = ld ? a.src[2 * (base + ((uint64_t)m << sl)) + half] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (uint32_t r = 0; r < 2 * kPer; r++) {
      const uint32_t m = mu0 + r * mu_step;
      if (t + r * kNT < 2 * elems) sm[half * kPlane + ((m << c) | qu)] = v[r];
    }
  }
  __syncthreads();

  // first pass: the check, and the factor of the way in (conversion, g^i)
  if (a.flags != nullptr) {
    bool bad = false;
    Fr f = a.in_c;
    const uint32_t i0 = ntt_src_base(a.plan, s, col_e) + (m0 << sl);
    // kLde: a thread's live elements are a prefix of its elements (the index grows with r)
    if (a.in_mode == kPowers && (kMode != kLde || ext_live(i0, a.live_log))) f = pow_seeds(a.in_c, a.pw, i0, k);
    const bool per_element = kMode == kQuot && !ext_table_shared(a.plan, a.ext_log);
    if (kMode == kQuot && a.in_mode == kTable) f = a.table[ext_table_index(a.plan, col_e, m0, a.ext_log)];
    const uint32_t step = sl + kTL - c;  // g^(m_step 2^sl): at most k - 2 (the index below is clamped all the same)
    const Fr fstep = a.pw[step < kNttMaxLog ? step : kNttMaxLog - 1];
#pragma unroll 1
    for (uint32_t r = 0; r < kPer; r++) {
      const uint32_t x = t + r * kNT;
      if (x < elems && (kMode != kLde || ext_live(i0 + ((r * m_step) << sl), a.live_log))) {
        Fr v = ld_el(sm, x);
        bad |= !v.is_reduced();
        if (a.in_mode != kNone) {
          if (per_element && r > 0) f = a.table[ext_table_index(a.plan, col_e, m0 + r * m_step, a.ext_log)];
          st_el(sm, x, v * f);
          if (a.in_mode == kPowers) f = f * fstep;
        }
      }
    }
    const int any_bad = __syncthreads_or(bad);  // also: the converted elements are visible
    if (t == 0) a.flags[blockIdx.x] = any_bad ? 1u : 0u;
  }

  // the w stages, kPer / 2 butterflies per thread between barriers
  const uint32_t zero_stages = kMode == kLde ? ext_zero_stages(a.plan, a.ext_log) : 0u;
  for (int st = (int)w - 1; st >= 0; st--) {
    Fr lo_v[kPer / 2], hi_v[kPer / 2];
#pragma unroll
    for (uint32_t r = 0; r < kPer / 2; r++) {
      const uint32_t b = t + r * kNT;
      if (b < elems / 2) {
        uint32_t m, j;
        ntt_stage_pair(b >> c, (uint32_t)st, &m, &j);
        const uint32_t x0 = (m << c) | (b & cmask), x1 = x0 + (1u << (st + c));
        if (kMode == kLde && (uint32_t)st + zero_stages >= w) {  // q = 0: the sum is p, in place
          if (ext_pair_dead(a.plan, a.ext_log, (uint32_t)st, m)) continue;  // p = 0 too: x1 stays zero
          hi_v[r] = ld_el(sm, x0);
          if (st > 0) hi_v[r] = hi_v[r] * a.tab_hi[ntt_stage_exp(j, (uint32_t)st, kRootLog) >> kTabLog];
          st_el(sm, x1, hi_v[r]);
          continue;
        }
        const Fr p = ld_el(sm, x0), q = ld_el(sm, x1);
        lo_v[r] = p + q;
        hi_v[r] = p - q;
        if (st > 0) hi_v[r] = hi_v[r] * a.tab_hi[ntt_stage_exp(j, (uint32_t)st, kRootLog) >> kTabLog];
        st_el(sm, x0, lo_v[r]);
        st_el(sm, x1, hi_v[r]);
      }
    }
    __syncthreads();
  }

  // the way out: frequency f from entry bitrev(f), the twiddle, the factor (conversion, 1 / n, g^-j)
  {
    const bool tw = !ntt_is_last(a.plan, s);
    Fr f = a.out_c;
    if (a.out_mode == kPowers) f = pow_seeds(a.out_c, a.pw, ntt_dst_base(a.plan, s, col_e) + (m0 << dl), k);
    const uint32_t step = dl + kTL - c;
    const Fr fstep = a.pw[step < kNttMaxLog ? step : kNttMaxLog - 1];
    Fr vals[kPer];
#pragma unroll
    for (uint32_t r = 0; r < kPer; r++) {
      const uint32_t x = t + r * kNT, fr = m0 + r * m_step;
      if (x < elems) {
        Fr v = ld_el(sm, (ntt_bitrev(fr, w) << c) | qe);
        if (tw) {
          const uint32_t e = ntt_root_exp(a.plan, ntt_twiddle_exp(a.plan, s, col_e, fr), kRootLog);
          Fr z = a.tab_hi[e >> kTabLog];
          if (k > kTabLog) z = z * a.tab_lo[e & kTabMask];
          v = v * z;
        }
        if (a.out_mode != kNone) {
          v = v * f;
          if (a.out_mode == kPowers) f = f * fstep;
        }
        vals[r] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kPer; r++) {
      const uint32_t x = t + r * kNT;
      if (x < elems) st_el(sm, x, vals[r]);
    }
    __syncthreads();
  }

  if (live_u) {
    const uint32_t db = ntt_dst_base(a.plan, s, col_u);
    const uint64_t base = first_u + db;
    const bool cut = kMode == kQuot && ntt_is_last(a.plan, s);
#pragma unroll
    for (uint32_t r = 0; r < 2 * kPer; r++) {
      const uint32_t m = mu0 + r * mu_step;
      if (t + r * kNT < 2 * elems && (!cut || ext_kept(db + (m << dl), a.keep)))
        a.dst[2 * (base + ((uint64_t)m << dl)) + half] = sm[half * kPlane + ((m << c) | qu)];
    }
  }
}

__global__ void __launch_bounds__(kNT) k_ntt_flags(const uint32_t* __restrict__ flags, uint32_t nb,
                                                    uint32_t* __restrict__ err) {
  uint32_t bad = 0;
  for (uint32_t i = threadIdx.x; i < nb; i += kNT) bad |= flags[i];
  const int any_bad = __syncthreads_or((int)bad);
  if (threadIdx.x == 0) *err = any_bad ? 1u : 0u;
}

// halo2curves' Fr::ROOT_OF_UNITY = 7^((r - 1) / 2^28), canonical
Fr root28() {
  Fr x;
  const uint32_t c[8] = {0x60c37c9cu, 0xd34f1ed9u, 0xd39329c8u, 0x3215cf6du,
                         0x3dd31f74u, 0x98865ea9u, 0x166d18b7u, 0x03ddb9f5u};
  for (int i = 0; i < 8; i++) x.v[i] = c[i];
  return fe_to_mont(x);
}
Fr root_mont(uint32_t log_n) {
  Fr x = root28();
  for (uint32_t i = log_n; i < 28; i++) x = fe_sqr(x);
  return x;
}

// the per-device tables: [forward hi | forward lo | inverse hi | inverse lo], 2^13 entries each
std::mutex g_tab_mu;
std::unordered_map<int, Fr*> g_tabs;

int tables_for(int device, hipStream_t st, const Fr** out) {
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto it = g_tabs.find(device);
  if (it != g_tabs.end()) {
    *out = it->second;
    return SV_OK;
  }
  const size_t n = size_t(1) << kTabLog;
  std::vector<Fr> h(4 * n);
  const Fr w = root_mont(kRootLog);
  const Fr roots[2] = {w, fe_inv(w)};
  for (int d = 0; d < 2; d++) {
    Fr* hi = h.data() + (2 * d) * n;
    Fr* lo = hi + n;
    lo[0] = Fr::one();
    for (size_t i = 1; i < n; i++) lo[i] = lo[i - 1] * roots[d];
    const Fr big = lo[n - 1] * roots[d];  // the root to the 2^13
    hi[0] = Fr::one();
    for (size_t i = 1; i < n; i++) hi[i] = hi[i - 1] * big;
  }
  Fr* dptr = nullptr;
  SV_HIP(hipMalloc(&dptr, h.size() * sizeof(Fr)));
  hipError_t e = hipMemcpyAsync(dptr, h.data(), h.size() * sizeof(Fr), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // h goes out of scope
  if (e != hipSuccess) {
    (void)hipFree(dptr);
    set_error("NTT root tables: %s", hipGetErrorString(e));
    return SV_ERR_DEVICE;
  }
  g_tabs[device] = dptr;
  *out = dptr;
  return SV_OK;
}

Fr fr_in(const sv_fe& a) {
  Fr x;
  memcpy(x.v, a.l, sizeof x.v);
  return x;
}

uint32_t pass_blocks(const NttPlan& plan, uint32_t s, size_t count) {
  const uint64_t cols = (uint64_t)count << ntt_cols_log(plan, s);
  const uint32_t c = ntt_block_cols_log(plan, s);
  return (uint32_t)((cols + (1ull << c) - 1) >> c);
}
size_t flags_bytes(const NttPlan& plan, size_t count) {
  return (pass_blocks(plan, 0, count) * sizeof(uint32_t) + 255) & ~size_t(255);
}

}  // namespace

int fr_root_of_unity(uint32_t log_n, int form, sv_fe* out) {
  if (log_n > 28) {
    set_error("root_of_unity: log_n = %u exceeds the field's two-adicity 28", log_n);
    return SV_ERR_ARG;
  }
  Fr x = root_mont(log_n);
  if (form != SV_MONTGOMERY) x = fe_from_mont(x);
  memcpy(out->l, x.v, sizeof x.v);
  return SV_OK;
}

size_t ntt_scratch_bytes(uint32_t log_n, size_t count, uint32_t tile_log) {
  const NttPlan plan = ntt_make_plan(log_n, tile_log);
  const size_t image = plan.passes > 1 ? (count << log_n) * sizeof(Fr) : 0;
  return kNttHeadBytes + flags_bytes(plan, count) + image;
}

int ntt_enqueue(const NttCall& call, int device, void* d_scratch, hipStream_t st) {
  static_assert(sizeof(Fr) == sizeof(sv_fe), "Fr is the ABI's element");
  const uint32_t k = call.log_n;
  const NttPlan plan = ntt_make_plan(k, call.tile_log);
  const uint32_t launches = ntt_launches(plan);
  const Fr* tabs;
  SV_TRY(tables_for(device, st, &tabs));
  const size_t tn = size_t(1) << kTabLog;

  char* scratch = static_cast<char*>(d_scratch);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kNttErrOffset);
  uint32_t* flags = reinterpret_cast<uint32_t*>(scratch + kNttHeadBytes);
  uint4* image = reinterpret_cast<uint4*>(scratch + kNttHeadBytes + flags_bytes(plan, call.count));

  const bool mont = call.form == SV_MONTGOMERY;
  PassArgs a;
  memset(&a, 0, sizeof a);
  a.tab_hi = tabs + (call.inverse ? 2 * tn : 0);
  a.tab_lo = a.tab_hi + tn;
  a.plan = plan;
  // the seeds: g^(2^b), or g^-(2^b) for the inverse
  Fr g = Fr::one();
  if (call.has_shift) {
    g = fr_in(call.shift);
    if (!mont) g = fe_to_mont(g);
    if (call.inverse) g = fe_inv(g);
  }
  for (uint32_t b = 0; b < kNttMaxLog; b++) {
    a.pw[b] = g;
    g = fe_sqr(g);
  }
  // a side's constant: x * c is a Montgomery product, so a raw R^2 converts a canonical element on
  // the way in and a raw 1 (or the canonical 1 / n) converts on the way out
  Fr raw_one = Fr::zero();
  raw_one.v[0] = 1;
  int in_mode = mont ? kNone : kConst;
  Fr in_c = mont ? Fr::one() : fe_to_mont(Fr::one());  // R, or R^2
  int out_mode = mont ? kNone : kConst;
  Fr out_c = mont ? Fr::one() : raw_one;
  if (call.inverse) {
    Fr n = Fr::one();
    for (uint32_t i = 0; i < k; i++) n = n + n;
    const Fr ninv = fe_inv(n);
    out_c = mont ? ninv : fe_from_mont(ninv);
    out_mode = call.has_shift ? kPowers : kConst;
  } else if (call.has_shift) {
    in_mode = kPowers;
  }

  for (uint32_t s = 0; s < launches; s++) {
    const bool first = s == 0, last = s + 1 == launches;
    a.src = first ? static_cast<const uint4*>(call.d_in) : image;
    a.dst = last ? static_cast<uint4*>(call.d_out) : image;
    a.flags = first ? flags : nullptr;
    a.total_cols = (uint64_t)call.count << ntt_cols_log(plan, s);
    a.pass = s;
    a.in_mode = first ? in_mode : kNone;
    a.in_c = in_c;
    a.out_mode = last ? out_mode : kNone;
    a.out_c = out_c;
    hipLaunchKernelGGL(k_ntt_pass<kNtt>, dim3(pass_blocks(plan, s, call.count)), dim3(kNT), 0, st, a);
  }
  hipLaunchKernelGGL(k_ntt_flags, dim3(1), dim3(kNT), 0, st, flags, pass_blocks(plan, 0, call.count), err);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

// ---- the extended-domain round trip: coset LDE in, quotient coefficients out ----
namespace {

// what both calls share with ntt_enqueue: the tables of a direction, the plan, the seeds of g
int ext_args(PassArgs* a, uint32_t K, uint32_t tile_log, bool inverse, Fr g, int device, hipStream_t st) {
  const Fr* tabs;
  SV_TRY(tables_for(device, st, &tabs));
  const size_t tn = size_t(1) << kTabLog;
  memset(a, 0, sizeof *a);
  a->tab_hi = tabs + (inverse ? 2 * tn : 0);
  a->tab_lo = a->tab_hi + tn;
  a->plan = ntt_make_plan(K, tile_log);
  for (uint32_t b = 0; b < kNttMaxLog; b++) {
    a->pw[b] = g;
    g = fe_sqr(g);
  }
  return SV_OK;
}

size_t ext_table_bytes(uint32_t log_ext) { return ((sizeof(Fr) << log_ext) + 255) & ~size_t(255); }

}  // namespace

size_t lde_scratch_bytes(uint32_t log_n, uint32_t log_ext, size_t count, uint32_t tile_log) {
  return ntt_scratch_bytes(log_n + log_ext, count, tile_log);
}

int lde_enqueue(const LdeCall& call, int device, void* d_scratch, hipStream_t st) {
  const uint32_t K = call.log_n + call.log_ext;
  const bool mont = call.form == SV_MONTGOMERY;
  Fr g = Fr::one();
  if (call.has_shift) {
    g = fr_in(call.shift);
    if (!mont) g = fe_to_mont(g);
  }
  PassArgs a;
  SV_TRY(ext_args(&a, K, call.tile_log, false, g, device, st));
  const NttPlan& plan = a.plan;
  const uint32_t launches = ntt_launches(plan);

  char* scratch = static_cast<char*>(d_scratch);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kNttErrOffset);
  uint32_t* flags = reinterpret_cast<uint32_t*>(scratch + kNttHeadBytes);
  uint4* image = reinterpret_cast<uint4*>(scratch + kNttHeadBytes + flags_bytes(plan, call.count));

  Fr raw_one = Fr::zero();
  raw_one.v[0] = 1;
  a.in_c = mont ? Fr::one() : fe_to_mont(Fr::one());  // R, or R^2
  a.out_c = mont ? Fr::one() : raw_one;
  a.live_log = call.log_n;
  a.ext_log = call.log_ext;
  for (uint32_t s = 0; s < launches; s++) {
    const bool first = s == 0, last = s + 1 == launches;
    a.src = first ? static_cast<const uint4*>(call.d_coeffs) : image;
    a.dst = last ? static_cast<uint4*>(call.d_evals) : image;
    a.flags = first ? flags : nullptr;
    a.total_cols = (uint64_t)call.count << ntt_cols_log(plan, s);
    a.pass = s;
    a.in_mode = !first ? kNone : call.has_shift ? kPowers : mont ? kNone : kConst;
    a.out_mode = last && !mont ? kConst : kNone;
    const dim3 grid(pass_blocks(plan, s, call.count));
    if (first) hipLaunchKernelGGL(k_ntt_pass<kLde>, grid, dim3(kNT), 0, st, a);
    else hipLaunchKernelGGL(k_ntt_pass<kNtt>, grid, dim3(kNT), 0, st, a);
  }
  hipLaunchKernelGGL(k_ntt_flags, dim3(1), dim3(kNT), 0, st, flags, pass_blocks(plan, 0, call.count), err);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

size_t quotient_scratch_bytes(uint32_t log_n, uint32_t log_ext, uint32_t tile_log) {
  return ext_table_bytes(log_ext) + ntt_scratch_bytes(log_n + log_ext, 1, tile_log);
}
size_t quotient_stage_bytes(uint32_t log_ext) { return ext_table_bytes(log_ext); }

bool coset_meets_domain(const sv_fe& shift, int form, uint32_t log_size) {
  Fr g = fr_in(shift);
  if (form != SV_MONTGOMERY) g = fe_to_mont(g);
  for (uint32_t i = 0; i < log_size; i++) g = fe_sqr(g);
  return memcmp(g.v, Fr::one().v, sizeof g.v) == 0;
}

int quotient_enqueue(const QuotCall& call, int device, void* d_scratch, void* h_stage, hipStream_t st) {
  const uint32_t k = call.log_n, e = call.log_ext, K = k + e;
  const bool mont = call.form == SV_MONTGOMERY;
  Fr g = fr_in(call.shift);
  if (!mont) g = fe_to_mont(g);
  PassArgs a;
  SV_TRY(ext_args(&a, K, call.tile_log, true, fe_inv(g), device, st));
  const NttPlan& plan = a.plan;
  const uint32_t launches = ntt_launches(plan);

  // table[i] = c / (g^n omega_e^i - 1), i < 2^e: one inversion (no t_i is zero: g^(2^K) != 1)
  const size_t m = size_t(1) << e;
  Fr gn = g;
  for (uint32_t i = 0; i < k; i++) gn = fe_sqr(gn);
  const Fr we = root_mont(e);
  std::vector<Fr> t(m), pre(m);
  Fr x = gn, acc = Fr::one();
  for (size_t i = 0; i < m; i++) {
    t[i] = x - Fr::one();
    pre[i] = acc;
    acc = acc * t[i];
    x = x * we;
  }
  Fr inv = fe_inv(acc);
  Fr* stage = static_cast<Fr*>(h_stage);
  for (size_t i = m; i-- > 0;) {
    const Fr ti = inv * pre[i];
    inv = inv * t[i];
    stage[i] = mont ? ti : fe_to_mont(ti);  // canonical data: the table carries the R^2 of the conversion
  }

  char* scratch = static_cast<char*>(d_scratch);
  const size_t tb = ext_table_bytes(e);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kNttErrOffset);
  Fr* table = reinterpret_cast<Fr*>(scratch + kNttHeadBytes);
  uint32_t* flags = reinterpret_cast<uint32_t*>(scratch + kNttHeadBytes + tb);
  uint4* image = reinterpret_cast<uint4*>(scratch + kNttHeadBytes + tb + flags_bytes(plan, 1));
  SV_HIP(hipMemcpyAsync(table, stage, m * sizeof(Fr), hipMemcpyHostToDevice, st));

  Fr n = Fr::one();
  for (uint32_t i = 0; i < K; i++) n = n + n;
  const Fr ninv = fe_inv(n);
  a.in_c = Fr::one();
  a.out_c = mont ? ninv : fe_from_mont(ninv);
  a.ext_log = e;
  a.keep = (uint64_t)call.pieces << k;
  a.table = table;
  for (uint32_t s = 0; s < launches; s++) {
    const bool first = s == 0, last = s + 1 == launches;
    a.src = first ? static_cast<const uint4*>(call.d_numer) : image;
    a.dst = last ? static_cast<uint4*>(call.d_out) : image;
    a.flags = first ? flags : nullptr;
    a.total_cols = 1ull << ntt_cols_log(plan, s);
    a.pass = s;
    a.in_mode = first ? kTable : kNone;
    a.out_mode = last ? kPowers : kNone;
    const dim3 grid(pass_blocks(plan, s, 1));
    if (first || last) hipLaunchKernelGGL(k_ntt_pass<kQuot>, grid, dim3(kNT), 0, st, a);
    else hipLaunchKernelGGL(k_ntt_pass<kNtt>, grid, dim3(kNT), 0, st, a);
  }
  hipLaunchKernelGGL(k_ntt_flags, dim3(1), dim3(kNT), 0, st, flags, pass_blocks(plan, 0, 1), err);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

}  // namespace sv
