// Test-only device harness for the Fq12 lane operations of csrc/decider.hip, one operation per launch
// (tests/test_gpu_decider_ops.py checks them against Python big integers):
//   dc_wg        the workgroup kernel's slot operations (namespace wg: w_mul, w_sqr, w_frob, w_conj,
//                w_norm_inv) on one 512-thread block per case, operands staged in LDS slots as
//                k_decide_wg stages them, the RAW [0, 2p) destination slot copied out
//   dc_norm24    norm24 + lz_reduce on signed 24-bit limb sums, or lz_reduce alone on 9 words
//   dc_lanes     the single-wave kernel's group operations (g_mul, g_msq, g_mline, g_mul_lds, g_frob,
//                g_conj, g_inv, g_pow_x) with Grp set up as k_decide_lanes<S> does, S = 4 or 8; at
//                S = 4 the two groups of a wave carry different cases
//   dc_prologue  conv6 per lane, and merge_products / merge_products_wide on one D
// Values are 8 x u32 little-endian limbs in Montgomery form; an Fq12 operand is 6 Fq2 in the
// w-basis of fq12_lanes.hpp.  Grid and block sizes are fixed per operation and every index comes
// from the validated arguments: nothing is addressed by data.  Every entry point returns 0, or the
// hipError_t (hipErrorInvalidValue for a malformed call).  Not part of libsvgpu.
#include "../../snark-verifier-axiom_amd/csrc/decider.hip"

#include <cstdint>

using namespace sv;

namespace {

enum { WG_MUL = 0, WG_SQR = 1, WG_FROB = 2, WG_CONJ = 3, WG_NORM_INV = 4, WG_OPS };
enum { N24_NORM = 0, N24_REDUCE = 1, N24_OPS };
enum { LN_MUL = 0, LN_MSQ, LN_MLINE, LN_MUL_LDS, LN_FROB1, LN_FROB2, LN_FROB3, LN_CONJ, LN_INV, LN_POW_X, LN_OPS };
enum { PR_CONV6 = 0, PR_MERGE = 1, PR_MERGE_WIDE = 2, PR_OPS };

constexpr int kFq12Words = 6 * 16;  // 6 Fq2 of 2 x 8 words
constexpr size_t kMaxCases = 1u << 16;

__global__ void __launch_bounds__(wg::kThreads) k_dc_wg(int op, int imm, const uint32_t* __restrict__ a,
                                                        const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  using namespace wg;
  __shared__ __attribute__((aligned(32))) Fq2 S[3 * 6];  // slots: operand a, operand b, destination
  __shared__ __attribute__((aligned(32))) Fq gam[kLdsGamma / sizeof(Fq)];
  __shared__ Fq2 tj[3], di;
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * kFq12Words;
  uint32_t* sw = reinterpret_cast<uint32_t*>(S);
  for (int i = t; i < kFq12Words; i += kThreads) {
    sw[i] = a[base + i];
    sw[kFq12Words + i] = b[base + i];
    sw[2 * kFq12Words + i] = 0;
  }
  for (int i = t; i < (int)(kLdsGamma / 4); i += kThreads) reinterpret_cast<uint32_t*>(gam)[i] = c_gamma[i];
  __syncthreads();
  const WLane L = wlane_init();
  Fq2* dst = S + 12;
  switch (op) {  // block-uniform; every operation ends with its own barrier
    case WG_MUL: w_mul(L, dst, S, S + 6, imm); break;
    case WG_SQR: w_sqr(L, dst, S); break;
    case WG_FROB: w_frob(L, dst, S, imm, gam); break;
    case WG_CONJ: w_conj(dst, S, imm != 0); break;
    default: w_norm_inv(dst, S, tj, &di); break;
  }
  for (int i = t; i < kFq12Words; i += kThreads) out[base + i] = sw[2 * kFq12Words + i];
}

__global__ void __launch_bounds__(64) k_dc_norm24(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                  uint32_t n) {
  using namespace wg;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Lz v;
  if (op == N24_NORM) {
    uint32_t s[kL24];
#pragma unroll
    for (int j = 0; j < kL24; j++) s[j] = in[(size_t)kL24 * i + j];
    v = norm24(s);
  } else {
#pragma unroll
    for (int j = 0; j < 9; j++) v.v[j] = in[(size_t)9 * i + j];
  }
  const Fq r = lz_reduce(v);
#pragma unroll
  for (int j = 0; j < 8; j++) out[(size_t)8 * i + j] = r.v[j];
}

// the group set-up of k_decide_lanes<S>; case = blockIdx.x * NGRP + grp (whole blocks only)
template <int S>
__global__ void __launch_bounds__(64) k_dc_lanes(int op, const Fq2* __restrict__ a, const Fq2* __restrict__ b,
                                                 const Fq2* __restrict__ l, Fq2* __restrict__ out) {
  constexpr int GL = 8 * S;
  constexpr int NGRP = 64 / GL;
  __shared__ Fq2 sh[2 * NGRP * 6];
  __shared__ Fq2 tabk[NGRP][(kTab + kKeep) * 6];
  const int lane = threadIdx.x, grp = lane / GL, gl = lane % GL;
  const bool active = gl < 6 * S;
  const int k = active ? gl / S : 5, sub = active ? gl % S : 0;
  const size_t cs = (size_t)blockIdx.x * NGRP + grp;
  Grp G{sh + grp * 12, sh + grp * 12 + 6, tabk[grp], tabk[grp] + kTab * 6, k, sub, active && sub == 0, {}, {}};
  G.sqh = (S == 8 && active) ? c_sqr[k][sub >> 1] : SqrTerm{-1, -1, 0, 0};
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int slot = t * S + sub;
    G.sq[t] = slot < 4 ? c_sqr[k][slot] : SqrTerm{-1, -1, 0, 0};
  }
  const Fq2 x = a[cs * 6 + k], y = b[cs * 6 + k];
  const Fq2 l0 = l[cs * 3], l1 = l[cs * 3 + 1], l3 = l[cs * 3 + 2];
  Fq2 r = Fq2::zero();
  switch (op) {  // block-uniform
    case LN_MUL: r = g_mul<S>(G, x, y); break;
    case LN_MSQ: r = g_msq<S>(G, x); break;
    case LN_MLINE: r = g_mline<S>(G, x, l0, l1, l3); break;
    case LN_MUL_LDS:
      g_put(G, G.keep, 0, y);
      __syncthreads();
      r = g_mul_lds<S>(G, x, G.keep);
      break;
    case LN_FROB1: r = g_frob(G, 1, x); break;
    case LN_FROB2: r = g_frob(G, 2, x); break;
    case LN_FROB3: r = g_frob(G, 3, x); break;
    case LN_CONJ: r = g_conj(G, x); break;
    case LN_INV: r = g_inv<S>(G, x); break;
    default: r = g_pow_x<S>(G, x); break;
  }
  if (G.w) out[cs * 6 + k] = r;
}

__global__ void __launch_bounds__(64) k_dc_conv6(const Fq2* __restrict__ a, const Fq2* __restrict__ b,
                                                 Fq2* __restrict__ out, uint32_t jobs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= jobs) return;
  const uint32_t cs = i / 6, k = i % 6;
  out[i] = wg::conv6(a + 6 * (size_t)cs, b + 6 * (size_t)cs, (int)k);
}

// one block per case: D (ATE_NUM_LINES x 6 Fq2, coefficient 5 unused) -> M (kMaxMerge x 6 Fq2, the
// first c_merge.n steps written); the wide form's scratch X holds kMaxMerge x 25 Fq2 per case
__global__ void __launch_bounds__(wg::kThreads) k_dc_merge(int wide, const Fq2* __restrict__ D, Fq2* __restrict__ M,
                                                           Fq2* __restrict__ X) {
  const Fq2* d = D + (size_t)blockIdx.x * ATE_NUM_LINES * 6;
  Fq2* m = M + (size_t)blockIdx.x * kMaxMerge * 6;
  if (wide) wg::merge_products_wide(m, d, X + (size_t)blockIdx.x * kMaxMerge * 25, threadIdx.x, wg::kThreads);
  else merge_products(m, d, threadIdx.x, wg::kThreads);
}

// device buffers of one call: the inputs uploaded, one zeroed output, all freed on return
struct Bufs {
  static constexpr int kMax = 5;
  void* p[kMax] = {};
  hipError_t e = hipSuccess;
  void* in(int i, const void* host, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(&p[i], bytes ? bytes : 4);
    if (e == hipSuccess && bytes) e = hipMemcpy(p[i], host, bytes, hipMemcpyHostToDevice);
    return p[i];
  }
  void* zero(int i, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(&p[i], bytes);
    if (e == hipSuccess) e = hipMemset(p[i], 0, bytes);
    return p[i];
  }
  int finish(void* host, int i, size_t bytes) {
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(host, p[i], bytes, hipMemcpyDeviceToHost);
    return (int)e;
  }
  ~Bufs() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
};

}  // namespace

// sizes the Python side needs to lay out dc_prologue's merge operands; 16 + m: the first pair index
// of merged step m (the step multiplies pairs first and first + 1)
extern "C" int dc_info(int which) {
  if (which >= 16 && which < 16 + make_merges().n) return make_merges().first[which - 16];
  switch (which) {
    case 0: return ATE_NUM_LINES;
    case 1: return make_merges().n;
    case 2: return kMaxMerge;
    case 3: return wg::kL24;
    default: return -1;
  }
}

// a, b, out: n x 6 Fq2.  imm: conj flags 0-3 (w_mul), n = 1..3 (w_frob), neg_odd 0/1 (w_conj)
extern "C" int dc_wg(int op, int imm, const void* a, const void* b, void* out, size_t n) {
  bool ok = op >= 0 && op < WG_OPS && n <= kMaxCases && a && b && out;
  if (op == WG_MUL) ok = ok && imm >= 0 && imm <= 3;
  else if (op == WG_FROB) ok = ok && imm >= 1 && imm <= 3;
  else if (op == WG_CONJ) ok = ok && (imm == 0 || imm == 1);
  else ok = ok && imm == 0;
  if (!ok) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = n * kFq12Words * 4;
  Bufs B;
  const uint32_t* da = static_cast<const uint32_t*>(B.in(0, a, bytes));
  const uint32_t* db = static_cast<const uint32_t*>(B.in(1, b, bytes));
  uint32_t* dout = static_cast<uint32_t*>(B.zero(2, bytes));
  if (B.e == hipSuccess) hipLaunchKernelGGL(k_dc_wg, dim3((unsigned)n), dim3(wg::kThreads), 0, 0, op, imm, da, db, dout);
  return B.finish(out, 2, bytes);
}

// op 0: in = n x 11 signed 32-bit limbs (the unbiased lane sum) -> lz_reduce(norm24(in));
// op 1: in = n x 9 words -> lz_reduce(in).  out: n x 8 words
extern "C" int dc_norm24(int op, const void* in, void* out, size_t n) {
  if (op < 0 || op >= N24_OPS || n > (1u << 20) || !in || !out) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t words = op == N24_NORM ? (size_t)wg::kL24 : 9;
  Bufs B;
  const uint32_t* din = static_cast<const uint32_t*>(B.in(0, in, n * words * 4));
  uint32_t* dout = static_cast<uint32_t*>(B.zero(1, n * 32));
  if (B.e == hipSuccess)
    hipLaunchKernelGGL(k_dc_norm24, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, din, dout, (uint32_t)n);
  return B.finish(out, 1, n * 32);
}

// a, b, out: n x 6 Fq2 (canonical); l: n x 3 Fq2 (l0, l1, l3).  n must fill whole blocks: a
// multiple of 2 at S = 4 (cases 2i and 2i + 1 share a wave), any n at S = 8
extern "C" int dc_lanes(int S, int op, const void* a, const void* b, const void* l, void* out, size_t n) {
  if ((S != 4 && S != 8) || op < 0 || op >= LN_OPS || n > kMaxCases || !a || !b || !l || !out)
    return (int)hipErrorInvalidValue;
  const size_t per_block = S == 4 ? 2 : 1;
  if (n % per_block != 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = n * kFq12Words * 4;
  Bufs B;
  const Fq2* da = static_cast<const Fq2*>(B.in(0, a, bytes));
  const Fq2* db = static_cast<const Fq2*>(B.in(1, b, bytes));
  const Fq2* dl = static_cast<const Fq2*>(B.in(2, l, bytes / 2));
  Fq2* dout = static_cast<Fq2*>(B.zero(3, bytes));
  if (B.e == hipSuccess) {
    const dim3 grid((unsigned)(n / per_block));
    if (S == 4) hipLaunchKernelGGL(k_dc_lanes<4>, grid, dim3(64), 0, 0, op, da, db, dl, dout);
    else hipLaunchKernelGGL(k_dc_lanes<8>, grid, dim3(64), 0, 0, op, da, db, dl, dout);
  }
  return B.finish(out, 3, bytes);
}

// op 0: out[c][k] = conv6(a[c], b[c], k); a, b, out: n x 6 Fq2.
// op 1 / 2: merge_products / merge_products_wide; a: n x (ATE_NUM_LINES x 6) Fq2 (the pair products
// D), b unused, out: n x (kMaxMerge x 6) Fq2 of which the first dc_info(1) x 6 are written
extern "C" int dc_prologue(int op, const void* a, const void* b, void* out, size_t n) {
  if (op < 0 || op >= PR_OPS || !a || !out || (op == PR_CONV6 && !b)) return (int)hipErrorInvalidValue;
  if (n > (op == PR_CONV6 ? kMaxCases : 64)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  Bufs B;
  if (op == PR_CONV6) {
    const size_t bytes = n * kFq12Words * 4;
    const Fq2* da = static_cast<const Fq2*>(B.in(0, a, bytes));
    const Fq2* db = static_cast<const Fq2*>(B.in(1, b, bytes));
    Fq2* dout = static_cast<Fq2*>(B.zero(2, bytes));
    const uint32_t jobs = (uint32_t)(n * 6);
    if (B.e == hipSuccess)
      hipLaunchKernelGGL(k_dc_conv6, dim3((jobs + 63) / 64), dim3(64), 0, 0, da, db, dout, jobs);
    return B.finish(out, 2, bytes);
  }
  const size_t in_bytes = n * ATE_NUM_LINES * 6 * sizeof(Fq2), out_bytes = n * kMaxMerge * 6 * sizeof(Fq2);
  const Fq2* dd = static_cast<const Fq2*>(B.in(0, a, in_bytes));
  Fq2* dm = static_cast<Fq2*>(B.zero(1, out_bytes));
  Fq2* dx = static_cast<Fq2*>(B.zero(2, n * kMaxMerge * 25 * sizeof(Fq2)));
  if (B.e == hipSuccess)
    hipLaunchKernelGGL(k_dc_merge, dim3((unsigned)n), dim3(wg::kThreads), 0, 0, op == PR_MERGE_WIDE ? 1 : 0, dd, dm, dx);
  return B.finish(out, 1, out_bytes);
}
