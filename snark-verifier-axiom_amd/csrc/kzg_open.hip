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
#include <hip/hip_runtime.h>

#include <cstring>

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

// x^e by square and multiply (host: the per-call weights)
Fr pow_u32(const Fr& x, uint32_t e) {
  Fr r = Fr::one();
  for (int bit = 31; bit >= 0; bit--) {
    r = fe_sqr(r);
    if ((e >> bit) & 1u) r = r * x;
  }
  return r;
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
  // the weights: z^T, squared per level up to z^(T 2^kLevels) = z^S, then (z^S)^c and its squares
  DivWeights dw;
  memcpy(dw.z.v, z.l, sizeof dw.z.v);
  if (!mont) dw.z = fe_to_mont(dw.z);
  Fr x = dw.z;
  for (int i = 0; i < ilog2(kDivPer); i++) x = fe_sqr(x);
  for (int l = 0; l < kLevels; l++) {
    dw.step[l] = x;
    x = fe_sqr(x);
  }
  CarryWeights cw;
  cw.W = x;
  x = pow_u32(x, (nb + kDivThreads - 1) / kDivThreads);
  for (int l = 0; l < kLevels; l++) {
    cw.step[l] = x;
    x = fe_sqr(x);
  }
  const uint4* c = static_cast<const uint4*>(d_coeffs);
  hipLaunchKernelGGL(k_div_reduce, dim3(nb), dim3(kNT), 0, st, c, (uint64_t)n, dw, mont, totals, flags);
  hipLaunchKernelGGL(k_div_carries, dim3(1), dim3(kNT), 0, st, totals, flags, nb, cw, mont, carries, eval, err);
  if (d_quotient && n > 1)
    hipLaunchKernelGGL(k_div_quotient, dim3(nb), dim3(kNT), 0, st, c, (uint64_t)n, dw, mont, carries,
                       q_form == SV_MONTGOMERY ? 1 : 0, static_cast<uint4*>(d_quotient));
  SV_HIP(hipGetLastError());
  return SV_OK;
}

}  // namespace sv
