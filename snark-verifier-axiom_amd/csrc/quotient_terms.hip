// The fixed-function terms of a halo2 quotient numerator over BN254 Fr columns that are already in
// HBM on the extended domain: the permutation argument's constraints
// (snark-verifier/src/system/halo2.rs:501-591) and each lookup's five (:593-655), joined onto a
// running accumulator by the Horner fold in y of :657-668,  acc <- acc y + c  per constraint c.
//
// One launch per call.  Every constraint is a selector column (l0, l_last or l_active) times an
// expression e_i, so with T constraints the fold is
//   out = acc_in y^T + l0 S0 + l_last SL + l_active SA,   S* = sum over its constraints of y^(T-1-i) e_i,
// and the field is exact: the result is the Horner fold's, bit for bit.  A thread keeps S0, SL and
// SA of its kQtPer consecutive rows in registers, walks the constraints once, and meets the three
// selector columns and the accumulator once, at the end.  The powers of y, one per constraint, come
// from the host with the column pointers in the call's table (pooled scratch, one small copy).
//
// Columns travel as in grand_product.hip: 16 B per lane, consecutive lanes consecutive addresses,
// through LDS images padded by 16 B per four rows, and d_out goes back the same way.  A rotation
// by one row of the original domain is 2^log_ext <= kQtHalo rows of the extended one, so the block
// stages its span and that halo in one image and reads z and rot(z, 1) (a' and rot(a', -1)) from
// the same staged rows: the column is read 1 + 2^log_ext / kQtSpan times, not twice.  Only
// rot(z_(i-1), last_rotation), arbitrarily far away, is a second read of its column.  Rows wrap
// mod N where they are staged.  X_j = g omega_K^j: the block's first wave builds g omega_K^(block's
// first row) from the host's seeds omega_K^(2^b) in the kernel arguments, a thread multiplies its
// own offset in (two table entries, one per 4-bit digit of its index) and steps by omega_K.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "field.hpp"
#include "ntt.hpp"
#include "quotient_terms.hpp"
#include "runtime.hpp"

namespace sv {

namespace {

constexpr int kP = (int)kQtPer;
constexpr int kNT = (int)kQtThreads;
constexpr int kSpan = (int)kQtSpan;
constexpr int kChunkRows = 4;                                  // rows per chunk of an LDS image
constexpr int kChunkQ = 2 * kChunkRows + 1;                    // uint4 per chunk (16 B of padding)
constexpr int kPlainQ = (kSpan / kChunkRows) * kChunkQ;        // an image of the span
constexpr int kHaloRows = kSpan + (int)kQtHalo;
constexpr int kHaloQ = (kHaloRows / kChunkRows) * kChunkQ;     // an image of the span and the widest halo
static_assert((kHaloQ + 2 * kPlainQ) * 16 <= 65536, "the three images fit a block's static LDS");
constexpr int kSeeds = SV_NTT_MAX_LOG;
constexpr int ilog2(uint32_t v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
constexpr int kSpanLog = ilog2(kQtSpan);
static_assert((1u << kSpanLog) == kQtSpan && kNT == 256, "a span is a power of two; a thread index is two 4-bit digits");
static_assert(kSpan % kChunkRows == 0 && kHaloRows % kChunkRows == 0, "whole chunks");

// The call's table in pooled scratch (the host's copy of it in pinned memory).
struct PermTable {
  uint32_t err, pad[7];
  const uint4* cols[SV_TERMS_COLUMNS_MAX];
  const uint4* sigmas[SV_TERMS_COLUMNS_MAX];
  const uint4* z[SV_TERMS_COLUMNS_MAX];
  Fr s[SV_TERMS_COLUMNS_MAX];             // Montgomery
  Fr wlo[16], whi[16];                    // omega_K^(kQtPer i) and omega_K^(16 kQtPer i): a thread's offset
  Fr ypow[2 * SV_TERMS_COLUMNS_MAX + 1];  // y^(T - 1 - i) of constraint i, Montgomery
};
struct LookupCols {
  const uint4 *z, *pa, *ps, *a, *s;
};
struct LookupTable {
  uint32_t err, pad[7];
  LookupCols c[SV_TERMS_LOOKUPS_MAX];
  Fr ypow[5 * SV_TERMS_LOOKUPS_MAX];
};
static_assert(offsetof(PermTable, err) == kQtErrOffset && offsetof(LookupTable, err) == kQtErrOffset, "the flag");

// What both kernels share, by value in the kernel arguments (wave-uniform: scalar loads).
struct TermsArgs {
  const uint4 *l0, *l_last, *l_active;
  const uint4* acc_in;  // may be null
  uint4* out;
  Fr beta, gamma, y_all;  // y_all = y^T
  uint32_t log_size;      // K
  uint32_t ext;           // E = 2^log_ext: the rows of one rotation
};
struct PermArgs {
  TermsArgs t;
  PermTable* tab;
  Fr g;           // the shift
  Fr pw[kSeeds];  // omega_K^(2^b)
  uint32_t m, chunk, n_z;
  uint32_t last_off;  // (N + last_rotation E) mod N
};
struct LookupArgs {
  TermsArgs t;
  LookupTable* tab;
  uint32_t n_lookups;
};
static_assert(sizeof(PermArgs) <= 3840, "kernel arguments hold 4 KiB");

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

// slot of the q-th uint4 of the staged rows in a padded image
__device__ __forceinline__ int image_slot(int q) { return (q / (2 * kChunkRows)) * kChunkQ + (q % (2 * kChunkRows)); }

// The block's place in the column: its first row, the rows of its span that exist, N - 1.
struct Span {
  uint64_t row0, mask;
  int live;
};
__device__ __forceinline__ Span block_span(uint32_t log_size) {
  Span s;
  const uint64_t n = 1ull << log_size;
  s.row0 = (uint64_t)blockIdx.x * kSpan;
  s.mask = n - 1;
  s.live = (int)(n - s.row0 < (uint64_t)kSpan ? n - s.row0 : (uint64_t)kSpan);
  return s;
}

// Rows [first, first + rows) mod N of a column into an image; rows <= kMaxRows.
template <int kMaxRows>
__device__ __forceinline__ void stage_rows(uint4* im, const uint4* __restrict__ col, uint64_t first, int rows,
                                           uint64_t mask) {
  constexpr int kIter = (2 * kMaxRows + kNT - 1) / kNT;
  const int t = (int)threadIdx.x;
  uint4 v[kIter];
#pragma unroll
  for (int k = 0; k < kIter; k++) {
    const int q = t + k * kNT;
    v[k] = q < 2 * rows ? col[2 * ((first + (uint64_t)(q >> 1)) & mask) + (uint64_t)(q & 1)] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < kIter; k++) {
    const int q = t + k * kNT;
    if (q < 2 * rows) im[image_slot(q)] = v[k];
  }
}
__device__ __forceinline__ void stage_span(uint4* im, const uint4* col, const Span& s, uint64_t off) {
  stage_rows<kSpan>(im, col, (s.row0 + off) & s.mask, s.live, s.mask);
}
__device__ __forceinline__ void stage_halo(uint4* im, const uint4* col, const Span& s, uint64_t off, uint32_t ext) {
  stage_rows<kHaloRows>(im, col, (s.row0 + off) & s.mask, s.live + (int)ext, s.mask);
}

// Staged row `row` of an image: checked below r, in Montgomery form; zero where the thread's row
// does not exist.
template <bool kMont>
__device__ __forceinline__ Fr staged(const uint4* im, int row, bool live, bool& bad) {
  Fr a = fe_select(live, ld_fr(im + image_slot(2 * row)), Fr::zero());
  bad |= !a.is_reduced();
  return kMont ? a : fe_to_mont(a);
}

// out = acc_in y^T + l0 S0 + l_last SL + l_active SA for the thread's rows, through the image, and
// the block's flag.  sm: two plain images.
template <bool kMont>
__device__ __forceinline__ void finish(uint4* sm, const TermsArgs& a, const Span& sp, uint32_t live,
                                       Fr (&S0)[kP], const Fr (&SL)[kP], const Fr (&SA)[kP], bool bad,
                                       uint32_t* err) {
  const int t = (int)threadIdx.x;
  uint4* imA = sm;
  uint4* imB = sm + kPlainQ;
  stage_span(imA, a.l0, sp, 0);
  stage_span(imB, a.l_last, sp, 0);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kP; k++)
    S0[k] = staged<kMont>(imA, kP * t + k, (live >> k) & 1u, bad) * S0[k] +
            staged<kMont>(imB, kP * t + k, (live >> k) & 1u, bad) * SL[k];
  __syncthreads();
  stage_span(imA, a.l_active, sp, 0);
  if (a.acc_in) stage_span(imB, a.acc_in, sp, 0);
  __syncthreads();
  Fr o[kP];
#pragma unroll
  for (int k = 0; k < kP; k++) {
    o[k] = S0[k] + staged<kMont>(imA, kP * t + k, (live >> k) & 1u, bad) * SA[k];
    if (a.acc_in) o[k] = o[k] + staged<kMont>(imB, kP * t + k, (live >> k) & 1u, bad) * a.y_all;
  }
  const int any_bad = __syncthreads_or(bad);  // and the images are consumed
#pragma unroll
  for (int k = 0; k < kP; k++) st_fr(imA + image_slot(2 * (kP * t + k)), kMont ? o[k] : fe_from_mont(o[k]));
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2 * kP; k++) {
    const int q = t + k * kNT;
    if (q < 2 * sp.live) a.out[2 * sp.row0 + q] = imA[image_slot(q)];
  }
  if (any_bad && t == 0) atomicOr(err, 1u);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT, 2) k_qt_permutation(const PermArgs a) {
  __shared__ uint4 sm[kHaloQ + 2 * kPlainQ];
  uint4* imZ = sm;
  uint4* imA = sm + kHaloQ;
  uint4* imB = imA + kPlainQ;
  const int t = (int)threadIdx.x;
  const Span sp = block_span(a.t.log_size);
  const PermTable& tab = *a.tab;
  uint32_t live = 0;  // bit k: the thread's row k exists
#pragma unroll
  for (int k = 0; k < kP; k++) live |= (kP * t + k < sp.live ? 1u : 0u) << k;
  bool bad = false;

  // X[k] = g omega_K^(row0 + kP t + k)
  Fr X[kP];
  if (t < 64) {  // the block's first wave: g omega_K^row0, the same in every lane
    Fr b = a.g;
    for (int i = kSpanLog; i < kSeeds; i++)
      if ((sp.row0 >> i) & 1u) b = b * a.pw[i];
    if (t == 0) st_fr(imZ, b);
  }
  X[0] = tab.wlo[t & 15] * tab.whi[t >> 4];
  __syncthreads();
  X[0] = X[0] * ld_fr(imZ);
#pragma unroll
  for (int k = 1; k < kP; k++) X[k] = X[k - 1] * a.pw[0];
  __syncthreads();  // imZ is staged into next

  Fr S0[kP], SL[kP], SA[kP];
#pragma unroll
  for (int k = 0; k < kP; k++) S0[k] = SL[k] = SA[k] = Fr::zero();
  const uint32_t nz = a.n_z;
#pragma unroll 1
  for (uint32_t i = 0; i < nz; i++) {
    const uint32_t j0 = i * a.chunk, j1 = min(j0 + a.chunk, a.m);
    Fr left[kP], right[kP];
#pragma unroll 1
    for (uint32_t j = j0; j < j1; j++) {
      stage_span(imA, tab.cols[j], sp, 0);
      stage_span(imB, tab.sigmas[j], sp, 0);
      __syncthreads();
      const Fr sj = tab.s[j];
#pragma unroll
      for (int k = 0; k < kP; k++) {
        const Fr v = staged<kMont>(imA, kP * t + k, (live >> k) & 1u, bad) + a.t.gamma;
        const Fr l = v + a.t.beta * staged<kMont>(imB, kP * t + k, (live >> k) & 1u, bad);
        const Fr r = v + sj * X[k];
        left[k] = j == j0 ? l : left[k] * l;
        right[k] = j == j0 ? r : right[k] * r;
      }
      __syncthreads();  // the images are consumed
    }
    stage_halo(imZ, tab.z[i], sp, 0, a.t.ext);
    if (i > 0) stage_span(imA, tab.z[i - 1], sp, a.last_off);
    __syncthreads();
    const Fr yp = tab.ypow[nz + 1 + i];
#pragma unroll
    for (int k = 0; k < kP; k++) {
      const Fr z = staged<kMont>(imZ, kP * t + k, (live >> k) & 1u, bad);
      const Fr zr = staged<kMont>(imZ, kP * t + k + (int)a.t.ext, (live >> k) & 1u, bad);
      SA[k] = SA[k] + yp * (zr * left[k] - z * right[k]);
      if (i == 0) S0[k] = S0[k] + tab.ypow[0] * (Fr::one() - z);
      if (i + 1 == nz) SL[k] = tab.ypow[1] * (z * z - z);
      if (i > 0) S0[k] = S0[k] + tab.ypow[1 + i] * (z - staged<kMont>(imA, kP * t + k, (live >> k) & 1u, bad));
    }
    __syncthreads();
  }
  finish<kMont>(imA, a.t, sp, live, S0, SL, SA, bad, &a.tab->err);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT, 2) k_qt_lookup(const LookupArgs a) {
  __shared__ uint4 sm[kHaloQ + 2 * kPlainQ];
  uint4* imZ = sm;
  uint4* imA = sm + kHaloQ;
  uint4* imB = imA + kPlainQ;
  const int t = (int)threadIdx.x;
  const Span sp = block_span(a.t.log_size);
  const LookupTable& tab = *a.tab;
  const int ext = (int)a.t.ext;
  uint32_t live = 0;  // bit k: the thread's row k exists
#pragma unroll
  for (int k = 0; k < kP; k++) live |= (kP * t + k < sp.live ? 1u : 0u) << k;
  bool bad = false;
  Fr S0[kP], SL[kP], SA[kP];
#pragma unroll
  for (int k = 0; k < kP; k++) S0[k] = SL[k] = SA[k] = Fr::zero();
#pragma unroll 1
  for (uint32_t l = 0; l < a.n_lookups; l++) {
    const LookupCols c = tab.c[l];
    const Fr* yp = tab.ypow + 5 * l;
    stage_halo(imZ, c.z, sp, 0, a.t.ext);
    stage_span(imA, c.a, sp, 0);
    stage_span(imB, c.s, sp, 0);
    __syncthreads();
    Fr zr[kP], right[kP];
#pragma unroll
    for (int k = 0; k < kP; k++) {
      const Fr z = staged<kMont>(imZ, kP * t + k, (live >> k) & 1u, bad);
      zr[k] = staged<kMont>(imZ, kP * t + k + ext, (live >> k) & 1u, bad);
      right[k] = z * (staged<kMont>(imA, kP * t + k, (live >> k) & 1u, bad) + a.t.beta) *
                 (staged<kMont>(imB, kP * t + k, (live >> k) & 1u, bad) + a.t.gamma);
      S0[k] = S0[k] + yp[0] * (Fr::one() - z);
      SL[k] = SL[k] + yp[1] * (z * z - z);
    }
    __syncthreads();
    stage_halo(imZ, c.pa, sp, sp.mask + 1 - (uint64_t)ext, a.t.ext);  // from row0 - E: rot(a', -1) beside a'
    stage_span(imA, c.ps, sp, 0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kP; k++) {
      const Fr ap = staged<kMont>(imZ, kP * t + k + ext, (live >> k) & 1u, bad);
      const Fr apm = staged<kMont>(imZ, kP * t + k, (live >> k) & 1u, bad);
      const Fr ps = staged<kMont>(imA, kP * t + k, (live >> k) & 1u, bad);
      const Fr d = ap - ps;
      SA[k] = SA[k] + yp[2] * (zr[k] * (ap + a.t.beta) * (ps + a.t.gamma) - right[k]) + yp[4] * (d * (ap - apm));
      S0[k] = S0[k] + yp[3] * d;
    }
    __syncthreads();
  }
  finish<kMont>(imA, a.t, sp, live, S0, SL, SA, bad, &a.tab->err);
}

Fr fr_in(const sv_fe& a, bool mont) {
  Fr x;
  memcpy(x.v, a.l, sizeof x.v);
  return mont ? x : fe_to_mont(x);
}

const uint4* col(const void* p) { return static_cast<const uint4*>(p); }

// ypow[i] = y^(T - 1 - i); returns y^T
Fr y_powers(const Fr& y, size_t T, Fr* ypow) {
  Fr p = Fr::one();
  for (size_t i = T; i-- > 0;) {
    ypow[i] = p;
    p = p * y;
  }
  return p;
}

void terms_args(TermsArgs* t, const sv_fe* l0, const sv_fe* l_last, const sv_fe* l_active, const void* acc_in,
                void* out, const sv_fe& beta, const sv_fe& gamma, uint32_t log_n, uint32_t log_ext, bool mont) {
  t->l0 = col(l0), t->l_last = col(l_last), t->l_active = col(l_active);
  t->acc_in = col(acc_in);
  t->out = static_cast<uint4*>(out);
  t->beta = fr_in(beta, mont), t->gamma = fr_in(gamma, mont);
  t->log_size = log_n + log_ext;
  t->ext = 1u << log_ext;
}

uint32_t blocks_for(uint32_t log_size) { return (uint32_t)(((1ull << log_size) + kQtSpan - 1) / kQtSpan); }

}  // namespace

size_t quotient_terms_table_bytes(bool lookups) { return lookups ? sizeof(LookupTable) : sizeof(PermTable); }

int permutation_terms_enqueue(const QtPermCall& call, void* d_scratch, void* h_stage, hipStream_t st) {
  static_assert(sizeof(Fr) == sizeof(sv_fe), "Fr is the ABI's element");
  const bool mont = call.form == SV_MONTGOMERY;
  const uint32_t K = call.log_n + call.log_ext;
  const size_t n_z = (call.m + call.chunk - 1) / call.chunk;
  if (call.m == 0 || call.m > SV_TERMS_COLUMNS_MAX || K > SV_NTT_MAX_LOG || call.log_ext > SV_EXT_LOG_MAX) {
    set_error("permutation terms: m = %zu, K = %u, log_ext = %u out of range", call.m, K, call.log_ext);
    return SV_ERR_LEN;
  }
  PermTable* h = static_cast<PermTable*>(h_stage);
  memset(h, 0, sizeof *h);
  for (size_t j = 0; j < call.m; j++) {
    h->cols[j] = col(call.d_cols[j]);
    h->sigmas[j] = col(call.d_sigmas[j]);
    h->s[j] = fr_in(call.s[j], mont);
  }
  for (size_t i = 0; i < n_z; i++) h->z[i] = col(call.d_z[i]);
  PermArgs a;
  memset(&a, 0, sizeof a);
  terms_args(&a.t, call.d_l0, call.d_l_last, call.d_l_active, call.d_acc_in, call.d_out, call.beta, call.gamma,
             call.log_n, call.log_ext, mont);
  a.t.y_all = y_powers(fr_in(call.y, mont), 2 * n_z + 1, h->ypow);
  a.tab = static_cast<PermTable*>(d_scratch);
  a.g = call.has_shift ? fr_in(call.shift, mont) : Fr::one();
  sv_fe root;
  SV_TRY(fr_root_of_unity(K, SV_MONTGOMERY, &root));
  Fr w = fr_in(root, true);
  for (int b = 0; b < kSeeds; b++) {
    a.pw[b] = w;
    w = fe_sqr(w);
  }
  h->wlo[0] = Fr::one();
  for (int i = 1; i < 16; i++) {
    h->wlo[i] = h->wlo[i - 1];
    for (int k = 0; k < kP; k++) h->wlo[i] = h->wlo[i] * a.pw[0];
  }
  h->whi[0] = Fr::one();
  const Fr w16 = h->wlo[15] * h->wlo[1];
  for (int i = 1; i < 16; i++) h->whi[i] = h->whi[i - 1] * w16;
  a.m = (uint32_t)call.m, a.chunk = (uint32_t)std::min(call.chunk, call.m), a.n_z = (uint32_t)n_z;
  const int64_t N = int64_t(1) << K;
  a.last_off = (uint32_t)(N + (int64_t)call.last_rotation * (int64_t)a.t.ext);
  SV_HIP(hipMemcpyAsync(d_scratch, h, sizeof *h, hipMemcpyHostToDevice, st));
  if (mont) hipLaunchKernelGGL(k_qt_permutation<true>, dim3(blocks_for(K)), dim3(kNT), 0, st, a);
  else hipLaunchKernelGGL(k_qt_permutation<false>, dim3(blocks_for(K)), dim3(kNT), 0, st, a);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

int lookup_terms_enqueue(const QtLookupCall& call, void* d_scratch, void* h_stage, hipStream_t st) {
  const bool mont = call.form == SV_MONTGOMERY;
  const uint32_t K = call.log_n + call.log_ext;
  if (call.n_lookups == 0 || call.n_lookups > SV_TERMS_LOOKUPS_MAX || K > SV_NTT_MAX_LOG ||
      call.log_ext > SV_EXT_LOG_MAX) {
    set_error("lookup terms: %zu lookups, K = %u, log_ext = %u out of range", call.n_lookups, K, call.log_ext);
    return SV_ERR_LEN;
  }
  LookupTable* h = static_cast<LookupTable*>(h_stage);
  memset(h, 0, sizeof *h);
  for (size_t l = 0; l < call.n_lookups; l++) {
    const sv_fr_lookup& d = call.lookups[l];
    h->c[l] = LookupCols{col(d.d_z), col(d.d_permuted_input), col(d.d_permuted_table), col(d.d_input), col(d.d_table)};
  }
  LookupArgs a;
  memset(&a, 0, sizeof a);
  terms_args(&a.t, call.d_l0, call.d_l_last, call.d_l_active, call.d_acc_in, call.d_out, call.beta, call.gamma,
             call.log_n, call.log_ext, mont);
  a.t.y_all = y_powers(fr_in(call.y, mont), 5 * call.n_lookups, h->ypow);
  a.tab = static_cast<LookupTable*>(d_scratch);
  a.n_lookups = (uint32_t)call.n_lookups;
  SV_HIP(hipMemcpyAsync(d_scratch, h, sizeof *h, hipMemcpyHostToDevice, st));
  if (mont) hipLaunchKernelGGL(k_qt_lookup<true>, dim3(blocks_for(K)), dim3(kNT), 0, st, a);
  else hipLaunchKernelGGL(k_qt_lookup<false>, dim3(blocks_for(K)), dim3(kNT), 0, st, a);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

}  // namespace sv
