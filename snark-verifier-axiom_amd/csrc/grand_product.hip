// Running products over BN254 Fr columns that are already in HBM: z[0] = z0 and
// z[i + 1] = z[i] num(i) / den(i), where num(i) and den(i) are products of up to 16 factors each
// formed from the columns (x + c, x + s y + c, x + s omega^i + c) -- the permutation and lookup z
// columns of a halo2 prover -- and batch inversion of one column.
//
// One field inversion per call.  With N_<i the exclusive prefix product of the rows' numerators,
// D_>=i the inclusive suffix product of their denominators and D the product of all of them,
//   z[i] = z0 N_<i / D_<i = z0 N_<i D_>=i D^-1,
// so a call is a forward product scan, a backward product scan and one fe_inv.  Batch inversion is
// the same on one column: 1 / a_i = P_<i S_>i A^-1 with the exclusive suffix.  A row whose
// denominator is zero takes the ratio 0 / 1 (a select where the factors are formed), which leaves
// every later z zero, as halo2's batch inversion does by keeping a zero "inverse" zero; in batch
// inversion a zero enters the products as 1 and its output is masked to 0.  The scans themselves
// have no special case, and the field is exact: every output is determined bit for bit.
//
// Three launches in stream order that never wait for another block (kzg_open.hip's division has
// the reason: no look-back on a shared device):
//   1. k_gp_reduce   each block forms the two products of its span's kGpSpan rows, checks that every
//                    element read is below r (a plain per-block flag), leaves the rows' products in
//                    pooled scratch and multiplies them into the block's two totals (a tree over the
//                    threads);
//   2. k_gp_carries  one block scans the totals: the exclusive prefix of the numerator totals, the
//                    exclusive suffix of the denominator totals; its thread 0 runs the one fe_inv
//                    and z0 D^-1 is folded into the prefix carries, so it costs no product per row;
//                    the grand total z0 N / D and the folded flag go to the call's head;
//   3. k_gp_apply    each block reads its rows' products back (batch inversion: its one column again),
//                    scans the thread products in LDS (prefix and suffix between the same barriers)
//                    seeded with its two carries, and writes z.
// The columns are read once: the second launch takes 64 B per row from scratch instead of forming the
// factors again, which measured faster for both prover shapes ("tried and rejected").
// A thread owns kGpPer consecutive rows.  Columns travel as in the division: 16 B per lane,
// consecutive lanes consecutive addresses, through LDS images padded by 16 B per thread chunk, and
// z goes back the same way, so global traffic is in coalesced 16-B runs.  omega^i: a thread builds
// omega^(its first row) from the host's seeds omega^(2^b) in the kernel arguments and steps by omega.
#include <hip/hip_runtime.h>

#include <cstring>

#include "field.hpp"
#include "grand_product.hpp"
#include "runtime.hpp"

namespace sv {

namespace {

constexpr int kP = (int)kGpPer;              // rows per thread
constexpr int kNT = (int)kGpThreads;         // threads per block
constexpr int kChunkQ = 2 * kP + 1;          // uint4 per thread chunk of the LDS image (16 B of padding)
constexpr int kImageQ = kNT * kChunkQ;       // uint4 in the image
constexpr int kScanQ = 2 * kNT;              // uint4 in one array of thread values
constexpr int kSeeds = 26;                   // omega^(2^b), b < log2 kGpMaxRows
static_assert(kGpSpan == kGpThreads * kGpPer, "span = threads x rows per thread");
static_assert(4 * kScanQ <= kImageQ, "the scans' buffers (two values, two generations) live in the image");
static_assert((size_t(1) << kSeeds) == kGpMaxRows, "a row index has kSeeds bits");

constexpr int ilog2(uint32_t v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
constexpr int kLevels = ilog2(kGpThreads);
static_assert((1u << kLevels) == kGpThreads, "the block scans double their stride per level");

struct GpFactor {
  const uint4* x;
  const uint4* y;
  Fr s, c;  // Montgomery
  uint32_t kind, pad;
};
// The call, by value in the kernel arguments (wave-uniform: scalar loads).
struct GpArgs {
  GpFactor f[2 * SV_PRODUCT_FACTORS_MAX];  // the numerator's factors, then the denominator's
  Fr pw[kSeeds];                           // omega^(2^b), Montgomery
  uint64_t n;
  uint32_t n_num, n_den;
  uint32_t has_identity;
  uint32_t pad;
};
static_assert(sizeof(GpArgs) <= 3840, "kernel arguments hold 4 KiB");

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

// slot of the span's q-th uint4 in the padded image
__device__ __forceinline__ int image_slot(int q) { return (q / (2 * kP)) * kChunkQ + (q % (2 * kP)); }

// One column's span, the uint4 [q0, q0 + 2 S) (zeros past qn), into an image.
__device__ __forceinline__ void stage_column(uint4* im, const uint4* __restrict__ col, uint64_t q0, uint64_t qn) {
  const int t = (int)threadIdx.x;
  uint4 v[2 * kP];
#pragma unroll
  for (int k = 0; k < 2 * kP; k++) {
    const uint64_t g = q0 + t + k * kNT;
    v[k] = g < qn ? col[g] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < 2 * kP; k++) im[image_slot(t + k * kNT)] = v[k];
}

// This thread's k-th row of a staged column: checked below r, in Montgomery form.
template <bool kMont>
__device__ __forceinline__ Fr staged_row(const uint4* im, int k, bool& bad) {
  Fr a = ld_fr(im + (int)threadIdx.x * kChunkQ + 2 * k);
  bad |= !a.is_reduced();
  return kMont ? a : fe_to_mont(a);
}

// The product of one side's `count` factors (from a.f[first]) at each of this thread's rows.  A
// factor's columns are staged in the two images (x, and the y of a COLUMN factor) between one pair
// of barriers and read from there row by row: a register copy of a column is what the kernels have
// no room for beside the two sides' products and the powers of omega.
template <bool kMont>
__device__ __forceinline__ void side_rows(uint4* sm, const GpArgs& a, uint32_t first, uint32_t count, uint64_t q0,
                                          const Fr (&w)[kP], Fr (&acc)[kP], bool& bad) {
#pragma unroll
  for (int k = 0; k < kP; k++) acc[k] = Fr::one();
  for (uint32_t j = first; j < first + count; j++) {
    const uint32_t kind = a.f[j].kind;  // the same for the whole block
    stage_column(sm, a.f[j].x, q0, 2 * a.n);
    if (kind == SV_FACTOR_COLUMN) stage_column(sm + kImageQ, a.f[j].y, q0, 2 * a.n);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kP; k++) {
      Fr f = staged_row<kMont>(sm, k, bad) + a.f[j].c;
      if (kind == SV_FACTOR_COLUMN) f = f + a.f[j].s * staged_row<kMont>(sm + kImageQ, k, bad);
      if (kind == SV_FACTOR_IDENTITY) f = f + a.f[j].s * w[k];
      acc[k] = j == first ? f : acc[k] * f;
    }
    __syncthreads();  // the images are consumed
  }
}

// This thread's rows: num[k] and den[k] with the zero rules applied, 1 / 1 past the last row.
// Returns the mask of the rows whose input is zero (batch inversion: their output).
template <bool kMont, bool kInvert>
__device__ __forceinline__ uint32_t form_rows(uint4* sm, const GpArgs& a, Fr (&num)[kP], Fr (&den)[kP], bool& bad) {
  const uint64_t row0 = (uint64_t)blockIdx.x * kGpSpan + (uint64_t)threadIdx.x * kP;
  const uint64_t q0 = (uint64_t)blockIdx.x * (2 * kGpSpan);
  Fr w[kP];
#pragma unroll
  for (int k = 0; k < kP; k++) w[k] = Fr::one();
  if (a.has_identity) {
    for (int b = 0; b < kSeeds; b++)
      if ((row0 >> b) & 1u) w[0] = w[0] * a.pw[b];
#pragma unroll
    for (int k = 1; k < kP; k++) w[k] = w[k - 1] * a.pw[0];
  }
  side_rows<kMont>(sm, a, 0, a.n_num, q0, w, num, bad);
  if (!kInvert) side_rows<kMont>(sm, a, a.n_num, a.n_den, q0, w, den, bad);
  uint32_t zmask = 0;
#pragma unroll
  for (int k = 0; k < kP; k++) {
    const bool live = row0 + k < a.n;
    if (kInvert) {
      const bool z = num[k].is_zero();
      zmask |= (z ? 1u : 0u) << k;
      num[k] = fe_select(z || !live, Fr::one(), num[k]);
      den[k] = num[k];
    } else {
      const bool z = den[k].is_zero();
      num[k] = fe_select(!live, Fr::one(), fe_select(z, Fr::zero(), num[k]));
      den[k] = fe_select(z || !live, Fr::one(), den[k]);
    }
  }
  return zmask;
}

// The products of a and of b over the block's threads, returned by thread 0: a tree whose level l
// folds neighbouring pairs of the kNT >> l values left by the level before.
__device__ __forceinline__ void block_product2(uint4* sm, Fr& a, Fr& b) {
  const int t = (int)threadIdx.x;
  uint4* cur = sm;
  uint4* nxt = sm + 2 * kScanQ;
  st_fr(cur + 2 * t, a);
  st_fr(cur + kScanQ + 2 * t, b);
  __syncthreads();
#pragma unroll 1
  for (int l = 0; l < kLevels; l++) {
    if (t < (kNT >> (l + 1))) {
      a = ld_fr(cur + 4 * t) * ld_fr(cur + 4 * t + 2);
      b = ld_fr(cur + kScanQ + 4 * t) * ld_fr(cur + kScanQ + 4 * t + 2);
      st_fr(nxt + 2 * t, a);
      st_fr(nxt + kScanQ + 2 * t, b);
    }
    __syncthreads();
    uint4* s = cur;
    cur = nxt, nxt = s;
  }
}

// Two Hillis-Steele scans between the same barriers: p becomes the inclusive prefix product over
// the threads, s the inclusive suffix product.  Every thread's results are left in *result (p of
// thread t at 2 t, s at kScanQ + 2 t); the caller synchronises before it overwrites sm.
__device__ __forceinline__ void block_scan2(uint4* sm, Fr& p, Fr& s, const uint4** result) {
  const int t = (int)threadIdx.x;
  uint4* cur = sm;
  uint4* nxt = sm + 2 * kScanQ;
  st_fr(cur + 2 * t, p);
  st_fr(cur + kScanQ + 2 * t, s);
  __syncthreads();
#pragma unroll 1
  for (int l = 0; l < kLevels; l++) {
    const int d = 1 << l;
    if (t >= d) p = p * ld_fr(cur + 2 * (t - d));
    if (t + d < kNT) s = s * ld_fr(cur + kScanQ + 2 * (t + d));
    st_fr(nxt + 2 * t, p);
    st_fr(nxt + kScanQ + 2 * t, s);
    __syncthreads();  // one barrier per level: the level after this one writes the buffer read here
    uint4* x = cur;
    cur = nxt, nxt = x;
  }
  *result = cur;
}

// A thread's per-row products in pooled scratch, which k_gp_reduce leaves for k_gp_apply: the layout
// is the kernels' own, 16 B per lane with consecutive lanes at consecutive addresses.
__device__ __forceinline__ uint4* prod_slot(uint4* prods, int side, int k, int half) {
  return prods + (size_t)blockIdx.x * (4 * kP * kNT) + ((side * kP + k) * 2 + half) * kNT + threadIdx.x;
}

template <bool kMont, bool kInvert>
__global__ void __launch_bounds__(kNT, 2) k_gp_reduce(const GpArgs a, Fr* __restrict__ totals,
                                                    uint32_t* __restrict__ flags, uint4* __restrict__ prods) {
  __shared__ uint4 sm[2 * kImageQ];
  Fr num[kP], den[kP];
  bool bad = false;
  (void)form_rows<kMont, kInvert>(sm, a, num, den, bad);
  if (!kInvert) {
#pragma unroll
    for (int k = 0; k < kP; k++) {
      *prod_slot(prods, 0, k, 0) = make_uint4(num[k].v[0], num[k].v[1], num[k].v[2], num[k].v[3]);
      *prod_slot(prods, 0, k, 1) = make_uint4(num[k].v[4], num[k].v[5], num[k].v[6], num[k].v[7]);
      *prod_slot(prods, 1, k, 0) = make_uint4(den[k].v[0], den[k].v[1], den[k].v[2], den[k].v[3]);
      *prod_slot(prods, 1, k, 1) = make_uint4(den[k].v[4], den[k].v[5], den[k].v[6], den[k].v[7]);
    }
  }
  Fr N = num[0], D = den[0];
#pragma unroll
  for (int k = 1; k < kP; k++) N = N * num[k], D = D * den[k];
  const int any_bad = __syncthreads_or(bad);
  block_product2(sm, N, D);
  if (threadIdx.x == 0) {
    totals[blockIdx.x] = N;
    totals[gridDim.x + blockIdx.x] = D;
    flags[blockIdx.x] = any_bad ? 1u : 0u;
  }
}

// One block over the nb pairs of block totals, c = ceil(nb / kNT) consecutive pairs per thread:
// carries[b] = z0 D^-1 prod_{u < b} N_u, carries[nb + b] = prod_{u > b} D_u, *total = z0 N / D,
// *err = any block's flag.  has_den == 0 (no denominator factors): every D_u is 1 and no inversion runs.
__global__ void __launch_bounds__(kNT) k_gp_carries(const Fr* __restrict__ totals, const uint32_t* __restrict__ flags,
                                                     uint32_t nb, const Fr z0, int has_den, int out_mont,
                                                     Fr* __restrict__ carries, Fr* __restrict__ total,
                                                     uint32_t* __restrict__ err) {
  __shared__ uint4 sm[4 * kScanQ + 2];
  const int t = (int)threadIdx.x;
  const uint32_t c = (nb + kNT - 1) / kNT;
  const uint32_t lo = (uint32_t)t * c;
  Fr N = Fr::one(), D = Fr::one();
  uint32_t bad = 0;
  for (uint32_t k = 0; k < c; k++)
    if (lo + k < nb) {
      N = N * totals[lo + k];
      D = D * totals[nb + lo + k];
      bad |= flags[lo + k];
    }
  const int any_bad = __syncthreads_or((int)bad);
  const uint4* res;
  block_scan2(sm, N, D, &res);
  if (t == 0) {
    Fr m = z0;
    if (has_den) m = m * fe_inv(ld_fr(res + kScanQ));  // thread 0's suffix is D, never zero
    st_fr(sm + 4 * kScanQ, m);
    const Fr tot = m * ld_fr(res + 2 * (kNT - 1));
    *total = out_mont ? tot : fe_from_mont(tot);
    *err = any_bad ? 1u : 0u;
  }
  __syncthreads();
  Fr pn = ld_fr(sm + 4 * kScanQ);
  if (t > 0) pn = pn * ld_fr(res + 2 * (t - 1));
  Fr sd = t + 1 < kNT ? ld_fr(res + kScanQ + 2 * (t + 1)) : Fr::one();
  for (uint32_t k = 0; k < c; k++)
    if (lo + k < nb) {
      carries[lo + k] = pn;
      pn = pn * totals[lo + k];
    }
  for (uint32_t k = c; k-- > 0;)
    if (lo + k < nb) {
      carries[nb + lo + k] = sd;
      sd = sd * totals[nb + lo + k];
    }
}

// Grand product: the rows' products come from scratch.  Inversion: the one column is read again (a
// block reads its whole span before it writes, so in place is safe) for the mask of its zeros.
template <bool kMont, bool kInvert>
__global__ void __launch_bounds__(kNT, 2) k_gp_apply(const GpArgs a, const Fr* __restrict__ carries, int out_mont,
                                                   uint4* __restrict__ prods, uint4* __restrict__ out) {
  __shared__ uint4 sm[(kInvert ? 2 : 1) * kImageQ];  // the second image stages a COLUMN factor's y: form_rows only
  const int t = (int)threadIdx.x;
  Fr num[kP], den[kP];
  bool bad = false;
  uint32_t zmask = 0;
  if (!kInvert) {
#pragma unroll
    for (int k = 0; k < kP; k++) {
      const uint4 n0 = *prod_slot(prods, 0, k, 0), n1 = *prod_slot(prods, 0, k, 1);
      const uint4 d0 = *prod_slot(prods, 1, k, 0), d1 = *prod_slot(prods, 1, k, 1);
      num[k].v[0] = n0.x, num[k].v[1] = n0.y, num[k].v[2] = n0.z, num[k].v[3] = n0.w;
      num[k].v[4] = n1.x, num[k].v[5] = n1.y, num[k].v[6] = n1.z, num[k].v[7] = n1.w;
      den[k].v[0] = d0.x, den[k].v[1] = d0.y, den[k].v[2] = d0.z, den[k].v[3] = d0.w;
      den[k].v[4] = d1.x, den[k].v[5] = d1.y, den[k].v[6] = d1.z, den[k].v[7] = d1.w;
    }
  } else {
    zmask = form_rows<kMont, kInvert>(sm, a, num, den, bad);
  }
  // the block's carries enter at its first and its last thread, so the scans give the true values
  Fr N = num[0], D = den[0];
#pragma unroll
  for (int k = 1; k < kP; k++) N = N * num[k], D = D * den[k];
  const Fr cn = carries[blockIdx.x], cd = carries[gridDim.x + blockIdx.x];  // wave-uniform
  if (t == 0) N = cn * N;
  if (t == kNT - 1) D = D * cd;
  const uint4* res;
  block_scan2(sm, N, D, &res);
  Fr pn = t > 0 ? ld_fr(res + 2 * (t - 1)) : cn;                   // z0 D^-1 N_<(first row)
  const Fr sd = t + 1 < kNT ? ld_fr(res + kScanQ + 2 * (t + 1)) : cd;  // D_>(last row)
  __syncthreads();  // the scans' buffers are read: the image is written again
  // sfx[k]: the product sd of the rows behind the thread times this thread's denominators from row
  // k on (grand product: z[i] takes D_>=i), or from row k + 1 on (inversion: 1 / a_i takes S_>i)
  Fr sfx[kP];
  if (kInvert) {
    sfx[kP - 1] = sd;
#pragma unroll
    for (int k = kP - 2; k >= 0; k--) sfx[k] = den[k + 1] * sfx[k + 1];
  } else {
    sfx[kP - 1] = den[kP - 1] * sd;
#pragma unroll
    for (int k = kP - 2; k >= 0; k--) sfx[k] = den[k] * sfx[k + 1];
  }
#pragma unroll
  for (int k = 0; k < kP; k++) {
    Fr z = pn * sfx[k];
    z = fe_select((zmask >> k) & 1u, Fr::zero(), z);
    st_fr(sm + t * kChunkQ + 2 * k, out_mont ? z : fe_from_mont(z));
    if (k + 1 < kP) pn = pn * num[k];
  }
  __syncthreads();
  const uint64_t q0 = (uint64_t)blockIdx.x * (2 * kGpSpan);
#pragma unroll
  for (int k = 0; k < 2 * kP; k++) {
    const int q = t + k * kNT;
    if (q0 + q < 2 * a.n) out[q0 + q] = sm[image_slot(q)];
  }
}

Fr fr_in(const sv_fe& a, bool mont) {
  Fr x;
  memcpy(x.v, a.l, sizeof x.v);
  return mont ? x : fe_to_mont(x);
}

}  // namespace

size_t grand_product_scratch_bytes(size_t n, bool invert) {
  const size_t nb = (n + kGpSpan - 1) / kGpSpan;
  const size_t small = (kGpHeadBytes + nb * (4 * sizeof(Fr) + sizeof(uint32_t)) + 255) & ~size_t(255);
  return small + (invert ? 0 : nb * kGpSpan * 2 * sizeof(Fr));
}

int grand_product_enqueue(const GpCall& call, void* d_scratch, hipStream_t st) {
  static_assert(sizeof(Fr) == sizeof(sv_fe), "Fr is the ABI's element");
  if (call.n == 0 || call.n > kGpMaxRows || call.n_num > SV_PRODUCT_FACTORS_MAX ||
      call.n_den > SV_PRODUCT_FACTORS_MAX) {
    set_error("grand product: n = %zu with %zu + %zu factors out of range", call.n, call.n_num, call.n_den);
    return SV_ERR_LEN;
  }
  const bool mont = call.form == SV_MONTGOMERY;
  const uint32_t nb = (uint32_t)((call.n + kGpSpan - 1) / kGpSpan);
  char* scratch = static_cast<char*>(d_scratch);
  Fr* total = reinterpret_cast<Fr*>(scratch + kGpTotalOffset);
  uint32_t* err = reinterpret_cast<uint32_t*>(scratch + kGpErrOffset);
  Fr* totals = reinterpret_cast<Fr*>(scratch + kGpHeadBytes);
  Fr* carries = totals + 2 * (size_t)nb;
  uint32_t* flags = reinterpret_cast<uint32_t*>(carries + 2 * (size_t)nb);

  GpArgs a;
  memset(&a, 0, sizeof a);
  a.n = call.n;
  a.n_num = (uint32_t)call.n_num;
  a.n_den = (uint32_t)call.n_den;
  for (size_t j = 0; j < call.n_num + call.n_den; j++) {
    const sv_fr_factor& f = j < call.n_num ? call.num[j] : call.den[j - call.n_num];
    GpFactor& g = a.f[j];
    g.x = reinterpret_cast<const uint4*>(f.d_x);
    g.y = reinterpret_cast<const uint4*>(f.d_y);
    g.kind = f.kind;
    g.c = fr_in(f.c, mont);
    g.s = f.kind == SV_FACTOR_PLAIN ? Fr::zero() : fr_in(f.s, mont);
    if (f.kind == SV_FACTOR_IDENTITY) a.has_identity = 1;
  }
  if (a.has_identity) {
    Fr w = fr_in(*call.omega, mont);
    for (int b = 0; b < kSeeds; b++) {
      a.pw[b] = w;
      w = fe_sqr(w);
    }
  }
  const Fr z0 = call.invert ? Fr::one() : fr_in(call.z0, mont);
  const int has_den = call.invert || call.n_den > 0;
  uint4* out = static_cast<uint4*>(call.d_out);
  uint4* prods = reinterpret_cast<uint4*>(scratch + grand_product_scratch_bytes(call.n, true));
  const int om = mont ? 1 : 0;
#define SV_GP_LAUNCH(M, I)                                                                                     \
  do {                                                                                                         \
    hipLaunchKernelGGL((k_gp_reduce<M, I>), dim3(nb), dim3(kNT), 0, st, a, totals, flags, prods);              \
    hipLaunchKernelGGL(k_gp_carries, dim3(1), dim3(kNT), 0, st, totals, flags, nb, z0, has_den, om, carries,   \
                       total, err);                                                                            \
    hipLaunchKernelGGL((k_gp_apply<M, I>), dim3(nb), dim3(kNT), 0, st, a, carries, om, prods, out);            \
  } while (0)
  if (mont && call.invert) SV_GP_LAUNCH(true, true);
  else if (mont) SV_GP_LAUNCH(true, false);
  else if (call.invert) SV_GP_LAUNCH(false, true);
  else SV_GP_LAUNCH(false, false);
#undef SV_GP_LAUNCH
  SV_HIP(hipGetLastError());
  return SV_OK;
}

}  // namespace sv
