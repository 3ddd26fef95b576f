// Division of an Fr polynomial by (X - z) on the device: the step between a KZG commit and the
// witness MSM of an opening (see kzg_open.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgpu.h"

namespace sv {

// Coefficients per block of the scan (kDivThreads threads x kDivPer consecutive coefficients each).
// One block of kDivThreads threads scans the block totals, ceil(blocks / kDivThreads) of them per
// thread, so the only other size at which a loop count changes is kDivThreads * kDivSpan + 1.
constexpr uint32_t kDivSpan = 1024;
constexpr uint32_t kDivThreads = 256;
constexpr uint32_t kDivPer = kDivSpan / kDivThreads;

// Device scratch of one division: the evaluation (32 B, in the call's form) at offset 0, the error
// flag (u32: a coefficient not below r) at offset 32, then the block totals and the carries.
constexpr size_t kDivEvalOffset = 0, kDivErrOffset = 32, kDivHeadBytes = 64;
size_t poly_div_scratch_bytes(size_t n);

// Enqueues q = (p - p(z)) / (X - z) on `st` for the n coefficients at d_coeffs (`form`, as is z):
// d_quotient (n - 1 elements, Montgomery when q_form == SV_MONTGOMERY, else canonical; NULL =
// evaluate only; must not overlap d_coeffs).  Nothing is synchronised: the caller reads the first
// kDivHeadBytes of d_scratch (layout above) after the stream has drained.
int poly_div_linear_enqueue(const void* d_coeffs, size_t n, const sv_fe& z, int form, int q_form, void* d_quotient,
                            void* d_scratch, hipStream_t st);

// ---- several polynomials at one point: c = sum_j v^j p_j and e_j = p_j(z) in one pass ----
// One row of the per-call table (the host writes it, one H2D copy brings it to pooled scratch): a
// polynomial's coefficients in HBM, its length, and v^j in Montgomery form.
struct BatchRow {
  const void* coeffs;
  uint64_t len;
  sv_fe vpow;
};
static_assert(sizeof(BatchRow) == 48, "the table's row");
sv_fe poly_fr_to_mont(const sv_fe& canonical);  // a reduced Fr element into Montgomery form (host)
void poly_batch_fill_table(BatchRow* rows, const sv_fe* const* d_polys, const uint64_t* lens, size_t m,
                           const sv_fe& v, int form);
// the same with m explicit weights (in `form`) in place of the powers of v
void poly_batch_fill_table_weights(BatchRow* rows, const sv_fe* const* d_polys, const uint64_t* lens, size_t m,
                                   const sv_fe* weights, int form);

// Device scratch of one pass: the error flag (u32: a coefficient not below r) at offset 0, the m
// evaluations (32 B each, in the call's form) from offset 32, then the per-block totals (m rows of
// ceil(N / kDivSpan)) and the per-block flags.  The fold of a polynomial's totals takes
// ceil(ceil(N / kDivSpan) / kDivThreads) of them per thread, so its loop count changes where the
// division's does: at N = kDivThreads * kDivSpan + 1.
constexpr size_t kBatchErrOffset = 0, kBatchEvalsOffset = 32;
inline size_t poly_batch_head_bytes(size_t m) { return kBatchEvalsOffset + m * sizeof(sv_fe); }
size_t poly_batch_scratch_bytes(size_t m, size_t N);

// Enqueues the pass on `st` over the m rows at d_table (N = the longest length; a shorter polynomial
// is zero past its end): d_combined (N elements, Montgomery when c_form == SV_MONTGOMERY, else
// canonical; NULL = evaluate only; must not overlap a polynomial).  Nothing is synchronised: the
// caller reads the first poly_batch_head_bytes(m) of d_scratch after the stream has drained.
int poly_combine_eval_enqueue(const BatchRow* d_table, size_t m, size_t N, const sv_fe& z, int form, int c_form,
                              void* d_combined, void* d_scratch, hipStream_t st);

// ---- several polynomials at several points: every p_j(x_k) in one pass (each polynomial read once) ----
// The pass takes up to kPointsPerLaunch points per launch (K trees folded between one pair of
// barriers); more points run ceil(K / kPointsPerLaunch) launches over one set of totals.  A point's
// row of the per-call table holds its weights (the division's DivWeights and CarryWeights, computed
// on the host): kPointRowBytes each, behind the polynomials' BatchRows.
constexpr uint32_t kPointsPerLaunch = 4;
constexpr size_t kPointRowBytes = 576;
void poly_points_fill_rows(void* rows, const sv_fe* points, size_t K, int form, size_t N);

// Device scratch of one call: the error flag (u32) at offset 0, the m * K evaluations ([j * K + k],
// in the call's form) from offset 32, then the per-block totals (m * min(K, kPointsPerLaunch) rows of
// ceil(N / kDivSpan)) and the per-block flags.
constexpr size_t kPointsErrOffset = 0, kPointsEvalsOffset = 32;
inline size_t poly_points_head_bytes(size_t m, size_t K) { return kPointsEvalsOffset + m * K * sizeof(sv_fe); }
size_t poly_points_scratch_bytes(size_t m, size_t K, size_t N);

// Enqueues the passes and their folds on `st` over the m rows at d_table and the K point rows at
// d_points, whose host copy is h_points (N = the longest length).  K == 1 takes the single-point
// pass (poly_combine_eval_enqueue's, evaluate only) with the weights of h_points[0] in its
// arguments.  Nothing is synchronised: the caller reads the first poly_points_head_bytes(m, K) of
// d_scratch after the stream has drained.
int poly_eval_points_enqueue(const BatchRow* d_table, size_t m, size_t N, const void* d_points, const void* h_points,
                             size_t K, int form, void* d_scratch, hipStream_t st);

// ---- division by several roots: the quotient of p by prod_k (X - x_k), remainder dropped ----
// K runs of the three-launch division, each over the quotient of the one before (in Montgomery form,
// in d_tmp[0] and d_tmp[1] by turns: n - 1 elements each, unused when K == 1).  The first run's head
// (its flag: a raw coefficient not below r) stays at the start of d_scratch; the later runs use the
// second half of poly_div_roots_scratch_bytes(n, K).  d_quotient: n - K elements (q_form), n > K.
size_t poly_div_roots_scratch_bytes(size_t n, size_t K);
int poly_div_roots_enqueue(const void* d_coeffs, size_t n, const sv_fe* roots, size_t K, int form, int q_form,
                           void* d_quotient, void* const d_tmp[2], void* d_scratch, hipStream_t st);

// Host field helpers of the SHPLONK linearisation (Montgomery in, Montgomery out).
sv_fe poly_fr_mul(const sv_fe& a, const sv_fe& b);
sv_fe poly_fr_sub(const sv_fe& a, const sv_fe& b);
sv_fe poly_fr_inv(const sv_fe& a);  // 0 -> 0
sv_fe poly_fr_one();

}  // namespace sv
