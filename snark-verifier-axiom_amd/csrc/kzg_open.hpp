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

}  // namespace sv
