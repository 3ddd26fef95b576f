// A stable sort of a BN254 Fr column by canonical value and, on top of it, the permuted columns
// A', S' of a halo2 lookup argument (permute_expression_pair), for columns that are already in HBM
// (see lookup_permute.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgpu.h"

namespace sv {

// Keys per block of a radix pass (kLpThreads threads x kLpPer keys each, a wave owning kLpPer runs of
// 64 consecutive keys) and rows per block of the permutation's scans.  One block of kLpThreads
// threads scans a digit's per-block counts (and the permutation's block totals), ceil(blocks /
// kLpThreads) of them per thread, so the only other size at which a loop count changes is
// kLpThreads * kLpTile + 1.
constexpr uint32_t kLpTile = 1024;
constexpr uint32_t kLpThreads = 256;
constexpr uint32_t kLpPer = kLpTile / kLpThreads;
constexpr uint32_t kLpDigits = 32;  // 8-bit digits of the canonical 256-bit value
constexpr size_t kLpMaxRows = size_t(1) << 26;

// One call: the sort of d_in into d_out (d_out may be d_in), or -- permute -- A = d_in and S =
// d_table into A' = d_out and S' = d_out_table.
struct LpCall {
  const sv_fe* d_in;
  const sv_fe* d_table;
  size_t n;
  int form;
  bool permute;
  sv_fe* d_out;
  sv_fe* d_out_table;
};

// Device scratch of one call.  The head: the error flag (u32: an element not below r) at offset 0
// and, at offset 8, UINT64_MAX - (the smallest row of A' whose value is not in the table), 0 when
// there is none (u64; an atomicMax on zeroed memory); then per sorted column its 32 digit
// histograms and the pass plan, the per-block digit counts of one pass, two canonical images per
// sorted column (32 B per row each) and -- permute -- four u32 per row (repeat flags, used flags,
// the repeated rows, the unused table positions) and the scans' block totals and carries.  Per row:
// 65 B (sort), 145 B (permute).
constexpr size_t kLpErrOffset = 0, kLpMissingOffset = 8, kLpHeadBytes = 64;
constexpr uint32_t kLpErrNotReduced = 1, kLpErrNotSorted = 2;  // bits of the error flag
size_t lookup_permute_scratch_bytes(size_t n, bool permute);

// Enqueues the launches on `st`.  Nothing is synchronised: the caller reads the first kLpHeadBytes
// of d_scratch (layout above) after the stream has drained.
int lookup_permute_enqueue(const LpCall& call, void* d_scratch, hipStream_t st);

// A batch of lookups over n rows each (sv_bn254_fr_lookup_permute_batch_device), past the checks of
// lp_batch_plan.hpp: `plan` is that call's accepted plan and names the distinct tables; the three
// arrays are host arrays of plan->count device pointers.  The scratch is plan->total bytes, laid out
// by the plan: one head of kLpHeadBytes per lookup from offset 0 (lookup j's missing row at j *
// kLpHeadBytes + kLpMissingOffset; the error flag of the whole call is head 0's), then per sorted
// column -- every input, and every distinct table unless the caller has sorted them -- a state, the
// per-block digit counts and two canonical images (65 B per row), one image per table the caller
// has sorted (32 B per row), and four u32 per row and lookup (16 B) with their block totals and
// carries.
struct LpBatchPlan;
struct LpBatchCall {
  const LpBatchPlan* plan;
  const sv_fe* const* d_inputs;
  size_t n;
  int form;
  sv_fe* const* d_out_inputs;
  sv_fe* const* d_out_tables;
};

// Enqueues the launches on `st`, their number independent of the number of lookups.  Nothing is
// synchronised: the caller reads the first plan->count heads after the stream has drained.
int lookup_permute_batch_enqueue(const LpBatchCall& call, void* d_scratch, hipStream_t st);

}  // namespace sv
