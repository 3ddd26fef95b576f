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

}  // namespace sv
