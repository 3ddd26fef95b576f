// Running products and batch inversion over BN254 Fr columns on the device: the permutation and
// lookup z columns of a halo2 prover, for columns that are already in HBM (see grand_product.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgpu.h"

namespace sv {

// Rows per block of the scans (kGpThreads threads x kGpPer consecutive rows each).  One block of
// kGpThreads threads scans the block totals, ceil(blocks / kGpThreads) of them per thread, so the
// only other size at which a loop count changes is kGpThreads * kGpSpan + 1.
constexpr uint32_t kGpSpan = 1024;
constexpr uint32_t kGpThreads = 256;
constexpr uint32_t kGpPer = kGpSpan / kGpThreads;
constexpr size_t kGpMaxRows = size_t(1) << 26;

// One call: the two sides' factors (host copies of the caller's descriptors; s and c in `form`), or
// -- invert -- the one column d_in, whose zeros stay zero.
struct GpCall {
  const sv_fr_factor* num;
  size_t n_num;
  const sv_fr_factor* den;
  size_t n_den;
  size_t n;
  sv_fe z0;            // in `form` (invert: unused)
  const sv_fe* omega;  // in `form`; read when a factor is SV_FACTOR_IDENTITY
  int form;
  bool invert;         // batch inversion of num[0].d_x (n_num == 1, n_den == 0)
  void* d_out;         // z, or the inverses (may be the column itself when invert)
};

// Device scratch of one call: the grand total z0 N / D (32 B, in the call's form) at offset 0, the
// error flag (u32: an element not below r) at offset 32, then the block totals and carries of both
// sides and the per-block flags, and -- grand product -- the rows' two products (64 B per row,
// rounded up to whole spans), which the first launch writes and the last one reads.
constexpr size_t kGpTotalOffset = 0, kGpErrOffset = 32, kGpHeadBytes = 64;
size_t grand_product_scratch_bytes(size_t n, bool invert);

// Enqueues the three launches on `st`.  Nothing is synchronised: the caller reads the first
// kGpHeadBytes of d_scratch (layout above) after the stream has drained.
int grand_product_enqueue(const GpCall& call, void* d_scratch, hipStream_t st);

}  // namespace sv
