// The fixed-function terms of a halo2 quotient numerator on extended columns in HBM: the
// permutation argument's constraints and each lookup's five, folded in y onto a running
// accumulator (see quotient_terms.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgpu.h"

namespace sv {

// Rows per block (kQtThreads threads x kQtPer consecutive rows each) and the widest halo a block
// stages beside its span: a rotation by one row of the original domain is 2^log_ext <= kQtHalo rows.
constexpr uint32_t kQtThreads = 256;
constexpr uint32_t kQtPer = 1;
constexpr uint32_t kQtSpan = kQtThreads * kQtPer;
constexpr uint32_t kQtHalo = 1u << SV_EXT_LOG_MAX;

// One call past its argument rules (host copies of the caller's arrays; scalars in `form`).
struct QtPermCall {
  const sv_fe* const* d_cols;
  const sv_fe* const* d_sigmas;
  const sv_fe* s;
  size_t m, chunk;
  const sv_fe* const* d_z;
  const sv_fe *d_l0, *d_l_last, *d_l_active;
  sv_fe beta, gamma, y;
  bool has_shift;
  sv_fe shift;
  int32_t last_rotation;
  const void* d_acc_in;  // may be null
  void* d_out;
  uint32_t log_n, log_ext;
  int form;
};
struct QtLookupCall {
  const sv_fr_lookup* lookups;
  size_t n_lookups;
  const sv_fe *d_l0, *d_l_last, *d_l_active;
  sv_fe beta, gamma, y;
  const void* d_acc_in;  // may be null
  void* d_out;
  uint32_t log_n, log_ext;
  int form;
};

// Device scratch of one call: its table -- the error flag (u32: an element not below r) at
// kQtErrOffset, then the column pointers, the s_j and one power of y per constraint.  The host
// builds the table in h_stage (as many bytes of pinned memory, valid until the stream has drained)
// and one copy on the call's stream carries it over, the cleared flag included.
constexpr size_t kQtErrOffset = 0;
size_t quotient_terms_table_bytes(bool lookups);

// Enqueues the copy and the one launch on `st`.  Nothing is synchronised: the caller reads the flag
// after the stream has drained.
int permutation_terms_enqueue(const QtPermCall& call, void* d_scratch, void* h_stage, hipStream_t st);
int lookup_terms_enqueue(const QtLookupCall& call, void* d_scratch, void* h_stage, hipStream_t st);

}  // namespace sv
