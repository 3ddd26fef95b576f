// Expression programs over extended columns in HBM: custom gate constraints folded in y onto the
// running accumulator of the terms calls, and theta-compressed lookup columns (see expressions.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgpu.h"
#include "expr_plan.hpp"

namespace sv {

constexpr uint32_t kExprThreads = 256;  // threads per block, one row each

// One call past its argument rules (host copies of the caller's arrays; scalars in `form`); `plan`
// is what expr_walk made of `program`.
struct ExprCall {
  const sv_fr_expr_op* program;
  size_t n_ops;
  const sv_fe* const* d_cols;
  size_t n_cols;
  const sv_fe* consts;
  size_t n_consts;
  sv_fe* const* d_stores;
  size_t n_stores;
  const sv_fe* y;        // read when the program folds
  const void* d_acc_in;  // may be null
  void* d_out;
  uint32_t log_n, log_ext;
  int form;
  const ExprPlan* plan;
};

// Device scratch of one call: its table -- the error flag (u32: an element not below r) at
// kExprErrOffset, then the column and store pointers, the constants, y and the ops.  The host builds
// the table in h_stage (as many bytes of pinned memory, valid until the stream has drained) and one
// copy on the call's stream carries it over, the cleared flag included.
constexpr size_t kExprErrOffset = 0;
size_t expressions_table_bytes(size_t n_ops);

// Enqueues the copy and the one launch on `st`.  Nothing is synchronised: the caller reads the flag
// after the stream has drained.
int expressions_enqueue(const ExprCall& call, void* d_scratch, void* h_stage, hipStream_t st);

}  // namespace sv
