// Expression programs over BN254 Fr columns that are already in HBM: the reference's Expression<F>
// (snark-verifier/src/verifier/plonk/protocol.rs:309-370) as a flat postfix program over an operand
// stack, evaluated independently at every row of the extended domain.  Two sinks: FOLD joins a value
// onto the running accumulator of the quotient numerator, acc <- acc y + v (the Horner fold of
// snark-verifier/src/system/halo2.rs:657-668 that the terms calls of quotient_terms.hip continue),
// and STORE writes a value to a column of its own (the theta-compression of :614-619).
//
// One launch per call, one thread per row.  Every thread of the grid executes the same op, so the
// fetch of an op, the switch on its opcode, the stack depth and every table entry (a column pointer,
// a constant, y) are wave-uniform: scalar loads and scalar branches, no divergence.  The top of the
// operand stack and the accumulator live in registers; what lies below the top lives in LDS, slot s
// of thread t as the two uint4 at [(2 s + h) kExprThreads + t], h = 0, 1: a wave's 16-byte access
// covers 1 KiB of consecutive addresses, free of bank conflicts, and a thread only ever meets its own
// slots, so the kernel has no barrier.  A push spills the old top (one LDS write), a binary op reads
// its lower operand (one LDS read), a sink refills the top if the stack is not empty.  The stack
// pointer indexes LDS, never a register array: no scratch.
//
// A COLUMN op reads global memory directly, two 16-byte loads per lane at row (j + r E) mod N: a
// wave covers one contiguous 2 KiB run, or two at the wrap.  Rows past N (a column shorter than a
// block) compute on wrapped rows and are never stored.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "expressions.hpp"
#include "field.hpp"
#include "runtime.hpp"

namespace sv {

namespace {

constexpr int kNT = (int)kExprThreads;
constexpr int kSlots = (int)kExprStackMax - 1;  // the top is a register
static_assert(kSlots * 2 * kNT * 16 <= 65536, "the stack below the top fits a block's static LDS");

// An op as the kernel reads it, two dwords so that one scalar load fetches it: the ABI's op with
// the rotation turned into a row offset.
struct DevOp {
  uint32_t word;  // op | index << 16
  uint32_t off;   // (r E) mod N
};
static_assert(sizeof(DevOp) == sizeof(sv_fr_expr_op), "an op stays 8 bytes");

// The call's table in pooled scratch (the host's copy of it in pinned memory); the ops come last
// and only those of the program travel, with one spare behind them: the kernel fetches an op ahead.
struct ExprTable {
  uint32_t err, pad[7];
  const uint4* cols[SV_EXPR_COLUMNS_MAX];
  uint4* stores[SV_EXPR_STORES_MAX];
  Fr consts[SV_EXPR_CONSTS_MAX];  // Montgomery
  Fr y;                           // Montgomery
  DevOp ops[SV_EXPR_OPS_MAX + 1];
};
static_assert(offsetof(ExprTable, err) == kExprErrOffset, "the flag");
static_assert(sizeof(ExprTable) <= 45 * 1024, "the table stays small");

// A column pointer comes out of the table, so the compiler cannot know that it points to global
// memory: said here, the accesses are global ones and not flat ones, which would count against the
// LDS counter as well.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 global_u32x4;

__device__ __forceinline__ Fr ld_fr(const uint4* q) {
  const global_u32x4* g = (const global_u32x4*)q;
  const u32x4 a = g[0], b = g[1];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_fr(uint4* q, const Fr& v) {
  global_u32x4* g = (global_u32x4*)q;
  g[0] = u32x4{v.v[0], v.v[1], v.v[2], v.v[3]};
  g[1] = u32x4{v.v[4], v.v[5], v.v[6], v.v[7]};
}

// slot s of the thread's stack in LDS
__device__ __forceinline__ Fr ld_slot(const uint4* stack, uint32_t s, int t) {
  const uint4 a = stack[(2 * s) * kNT + t], b = stack[(2 * s + 1) * kNT + t];
  Fr r;
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_slot(uint4* stack, uint32_t s, int t, const Fr& v) {
  stack[(2 * s) * kNT + t] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  stack[(2 * s + 1) * kNT + t] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

// A row of a column: checked below r where the thread's row exists, in Montgomery form.
template <bool kMont>
__device__ __forceinline__ Fr ld_row(const uint4* col, uint32_t row, bool live, bool& bad) {
  const Fr a = ld_fr(col + 2 * (size_t)row);
  bad |= live && !a.is_reduced();
  return kMont ? a : fe_to_mont(a);
}

template <bool kMont>
__global__ void __launch_bounds__(kNT, 2)
    k_expressions(const ExprTable* __restrict__ tab, uint32_t* __restrict__ err, const uint4* acc_in, uint4* out,
                  uint32_t n_ops, uint32_t log_size, uint32_t folds) {
  __shared__ uint4 stack[kSlots * 2 * kNT];
  const int t = (int)threadIdx.x;
  const uint32_t mask = (1u << log_size) - 1u;
  const uint32_t j = blockIdx.x * (uint32_t)kNT + (uint32_t)t;
  const bool live = j <= mask;
  bool bad = false;
  Fr top = Fr::zero(), acc = Fr::zero();
  if (folds && acc_in) acc = ld_row<kMont>(acc_in, j & mask, live, bad);
  uint32_t depth = 0;  // operands on the stack: the top in `top`, the others in slots 0 .. depth - 2
  DevOp next = tab->ops[0];
#pragma unroll 1
  for (uint32_t i = 0; i < n_ops; i++) {
    const DevOp o = next;
    next = tab->ops[i + 1];  // under this op's arithmetic; the spare behind the last op
    const uint32_t op = o.word & 0xffu, index = o.word >> 16;
    switch (op) {
      case SV_EXPR_COLUMN:
      case SV_EXPR_CONST: {
        if (depth) st_slot(stack, depth - 1, t, top);
        top = op == SV_EXPR_CONST ? tab->consts[index] : ld_row<kMont>(tab->cols[index], (j + o.off) & mask, live, bad);
        depth++;
        break;
      }
      case SV_EXPR_NEG: top = -top; break;
      case SV_EXPR_ADD: top = ld_slot(stack, depth - 2, t) + top, depth--; break;
      case SV_EXPR_SUB: top = ld_slot(stack, depth - 2, t) - top, depth--; break;
      case SV_EXPR_RSUB: top = top - ld_slot(stack, depth - 2, t), depth--; break;
      case SV_EXPR_MUL: top = ld_slot(stack, depth - 2, t) * top, depth--; break;
      default: {  // the sinks
        if (op == SV_EXPR_FOLD) acc = acc * tab->y + top;
        else if (live) st_fr(tab->stores[index] + 2 * (size_t)j, kMont ? top : fe_from_mont(top));
        depth--;
        if (depth) top = ld_slot(stack, depth - 1, t);
        break;
      }
    }
  }
  if (folds && live) st_fr(out + 2 * (size_t)j, kMont ? acc : fe_from_mont(acc));
  if (bad) atomicOr(err, 1u);
}

Fr fr_in(const sv_fe& a, bool mont) {
  Fr x;
  memcpy(x.v, a.l, sizeof x.v);
  return mont ? x : fe_to_mont(x);
}

}  // namespace

size_t expressions_table_bytes(size_t n_ops) { return offsetof(ExprTable, ops) + (n_ops + 1) * sizeof(DevOp); }

int expressions_enqueue(const ExprCall& call, void* d_scratch, void* h_stage, hipStream_t st) {
  static_assert(sizeof(Fr) == sizeof(sv_fe), "Fr is the ABI's element");
  const bool mont = call.form == SV_MONTGOMERY;
  const uint32_t K = call.log_n + call.log_ext;
  const ExprPlan& plan = *call.plan;
  if (call.n_ops == 0 || call.n_ops > SV_EXPR_OPS_MAX || call.n_cols > SV_EXPR_COLUMNS_MAX ||
      call.n_consts > SV_EXPR_CONSTS_MAX || call.n_stores > SV_EXPR_STORES_MAX || K > SV_NTT_MAX_LOG ||
      call.log_ext > SV_EXT_LOG_MAX || plan.depth > SV_EXPR_STACK_MAX) {
    set_error("expressions: %zu ops, %zu columns, %zu constants, %zu stores, K = %u, log_ext = %u out of range",
              call.n_ops, call.n_cols, call.n_consts, call.n_stores, K, call.log_ext);
    return SV_ERR_LEN;
  }
  ExprTable* h = static_cast<ExprTable*>(h_stage);
  memset(h, 0, offsetof(ExprTable, ops));
  // what the program never names stays null (zero): it is never dereferenced
  for (size_t j = 0; j < call.n_cols; j++)
    if (plan.col_used[j]) h->cols[j] = static_cast<const uint4*>(static_cast<const void*>(call.d_cols[j]));
  for (size_t j = 0; j < call.n_stores; j++)
    if (plan.store_used[j]) h->stores[j] = static_cast<uint4*>(static_cast<void*>(call.d_stores[j]));
  for (size_t j = 0; j < call.n_consts; j++)
    if (plan.const_used[j]) h->consts[j] = fr_in(call.consts[j], mont);
  if (plan.folds) h->y = fr_in(*call.y, mont);
  const int64_t E = int64_t(1) << call.log_ext, rows = int64_t(1) << K;
  for (size_t i = 0; i < call.n_ops; i++) {
    const sv_fr_expr_op& o = call.program[i];
    h->ops[i] = DevOp{(uint32_t)o.op | (uint32_t)o.index << 16, (uint32_t)(((int64_t)o.rotation * E) & (rows - 1))};
  }
  h->ops[call.n_ops] = DevOp{0, 0};
  const size_t bytes = expressions_table_bytes(call.n_ops);
  SV_HIP(hipMemcpyAsync(d_scratch, h, bytes, hipMemcpyHostToDevice, st));
  const ExprTable* d_tab = static_cast<const ExprTable*>(d_scratch);
  uint32_t* d_err = reinterpret_cast<uint32_t*>(static_cast<char*>(d_scratch) + kExprErrOffset);
  const uint4* acc_in = static_cast<const uint4*>(call.d_acc_in);
  uint4* out = static_cast<uint4*>(call.d_out);
  const dim3 grid((uint32_t)(((uint64_t)rows + kExprThreads - 1) / kExprThreads));
  const uint32_t n_ops = (uint32_t)call.n_ops, folds = plan.folds;
  if (mont) hipLaunchKernelGGL(k_expressions<true>, grid, dim3(kNT), 0, st, d_tab, d_err, acc_in, out, n_ops, K, folds);
  else hipLaunchKernelGGL(k_expressions<false>, grid, dim3(kNT), 0, st, d_tab, d_err, acc_in, out, n_ops, K, folds);
  SV_HIP(hipGetLastError());
  return SV_OK;
}

}  // namespace sv
