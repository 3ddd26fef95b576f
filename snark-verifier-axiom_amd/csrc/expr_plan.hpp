// The host side of an expression program (include/svgpu.h, sv_bn254_fr_expressions_device): the one
// walk over its flat postfix ops that validates them, finds the deepest operand stack and the number
// of FOLDs, and marks which columns, constants and stores the program names.  No HIP and no field
// code in here: api.cpp runs this text before any device work, and the CPU runs the same text over
// random bytes against a naive simulation (tests/native/expr_plan_check.cpp).
//
// The walk reads ops[0 .. n_ops) only, looks at no more than the caps allow whatever the counts say,
// and indexes a table only with an index it has compared with that table's count and cap.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sv {

// the ABI's sv_fr_expr_op and its numbers (api.cpp asserts that they agree with the header)
struct ExprOp {
  uint8_t op;
  uint8_t zero;
  uint16_t index;
  int32_t rotation;
};
static_assert(sizeof(ExprOp) == 8, "an op is 8 bytes");

enum : uint8_t {
  kExprColumn = 0,  // push cols[index] rotated
  kExprConst = 1,   // push consts[index]
  kExprNeg = 2,     // a   -> -a
  kExprAdd = 3,     // a b -> a + b
  kExprSub = 4,     // a b -> a - b
  kExprRsub = 5,    // a b -> b - a
  kExprMul = 6,     // a b -> a b
  kExprFold = 7,    // v   -> ; acc <- acc y + v
  kExprStore = 8,   // v   -> ; stores[index][j] = v
  kExprOpcodes = 9
};
constexpr size_t kExprOpsMax = 4096;     // SV_EXPR_OPS_MAX
constexpr size_t kExprColumnsMax = 256;  // SV_EXPR_COLUMNS_MAX
constexpr size_t kExprConstsMax = 256;   // SV_EXPR_CONSTS_MAX
constexpr size_t kExprStoresMax = 16;    // SV_EXPR_STORES_MAX
constexpr uint32_t kExprStackMax = 8;    // SV_EXPR_STACK_MAX

// Why a program is refused, in the order the walk tests an op; the last two after the last op.
enum ExprFault {
  kExprOk = 0,
  kExprBadOpcode,
  kExprZeroField,
  kExprBadIndex,
  kExprRotationRange,
  kExprRotationOnOther,
  kExprUnderflow,
  kExprTooDeep,
  kExprStoreTwice,
  kExprStackLeft,
  kExprNoSink
};

inline const char* expr_fault_text(ExprFault f) {
  switch (f) {
    case kExprOk: return "ok";
    case kExprBadOpcode: return "unknown opcode";
    case kExprZeroField: return "the zero field is not zero";
    case kExprBadIndex: return "index out of range for its table (0 for an op without one)";
    case kExprRotationRange: return "rotation outside -n < r < n";
    case kExprRotationOnOther: return "a rotation on an op that is not COLUMN";
    case kExprUnderflow: return "operand stack underflow";
    case kExprTooDeep: return "operand stack deeper than SV_EXPR_STACK_MAX";
    case kExprStoreTwice: return "a second STORE to one index";
    case kExprStackLeft: return "the operand stack is not empty at the end";
    case kExprNoSink: return "the program has neither FOLD nor STORE";
  }
  return "?";
}

struct ExprPlan {
  uint32_t depth;   // the deepest operand stack
  uint32_t folds;   // FOLD ops
  uint32_t stores;  // STORE ops
  uint32_t muls;    // MUL ops (the cost model's products per row, the folds' aside)
  uint8_t col_used[kExprColumnsMax];
  uint8_t const_used[kExprConstsMax];
  uint8_t store_used[kExprStoresMax];
};

// operands an opcode pops and pushes
inline uint32_t expr_pops(uint8_t op) {
  switch (op) {
    case kExprColumn:
    case kExprConst: return 0;
    case kExprNeg:
    case kExprFold:
    case kExprStore: return 1;
    default: return 2;
  }
}
inline uint32_t expr_pushes(uint8_t op) { return op == kExprFold || op == kExprStore ? 0u : 1u; }

// The walk.  Returns kExprOk with *plan filled, or the first fault with *at = the offending op (n_ops
// for the two end-of-program faults); *plan is then unspecified.  Counts above their caps are
// treated as the caps: the caller has refused them before (rule 5), the walk just never trusts them.
inline ExprFault expr_walk(const ExprOp* ops, size_t n_ops, size_t n_cols, size_t n_consts, size_t n_stores,
                           uint32_t log_n, ExprPlan* plan, size_t* at) {
  if (n_ops > kExprOpsMax) n_ops = kExprOpsMax;
  if (n_cols > kExprColumnsMax) n_cols = kExprColumnsMax;
  if (n_consts > kExprConstsMax) n_consts = kExprConstsMax;
  if (n_stores > kExprStoresMax) n_stores = kExprStoresMax;
  plan->depth = plan->folds = plan->stores = plan->muls = 0;
  for (size_t i = 0; i < kExprColumnsMax; i++) plan->col_used[i] = 0;
  for (size_t i = 0; i < kExprConstsMax; i++) plan->const_used[i] = 0;
  for (size_t i = 0; i < kExprStoresMax; i++) plan->store_used[i] = 0;
  const int64_t n = log_n < 62 ? int64_t(1) << log_n : int64_t(1) << 62;
  uint32_t depth = 0;
  for (size_t i = 0; i < n_ops; i++) {
    const ExprOp o = ops[i];
    *at = i;
    if (o.op >= kExprOpcodes) return kExprBadOpcode;
    if (o.zero != 0) return kExprZeroField;
    const size_t table = o.op == kExprColumn ? n_cols : o.op == kExprConst ? n_consts : o.op == kExprStore ? n_stores : 1;
    if (o.index >= table) return kExprBadIndex;
    if ((int64_t)o.rotation <= -n || (int64_t)o.rotation >= n) return kExprRotationRange;
    if (o.rotation != 0 && o.op != kExprColumn) return kExprRotationOnOther;
    if (depth < expr_pops(o.op)) return kExprUnderflow;
    depth = depth - expr_pops(o.op) + expr_pushes(o.op);
    if (depth > kExprStackMax) return kExprTooDeep;
    if (depth > plan->depth) plan->depth = depth;
    switch (o.op) {
      case kExprColumn: plan->col_used[o.index] = 1; break;
      case kExprConst: plan->const_used[o.index] = 1; break;
      case kExprMul: plan->muls++; break;
      case kExprFold: plan->folds++; break;
      case kExprStore:
        if (plan->store_used[o.index]) return kExprStoreTwice;
        plan->store_used[o.index] = 1;
        plan->stores++;
        break;
      default: break;
    }
  }
  *at = n_ops;
  if (depth != 0) return kExprStackLeft;
  if (plan->folds + plan->stores == 0) return kExprNoSink;
  return kExprOk;
}

}  // namespace sv
