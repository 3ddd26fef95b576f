// The walk over an expression program (csrc/expr_plan.hpp) on the CPU, built with the host compiler
// under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_expr_plan.py): seeded random op
// arrays -- raw random bytes, programs grown op by op so that most are accepted, and arrays one op
// short or long of every cap -- each in a heap block of exactly its size, so a read past n_ops or
// past the cap is a sanitizer report.  The walk must agree with the naive simulation below on accept
// or reject, on the deepest stack, the FOLD count and the tables' marks, and every hand-written
// rejection must come back with its fault and its op.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../snark-verifier-axiom_amd/csrc/expr_plan.hpp"

using namespace sv;

static uint64_t rng_state = 0x5EED0123456789ABull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Naive {
  bool ok;
  size_t depth, folds;
  std::vector<int> cols, consts, stores;
};

// The rules as the header states them, over a real stack of values that nobody reads.
static Naive naive(const ExprOp* ops, size_t n_ops, size_t n_cols, size_t n_consts, size_t n_stores, uint32_t log_n) {
  Naive r{false, 0, 0, std::vector<int>(256, 0), std::vector<int>(256, 0), std::vector<int>(16, 0)};
  if (n_ops > 4096) n_ops = 4096;
  if (n_cols > 256) n_cols = 256;
  if (n_consts > 256) n_consts = 256;
  if (n_stores > 16) n_stores = 16;
  const long long n = 1ll << log_n;
  std::vector<int> stack;
  size_t sinks = 0;
  for (size_t i = 0; i < n_ops; i++) {
    const ExprOp o = ops[i];
    if (o.op > 8 || o.zero) return r;
    const size_t limit = o.op == 0 ? n_cols : o.op == 1 ? n_consts : o.op == 8 ? n_stores : 1;
    if (o.index >= limit || o.rotation <= -n || o.rotation >= n || (o.op != 0 && o.rotation)) return r;
    const size_t pops = o.op <= 1 ? 0 : (o.op == 2 || o.op >= 7) ? 1 : 2;
    if (stack.size() < pops) return r;
    stack.resize(stack.size() - pops);
    if (o.op < 7) stack.push_back(0);
    if (stack.size() > 8) return r;
    if (stack.size() > r.depth) r.depth = stack.size();
    if (o.op == 0) r.cols[o.index] = 1;
    if (o.op == 1) r.consts[o.index] = 1;
    if (o.op == 7) r.folds++, sinks++;
    if (o.op == 8) {
      if (r.stores[o.index]) return r;
      r.stores[o.index] = 1, sinks++;
    }
  }
  r.ok = stack.empty() && sinks > 0;
  return r;
}

static long accepted = 0, rejected = 0;

// one program in a block of exactly its size (at most the cap: the walk may not look further)
static void compare(const std::vector<ExprOp>& prog, size_t claimed, size_t n_cols, size_t n_consts, size_t n_stores,
                    uint32_t log_n) {
  const size_t held = prog.size();
  ExprOp* ops = static_cast<ExprOp*>(malloc(held ? held * sizeof(ExprOp) : 1));
  if (held) memcpy(ops, prog.data(), held * sizeof(ExprOp));
  ExprPlan plan;
  size_t at = ~size_t(0);
  const ExprFault f = expr_walk(ops, claimed, n_cols, n_consts, n_stores, log_n, &plan, &at);
  const Naive want = naive(ops, claimed, n_cols, n_consts, n_stores, log_n);
  bool same = (f == kExprOk) == want.ok;
  if (same && want.ok) {
    same = plan.depth == want.depth && plan.folds == want.folds;
    for (size_t i = 0; i < 256; i++) same = same && plan.col_used[i] == want.cols[i] && plan.const_used[i] == want.consts[i];
    for (size_t i = 0; i < 16; i++) same = same && plan.store_used[i] == want.stores[i];
  }
  if (!same || at > (claimed < kExprOpsMax ? claimed : kExprOpsMax)) {
    printf("MISMATCH: %zu ops (%zu claimed), tables %zu %zu %zu, log_n %u: walk %d at %zu, naive %d\n", held, claimed,
           n_cols, n_consts, n_stores, log_n, (int)f, at, (int)want.ok);
    exit(1);
  }
  (f == kExprOk ? accepted : rejected)++;
  free(ops);
}

// an op that is legal at this depth, or (now and then) anything at all
static ExprOp grow(size_t depth, size_t n_cols, size_t n_consts, size_t n_stores, uint32_t log_n, bool wild) {
  ExprOp o{0, 0, 0, 0};
  if (wild) {
    const uint64_t bits = rnd();
    memcpy(&o, &bits, sizeof o);
    if (below(2)) o.op = (uint8_t)below(10);
    if (below(2)) o.zero = 0;
    return o;
  }
  uint32_t kind = below(depth >= 2 ? 9 : depth == 1 ? 5 : 2);  // 0 1 | 2 7 8 | 3 4 5 6
  static const uint8_t order[9] = {0, 1, 2, 7, 8, 3, 4, 5, 6};
  o.op = order[kind];
  if (depth >= 6 && below(2)) o.op = (uint8_t)(3 + below(4));
  const long long n = 1ll << log_n;
  if (o.op == 0) {
    o.index = (uint16_t)below((uint32_t)n_cols + (below(50) == 0 ? 2 : 0) + (n_cols ? 0 : 1));
    o.rotation = (int32_t)((long long)(rnd() % (uint64_t)(2 * n - 1)) - (n - 1));
    if (below(60) == 0) o.rotation = (int32_t)(below(2) ? n : -n);
  } else if (o.op == 1) {
    o.index = (uint16_t)below((uint32_t)n_consts + (below(50) == 0 ? 2 : 0) + (n_consts ? 0 : 1));
  } else if (o.op == 8) {
    o.index = (uint16_t)below((uint32_t)n_stores + (below(50) == 0 ? 2 : 0) + (n_stores ? 0 : 1));
  }
  return o;
}

static void expect(const std::vector<ExprOp>& prog, size_t n_cols, size_t n_consts, size_t n_stores, uint32_t log_n,
                   ExprFault want, size_t want_at) {
  ExprPlan plan;
  size_t at = ~size_t(0);
  const ExprFault f = expr_walk(prog.data(), prog.size(), n_cols, n_consts, n_stores, log_n, &plan, &at);
  if (f != want || at != want_at) {
    printf("hand-written case: fault %d at %zu, expected %d at %zu\n", (int)f, at, (int)want, want_at);
    exit(1);
  }
  compare(prog, prog.size(), n_cols, n_consts, n_stores, log_n);
}

int main() {
  // ---- every rejection of the walk, by hand (3 columns, 2 constants, 2 stores, n = 4) ----
  const ExprOp C{kExprConst, 0, 0, 0}, F{kExprFold, 0, 0, 0}, S0{kExprStore, 0, 0, 0}, COL{kExprColumn, 0, 2, -3};
  expect({COL, C, {kExprMul, 0, 0, 0}, F, C, S0}, 3, 2, 2, 2, kExprOk, 6);
  expect({{9, 0, 0, 0}}, 3, 2, 2, 2, kExprBadOpcode, 0);
  expect({C, {200, 0, 0, 0}}, 3, 2, 2, 2, kExprBadOpcode, 1);
  expect({C, {kExprFold, 1, 0, 0}}, 3, 2, 2, 2, kExprZeroField, 1);
  expect({{kExprColumn, 0, 3, 0}, F}, 3, 2, 2, 2, kExprBadIndex, 0);
  expect({{kExprConst, 0, 2, 0}, F}, 3, 2, 2, 2, kExprBadIndex, 0);
  expect({C, {kExprStore, 0, 2, 0}}, 3, 2, 2, 2, kExprBadIndex, 1);
  expect({C, {kExprNeg, 0, 1, 0}, F}, 3, 2, 2, 2, kExprBadIndex, 1);
  expect({{kExprColumn, 0, 0, 0}, F}, 0, 2, 2, 2, kExprBadIndex, 0);
  expect({{kExprColumn, 0, 0, 4}, F}, 3, 2, 2, 2, kExprRotationRange, 0);
  expect({{kExprColumn, 0, 0, -4}, F}, 3, 2, 2, 2, kExprRotationRange, 0);
  expect({{kExprColumn, 0, 0, INT32_MIN}, F}, 3, 2, 2, 26, kExprRotationRange, 0);
  expect({{kExprColumn, 0, 0, INT32_MAX}, F}, 3, 2, 2, 0, kExprRotationRange, 0);
  expect({{kExprColumn, 0, 0, 0}, F}, 3, 2, 2, 0, kExprOk, 2);
  expect({{kExprConst, 0, 0, 1}, F}, 3, 2, 2, 2, kExprRotationOnOther, 0);
  expect({C, {kExprFold, 0, 0, -1}}, 3, 2, 2, 2, kExprRotationOnOther, 1);
  expect({{kExprNeg, 0, 0, 0}}, 3, 2, 2, 2, kExprUnderflow, 0);
  expect({C, {kExprAdd, 0, 0, 0}}, 3, 2, 2, 2, kExprUnderflow, 1);
  expect({C, F, F}, 3, 2, 2, 2, kExprUnderflow, 2);
  expect({C, C, C, C, C, C, C, C, C}, 3, 2, 2, 2, kExprTooDeep, 8);
  expect({C, S0, C, S0}, 3, 2, 2, 2, kExprStoreTwice, 3);
  expect({C, C, F}, 3, 2, 2, 2, kExprStackLeft, 3);
  expect({C}, 3, 2, 2, 2, kExprStackLeft, 1);
  expect({}, 3, 2, 2, 2, kExprNoSink, 0);
  // an op's rules in their order
  expect({{9, 1, 9, 9}}, 3, 2, 2, 2, kExprBadOpcode, 0);
  expect({{kExprNeg, 1, 9, 9}}, 3, 2, 2, 2, kExprZeroField, 0);
  expect({{kExprNeg, 0, 9, 9}}, 3, 2, 2, 2, kExprBadIndex, 0);
  expect({{kExprNeg, 0, 0, 9}}, 3, 2, 2, 2, kExprRotationRange, 0);
  expect({{kExprNeg, 0, 0, 1}}, 3, 2, 2, 2, kExprRotationOnOther, 0);
  expect({C, S0, {kExprStore, 0, 0, 0}}, 3, 2, 2, 2, kExprUnderflow, 2);

  // ---- one op short or long of every cap ----
  for (size_t n : {kExprOpsMax - 1, kExprOpsMax, kExprOpsMax + 1, kExprOpsMax + 1000}) {
    // C F C F ..: accepted when the walk stops at an even count; the block holds min(n, cap) ops
    std::vector<ExprOp> prog;
    for (size_t i = 0; i < (n < kExprOpsMax ? n : kExprOpsMax); i++) prog.push_back(i % 2 ? F : C);
    compare(prog, n, 3, 2, 2, 2);
  }
  for (size_t cap_case = 0; cap_case < 3; cap_case++) {
    const size_t cap = cap_case == 0 ? kExprColumnsMax : cap_case == 1 ? kExprConstsMax : kExprStoresMax;
    const uint8_t op = cap_case == 0 ? kExprColumn : cap_case == 1 ? kExprConst : kExprStore;
    for (size_t count : {cap - 1, cap, cap + 1, cap + 70000})
      for (size_t index : {cap - 2, cap - 1, cap, cap + 1}) {
        std::vector<ExprOp> prog;
        if (op != kExprStore) prog = {{op, 0, (uint16_t)index, 0}, F};
        else prog = {C, {op, 0, (uint16_t)index, 0}};
        compare(prog, prog.size(), cap_case == 0 ? count : 3, cap_case == 1 ? count : 2, cap_case == 2 ? count : 2, 2);
      }
  }
  for (size_t deep : {(size_t)kExprStackMax - 1, (size_t)kExprStackMax, (size_t)kExprStackMax + 1}) {
    std::vector<ExprOp> prog(deep, C);
    for (size_t i = 1; i < deep; i++) prog.push_back({kExprAdd, 0, 0, 0});
    prog.push_back(F);
    compare(prog, prog.size(), 3, 2, 2, 2);
  }

  // ---- random bytes ----
  for (int it = 0; it < 100000; it++) {
    std::vector<ExprOp> prog(1 + below(24));
    for (auto& o : prog) {
      const uint64_t bits = rnd();
      memcpy(&o, &bits, sizeof o);
    }
    compare(prog, prog.size(), below(300), below(300), below(20), below(27));
  }
  // ---- programs grown op by op ----
  for (int it = 0; it < 300000; it++) {
    const size_t n_cols = below(8) ? 1 + below(12) : below(260), n_consts = below(8) ? 1 + below(6) : below(260);
    const size_t n_stores = below(18);
    const uint32_t log_n = below(5) ? below(6) : below(27);
    const bool clean = below(3) != 0;  // no wild ops at all: most of these are accepted
    std::vector<ExprOp> prog;
    size_t depth = 0;
    const size_t len = 1 + below(it % 100 == 0 ? 600 : 40);
    bool used[16] = {false};
    for (size_t i = 0; i < len; i++) {
      ExprOp o = grow(depth, n_cols, n_consts, n_stores, log_n, !clean && below(25) == 0);
      if (clean && o.op == kExprStore && (n_stores == 0 || used[o.index % 16])) o = F;
      if (o.op == kExprStore) used[o.index % 16] = true;
      prog.push_back(o);
      const uint32_t pops = expr_pops(o.op <= 8 ? o.op : 0), pushes = expr_pushes(o.op <= 8 ? o.op : 0);
      depth = depth >= pops ? depth - pops + pushes : 0;
      if (depth > 8) depth = 8;
    }
    while (clean && depth > 0) {  // drain what is left so that the end rules pass
      prog.push_back(F);
      depth--;
    }
    compare(prog, prog.size(), n_cols, n_consts, n_stores, log_n);
  }
  if (accepted < 50000 || rejected < 50000) {
    printf("the generator is lopsided: %ld accepted, %ld rejected\n", accepted, rejected);
    return 1;
  }
  printf("expr_plan_check ok: %ld programs accepted, %ld rejected\n", accepted, rejected);
  return 0;
}
