// The host plan of the batched lookup permutation (csrc/lp_batch_plan.hpp) against a naive quadratic
// restatement of the header's rules, over seeded random pointer sets: counts 0 .. 17, tables that
// alias, ranges that overlap by part of an element, abut or coincide, misaligned and null entries,
// null arrays, unknown flag bits and forms, n from 0 to one past the cap.  Every array is a heap block
// of exactly `count` entries, so a read past it is an AddressSanitizer report.  For every set: accept
// or reject and the rule that rejects; for an accepted one the number of table slots, every lookup's
// slot, and that the scratch regions are pairwise disjoint, 256-byte aligned and inside the total.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../../snark-verifier-axiom_amd/csrc/lp_batch_plan.hpp"

namespace {

using sv::LpBatchPlan;

struct Set {
  std::vector<uintptr_t> in, tab, oa, os;
  size_t count, n;
  int form;
  uint32_t flags;
  bool null_array[4];
};

bool hit(uintptr_t a, uintptr_t b, unsigned __int128 bytes) {  // [a, a + bytes) meets [b, b + bytes)
  const unsigned __int128 x = a, y = b;
  return x < y + bytes && y < x + bytes;
}

// the header's rules, one at a time, each over all the entries
int naive_rule(const Set& s) {
  if (s.form != 0 && s.form != 1) return 1;
  if (s.flags > 1) return 1;
  for (bool b : s.null_array)
    if (b) return 1;
  for (size_t j = 0; j < s.count; j++)
    for (uintptr_t p : {s.in[j], s.tab[j], s.oa[j], s.os[j]})
      if (p == 0) return 1;
  for (size_t j = 0; j < s.count; j++)
    for (uintptr_t p : {s.in[j], s.tab[j], s.oa[j], s.os[j]})
      if (p % 16 != 0) return 1;
  if (s.count == 0 || s.n == 0) return 2;
  if (s.count > 16 || s.n > (size_t(1) << 26)) return 3;
  std::vector<uintptr_t> outs, reads;
  for (size_t j = 0; j < s.count; j++) outs.push_back(s.oa[j]), outs.push_back(s.os[j]);
  for (size_t j = 0; j < s.count; j++) reads.push_back(s.in[j]), reads.push_back(s.tab[j]);
  const unsigned __int128 bytes = (unsigned __int128)s.n * 32;
  for (size_t a = 0; a < outs.size(); a++) {
    for (uintptr_t r : reads)
      if (hit(outs[a], r, bytes)) return 4;
    for (size_t b = 0; b < outs.size(); b++)
      if (a != b && hit(outs[a], outs[b], bytes)) return 4;
  }
  return 0;
}

struct Region {
  size_t at, bytes;
};

int fail(const char* what, unsigned long long iter) {
  std::printf("lp_batch_plan_check FAILED: %s (set %llu)\n", what, iter);
  return 1;
}

}  // namespace

int main() {
  std::mt19937_64 rng(0x6c705f6261746368ull);
  auto pick = [&rng](uint64_t m) { return (uint64_t)(rng() % m); };
  const size_t sizes[] = {0, 1, 1, 2, 3, 5, 64, 1023, 1024, 1025, 3071, size_t(1) << 26, (size_t(1) << 26) + 1};
  unsigned long long accepted = 0, by_rule[5] = {0, 0, 0, 0, 0}, shared = 0, presorted = 0;
  for (unsigned long long iter = 0; iter < 60000; iter++) {
    Set s{};
    s.count = pick(8) == 0 ? pick(18) : 1 + pick(4) + (pick(3) == 0 ? pick(13) : 0);
    s.n = sizes[pick(sizeof sizes / sizeof sizes[0])];
    const bool clean = pick(3) != 0;  // a set built to be accepted, or one with every kind of trouble
    s.form = clean || pick(12) ? (int)pick(2) : (int)pick(5) - 1;
    s.flags = clean || pick(12) ? (uint32_t)pick(2) : (uint32_t)pick(8);
    for (bool& b : s.null_array) b = !clean && pick(40) == 0;
    // cells of exactly one column, back to back: neighbours abut
    const uintptr_t base = 0x7000000000ull + 256 * pick(16);
    const size_t cell = (s.n ? s.n : 1) * 32;
    size_t next_cell = 0;
    auto fresh = [&]() { return base + cell * next_cell++; };
    auto trouble = [&](uintptr_t p) -> uintptr_t {
      if (clean) return p;
      switch (pick(30)) {
        case 0: return 0;
        case 1: return p + 8;
        case 2: return p + 1;
        case 3: return p + 16;                               // half an element into the next cell
        case 4: return p - 32;                               // one element in front
        case 5: return base + cell * pick(next_cell + 1);    // somebody's cell
        default: return p;
      }
    };
    std::vector<uintptr_t> tabs_seen;
    for (size_t j = 0; j < s.count; j++) {
      s.in.push_back(trouble(j && pick(5) == 0 ? s.in[pick(j)] : fresh()));
      uintptr_t t;
      if (j && pick(2)) t = s.tab[pick(j)];                                 // a shared table
      else if (j && pick(4) == 0 && s.n > 1) t = s.tab[pick(j)] + 32 * (1 + pick(s.n - 1));  // an overlapping one
      else t = fresh();
      if (t >= base + cell * next_cell - cell) next_cell = (t - base) / cell + 2;  // keep later cells off its range
      s.tab.push_back(trouble(t));
    }
    for (size_t j = 0; j < s.count; j++) s.oa.push_back(trouble(fresh()));
    for (size_t j = 0; j < s.count; j++) s.os.push_back(trouble(fresh()));

    // heap blocks of exactly count entries
    auto block = [&](const std::vector<uintptr_t>& v, bool null) -> std::unique_ptr<const void*[]> {
      if (null) return nullptr;
      std::unique_ptr<const void*[]> b(new const void*[v.size()]);
      for (size_t j = 0; j < v.size(); j++) b[j] = reinterpret_cast<const void*>(v[j]);
      return b;
    };
    auto in = block(s.in, s.null_array[0]), tab = block(s.tab, s.null_array[1]);
    auto oa = block(s.oa, s.null_array[2]), os = block(s.os, s.null_array[3]);
    const LpBatchPlan p = sv::lp_batch_plan(in.get(), tab.get(), s.count, s.n, s.form, s.flags,
                                            const_cast<void* const*>(reinterpret_cast<const void* const*>(oa.get())),
                                            const_cast<void* const*>(reinterpret_cast<const void* const*>(os.get())));
    const int want = naive_rule(s);
    if ((int)p.rule != want) {
      std::printf("plan says rule %d, the restatement %d\n", (int)p.rule, want);
      return fail("accept / reject", iter);
    }
    by_rule[want]++;
    if (want != 0) {
      if (!p.why || !p.why[0]) return fail("a refusal without a message", iter);
      continue;
    }
    accepted++;
    // slots: the distinct table pointers in order of first appearance
    size_t slots = 0;
    for (size_t j = 0; j < s.count; j++) {
      size_t first = j;
      for (size_t i = 0; i < j; i++)
        if (s.tab[i] == s.tab[j]) {
          first = i;
          break;
        }
      size_t before = 0;
      for (size_t i = 0; i < first; i++) {
        bool is_first = true;
        for (size_t k = 0; k < i; k++) is_first &= s.tab[k] != s.tab[i];
        before += is_first;
      }
      if (first == j) slots++;
      if (p.slot[j] != before) return fail("a lookup's slot", iter);
      if (reinterpret_cast<uintptr_t>(p.table[p.slot[j]]) != s.tab[j]) return fail("a slot's pointer", iter);
    }
    if (p.slots != slots || p.count != s.count) return fail("the number of slots", iter);
    shared += slots < s.count;
    const bool pre = s.flags & 1;
    presorted += pre;
    if (p.sorted_cols != s.count + (pre ? 0 : slots)) return fail("the sorted columns", iter);
    // regions
    const size_t nb = (s.n + 1023) / 1024, cols = s.count + slots;
    std::vector<Region> regions;
    regions.push_back({p.heads, s.count * 64});
    for (size_t c = 0; c < p.sorted_cols; c++) {
      regions.push_back({p.states + c * sv::kLpbStateBytes, sv::kLpbStateBytes});
      regions.push_back({p.counts + c * p.counts_stride, 256 * nb * 4});
    }
    for (size_t c = 0; c < cols; c++)
      for (uint32_t parity = 0; parity < (c < p.sorted_cols ? 2u : 1u); parity++)
        regions.push_back({p.images + sv::lpb_image_index(p, (uint32_t)c, parity) * p.image_stride, s.n * 32});
    for (size_t j = 0; j < s.count; j++) {
      for (size_t at : {p.repeat, p.used, p.rep_row, p.un_pos}) regions.push_back({at + j * p.flag_stride, s.n * 4});
      for (size_t at : {p.totals, p.carries}) regions.push_back({at + j * p.tot_stride, 2 * nb * 4});
    }
    if (p.heads != 0 || p.zeroed != p.states + p.sorted_cols * sv::kLpbStateBytes || p.zeroed > p.counts)
      return fail("the zeroed prefix is the heads and the states", iter);
    for (size_t a = 0; a < regions.size(); a++) {
      if (regions[a].at % 256) return fail("a region is not 256-byte aligned", iter);
      if (regions[a].at + regions[a].bytes > p.total) return fail("a region leaves the total", iter);
      for (size_t b = a + 1; b < regions.size(); b++)
        if (regions[a].at < regions[b].at + regions[b].bytes && regions[b].at < regions[a].at + regions[a].bytes)
          return fail("two regions overlap", iter);
    }
  }
  for (int r = 0; r < 5; r++)
    if (by_rule[r] < 500) return fail("a rule the random sets hardly reach", (unsigned long long)r);
  if (shared < 500 || presorted < 500) return fail("too few shared or presorted sets", 0);
  std::printf("lp_batch_plan_check ok: %llu accepted, refused by rule 1-4: %llu %llu %llu %llu\n", accepted, by_rule[1],
              by_rule[2], by_rule[3], by_rule[4]);
  return 0;
}
