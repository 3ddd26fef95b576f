// The host side of a batched lookup permutation (include/svgpu.h,
// sv_bn254_fr_lookup_permute_batch_device): the argument rules 1-4 of that call in their order, the
// deduplication of the table pointers into table slots, the slot of every lookup, and the layout of
// the call's device scratch.  No HIP and no field code in here: api.cpp runs this text before any
// device work, and the CPU runs the same text over random pointer sets against a naive quadratic
// restatement (tests/native/lp_batch_plan_check.cpp).
//
// Nothing is dereferenced but the four host arrays, entries [0, count) of each; the device pointers
// in them are only compared as integers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sv {

constexpr size_t kLpbMax = 16;                    // SV_LOOKUP_BATCH_MAX
constexpr uint32_t kLpbTablesSorted = 1;          // SV_LOOKUP_TABLES_SORTED
constexpr size_t kLpbMaxRows = size_t(1) << 26;   // kLpMaxRows
constexpr size_t kLpbElem = 32;                   // sizeof(sv_fe)
constexpr size_t kLpbTile = 1024;                 // kLpTile
constexpr size_t kLpbHeadBytes = 64;              // kLpHeadBytes, one head per lookup
constexpr size_t kLpbStateBytes = 32 * 256 * 4 + 32 * 4 + 128;  // sizeof(LpState) of lookup_permute.hip
constexpr int kLpbCanonical = 0, kLpbMontgomery = 1;            // SV_CANONICAL, SV_MONTGOMERY

// Why a call is refused: the number of the header's rule, 0 = accepted.
enum LpbRule { kLpbOk = 0, kLpbRuleArg = 1, kLpbRuleEmpty = 2, kLpbRuleLen = 3, kLpbRuleOverlap = 4 };

// Columns of a call: the lookups' inputs are columns [0, count), the table slots columns [count,
// count + slots).  The first `sorted_cols` columns go through the radix sort (a state, a counts
// block and two images each); with kLpbTablesSorted the table slots come after them and have one
// image and nothing else.  Offsets are bytes from the start of the scratch, 256-byte aligned.
struct LpBatchPlan {
  LpbRule rule;
  const char* why;         // the message of a refusal
  uint32_t count, slots;   // lookups, distinct table pointers
  uint32_t sorted_cols;    // count + slots, or count with presorted tables
  uint8_t slot[kLpbMax];   // lookup j reads table slot slot[j]
  const void* table[kLpbMax];  // the pointer of every slot, in order of first use
  size_t heads;            // count heads of kLpbHeadBytes; always 0
  size_t states;           // sorted_cols states of kLpbStateBytes
  size_t zeroed;           // bytes from 0 that start at zero: the heads and the states
  size_t counts, counts_stride;  // per sorted column, 256 * nb u32
  size_t images, image_stride;   // 2 * sorted_cols images, then one per presorted slot
  size_t repeat, used, rep_row, un_pos, flag_stride;  // per lookup, n u32 each
  size_t totals, carries, tot_stride;                 // per lookup, 2 * nb u32 each
  size_t total;
};

constexpr size_t lpb_align(size_t v) { return (v + 255) & ~size_t(255); }

inline bool lpb_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < bytes : x - y < bytes;
}

// The image of column c's parity p (p = 0 for a presorted slot), in images.
inline size_t lpb_image_index(const LpBatchPlan& p, uint32_t c, uint32_t parity) {
  return c < p.sorted_cols ? 2 * (size_t)c + parity : 2 * (size_t)p.sorted_cols + (c - p.sorted_cols);
}

inline LpBatchPlan lp_batch_plan(const void* const* inputs, const void* const* tables, size_t count, size_t n, int form,
                                 uint32_t flags, void* const* out_inputs, void* const* out_tables) {
  LpBatchPlan p{};
  auto refuse = [&p](LpbRule r, const char* why) {
    p.rule = r, p.why = why;
    return p;
  };
  // 1
  if (form != kLpbCanonical && form != kLpbMontgomery) return refuse(kLpbRuleArg, "bad form");
  if (flags & ~kLpbTablesSorted) return refuse(kLpbRuleArg, "unknown flag bit");
  if (!inputs || !tables || !out_inputs || !out_tables) return refuse(kLpbRuleArg, "null pointer array");
  for (size_t j = 0; j < count; j++)
    if (!inputs[j] || !tables[j] || !out_inputs[j] || !out_tables[j]) return refuse(kLpbRuleArg, "null pointer in an array");
  for (size_t j = 0; j < count; j++)
    if (((uintptr_t)inputs[j] | (uintptr_t)tables[j] | (uintptr_t)out_inputs[j] | (uintptr_t)out_tables[j]) & 15u)
      return refuse(kLpbRuleArg, "the columns must be 16-byte aligned");
  // 2
  if (count == 0) return refuse(kLpbRuleEmpty, "the batch should not be empty");
  if (n == 0) return refuse(kLpbRuleEmpty, "the columns should not be empty");
  // 3
  if (count > kLpbMax) return refuse(kLpbRuleLen, "count exceeds SV_LOOKUP_BATCH_MAX");
  if (n > kLpbMaxRows) return refuse(kLpbRuleLen, "n exceeds the per-device limit 2^26");
  // 4: an output against every input, every table and every other output
  const size_t bytes = n * kLpbElem;
  for (size_t a = 0; a < 2 * count; a++) {
    const void* o = a < count ? out_inputs[a] : out_tables[a - count];
    for (size_t j = 0; j < count; j++)
      if (lpb_overlap(o, inputs[j], bytes) || lpb_overlap(o, tables[j], bytes))
        return refuse(kLpbRuleOverlap, "an output overlaps an input column or a table (they are only read)");
    for (size_t b = a + 1; b < 2 * count; b++)
      if (lpb_overlap(o, b < count ? out_inputs[b] : out_tables[b - count], bytes))
        return refuse(kLpbRuleOverlap, "an output overlaps another output");
  }

  p.count = (uint32_t)count;
  for (size_t j = 0; j < count; j++) {  // tables are one table iff their pointers are equal
    uint32_t s = 0;
    while (s < p.slots && p.table[s] != tables[j]) s++;
    if (s == p.slots) p.table[p.slots++] = tables[j];
    p.slot[j] = (uint8_t)s;
  }
  const bool presorted = (flags & kLpbTablesSorted) != 0;
  p.sorted_cols = p.count + (presorted ? 0u : p.slots);
  const size_t nb = (n + kLpbTile - 1) / kLpbTile;
  size_t at = 0;
  p.heads = at, at += lpb_align(count * kLpbHeadBytes);
  p.states = at, at += (size_t)p.sorted_cols * kLpbStateBytes;
  p.zeroed = at;
  p.counts_stride = lpb_align(256 * nb * sizeof(uint32_t));
  p.counts = at, at += p.sorted_cols * p.counts_stride;
  p.image_stride = lpb_align(bytes);
  p.images = at, at += (2 * (size_t)p.sorted_cols + (presorted ? p.slots : 0u)) * p.image_stride;
  p.flag_stride = lpb_align(n * sizeof(uint32_t));
  p.repeat = at, at += count * p.flag_stride;
  p.used = at, at += count * p.flag_stride;
  p.rep_row = at, at += count * p.flag_stride;
  p.un_pos = at, at += count * p.flag_stride;
  p.tot_stride = lpb_align(2 * nb * sizeof(uint32_t));
  p.totals = at, at += count * p.tot_stride;
  p.carries = at, at += count * p.tot_stride;
  p.total = at;
  return p;
}

}  // namespace sv
