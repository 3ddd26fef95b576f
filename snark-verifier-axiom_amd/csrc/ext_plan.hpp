// The extended-domain round trip on top of the NTT's plan (ntt_plan.hpp): which input indices of a
// coset LDE hold a coefficient, which destination indices of a truncated inverse are kept, and
// which entry of the 1 / t table an input index takes.  No HIP and no field arithmetic in here: the
// CPU runs the same predicates over a toy field (tests/native/extended_plan_check.cpp).
//
// LDE: a polynomial of n = 2^k coefficients goes through the plan of K = k + e as if it were padded
// with zeros to 2^K, without the padding ever existing: an input index i < 2^K is LIVE iff i < n.
// Only pass 0 loads input indices; its tile entry m carries the top digit of i, so in a column the
// live entries are a prefix, and in the first min(e, w_0) radix-2 stages the upper partner of every
// butterfly is a zero (sum = p, difference = p omega^j).
//
// Quotient: t(X) = X^n - 1 takes 2^e values on the coset g omega_K^i, t_i = g^n omega_e^(i mod 2^e)
// - 1, so the way-in factor of pass 0 is table[i mod 2^e].  With L_0 >= e every entry of a column
// shares i mod 2^e (the stride between entries is 2^(L_0)).  The last pass stores destination index
// d only if d < pieces n: what halo2's truncate drops is never written.
#pragma once
#include "ntt_plan.hpp"

namespace sv {

constexpr uint32_t kExtLogMax = 8;  // SV_EXT_LOG_MAX

// Index (inside its transform) of tile entry m of column col, on the load and on the store side.
SV_HD uint32_t ext_src_index(const NttPlan& p, uint32_t s, uint32_t col, uint32_t m) {
  return ntt_src_base(p, s, col) + (m << ntt_src_stride_log(p, s));
}
SV_HD uint32_t ext_dst_index(const NttPlan& p, uint32_t s, uint32_t col, uint32_t f) {
  return ntt_dst_base(p, s, col) + (f << ntt_dst_stride_log(p, s));
}

// live input index: one of the n = 2^log_n coefficients (the rest of the 2^K inputs are zeros that
// are never loaded)
SV_HD bool ext_live(uint32_t idx, uint32_t log_n) { return (idx >> log_n) == 0u; }
// a column of pass 0 with no live entry: entry 0 has the column's smallest index
SV_HD bool ext_col_dead(const NttPlan& p, uint32_t col, uint32_t log_n) {
  return !ext_live(ext_src_index(p, 0, col, 0), log_n);
}
// stages of pass 0 (from the top one down) in which a butterfly's upper partner is a known zero
SV_HD uint32_t ext_zero_stages(const NttPlan& p, uint32_t ext_log) {
  const uint32_t w = ntt_width(p, 0);
  return ext_log < w ? ext_log : w;
}
// In such a stage st (w - z <= st < w, z = ext_zero_stages) the lower partner, entry m, is a zero
// as well unless the bits of m between w - z and st are all clear (the stages above st have filled
// the bits above it): the butterfly then has nothing to do.
SV_HD bool ext_pair_dead(const NttPlan& p, uint32_t ext_log, uint32_t st, uint32_t m) {
  const uint32_t w = ntt_width(p, 0), z = ext_zero_stages(p, ext_log);
  if (st + z < w) return false;
  const uint32_t low = w - z;
  return ((m >> low) & ((1u << (st - low)) - 1u)) != 0u;
}

// kept destination index: below pieces * n
SV_HD bool ext_kept(uint32_t idx, uint64_t keep) { return idx < keep; }

// table index of input index idx, and of tile entry m of column col in pass 0
SV_HD uint32_t ext_table_of(uint32_t idx, uint32_t ext_log) { return idx & ((1u << ext_log) - 1u); }
SV_HD uint32_t ext_table_index(const NttPlan& p, uint32_t col, uint32_t m, uint32_t ext_log) {
  return ext_table_of(ext_src_index(p, 0, col, m), ext_log);
}
// every entry of a pass-0 column takes the same table entry
SV_HD bool ext_table_shared(const NttPlan& p, uint32_t ext_log) { return ntt_src_stride_log(p, 0) >= ext_log; }

}  // namespace sv
