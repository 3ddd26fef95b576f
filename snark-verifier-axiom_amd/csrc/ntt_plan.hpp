// The plan of an Fr NTT of 2^k points: the pass widths for a tile log T, and every index map and
// twiddle exponent the kernels of ntt.hip use.  No HIP and no field arithmetic in here: the CPU runs
// the very same decomposition over a toy field (tests/native/ntt_plan_check.cpp).
//
// Decimation in frequency over digits.  The k index bits are cut into P = ceil(k / T) digits of
// widths w_0 .. w_{P-1} (balanced: they differ by at most one), digit 0 at the TOP of the input
// index.  Pass s owns digit s: with L_s = k - (w_0 + .. + w_s) bits below it and H_s = w_0 + .. +
// w_{s-1} bits above it, an input index is  i = hi 2^(w+L) + m 2^L + lo.  The pass runs the
// 2^w-point DFT over m for every (hi, lo) -- one COLUMN, numbered col = hi 2^L + lo -- and leaves
// the frequency digit f where m was.  Digit f_s carries the weight 2^(H_s) in the output index
// j = sum_s f_s 2^(H_s), and
//     i j = sum_s [ m_s f_s 2^(k - w_s)  +  (f_s 2^(H_s)) (i mod 2^(L_s)) ]   (mod 2^k):
// the first term is the tile's own DFT (root omega_n^(2^(k - w))), the second the twiddle a pass
// applies on the way out, whose exponent needs only f, H and the column's lo bits -- no digit
// reversal.  Passes 0 .. P-2 write where they read (src index == dst index); the LAST pass (L = 0:
// its tiles are contiguous rows) folds the digit reversal into its store: destination column d
// (the low k - w bits of j, contiguous across neighbouring columns) is fed from the row whose digits
// are d's in reverse order.  So neighbouring columns are neighbouring addresses on the side that is
// strided, in every pass.
#pragma once
#include <cstdint>

#ifndef SV_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define SV_HD __host__ __device__ __forceinline__
#define SV_NOINL __host__ __device__ inline __attribute__((noinline))
#else
#define SV_HD inline
#define SV_NOINL inline
#endif
#endif

namespace sv {

constexpr uint32_t kNttMaxLog = 26;     // SV_NTT_MAX_LOG
constexpr uint32_t kNttBlockLog = 11;   // elements a block holds in LDS: 2^11 x 32 B = 64 KiB
constexpr uint32_t kNttThreadsLog = 9;  // threads per block
constexpr uint32_t kNttBlockColsMaxLog = 7;  // columns per block: a thread's 16-B units stay in one column

struct NttPlan {
  uint8_t k, passes;
  uint8_t width[kNttMaxLog];
};

// widths for (k, T): ceil(k / T) passes, the first k mod P one wider than the rest
SV_HD NttPlan ntt_make_plan(uint32_t k, uint32_t tile_log) {
  NttPlan p;
  const uint32_t P = (k + tile_log - 1) / tile_log;
  p.k = (uint8_t)k;
  p.passes = (uint8_t)P;
  for (uint32_t s = 0; s < kNttMaxLog; s++) p.width[s] = 0;
  for (uint32_t s = 0; s < P; s++) p.width[s] = (uint8_t)(k / P + (s < k % P ? 1 : 0));
  return p;
}

// k = 0 has no pass in the plan and still takes one launch (the checked copy): a pass of width 0
SV_HD uint32_t ntt_launches(const NttPlan& p) { return p.passes ? p.passes : 1; }
SV_HD uint32_t ntt_width(const NttPlan& p, uint32_t s) { return s < p.passes ? p.width[s] : 0; }
SV_HD uint32_t ntt_hi_bits(const NttPlan& p, uint32_t s) {  // H_s
  uint32_t h = 0;
  for (uint32_t q = 0; q < s && q < p.passes; q++) h += p.width[q];
  return h;
}
SV_HD uint32_t ntt_lo_bits(const NttPlan& p, uint32_t s) { return p.k - ntt_hi_bits(p, s) - ntt_width(p, s); }  // L_s
SV_HD bool ntt_is_last(const NttPlan& p, uint32_t s) { return s + 1 >= ntt_launches(p); }
SV_HD uint32_t ntt_cols_log(const NttPlan& p, uint32_t s) { return p.k - ntt_width(p, s); }  // columns per transform

// columns a block takes (log2): as many as fill the block's LDS, up to the cap
SV_HD uint32_t ntt_block_cols_log(const NttPlan& p, uint32_t s) {
  const uint32_t c = kNttBlockLog - ntt_width(p, s);
  return c < kNttBlockColsMaxLog ? c : kNttBlockColsMaxLog;
}

// Element index (inside its transform) of tile entry 0 of column `col` on the load side, and the
// log2 of the stride between tile entries.
SV_HD uint32_t ntt_src_base(const NttPlan& p, uint32_t s, uint32_t col) {
  const uint32_t w = ntt_width(p, s);
  if (!ntt_is_last(p, s)) {
    const uint32_t L = ntt_lo_bits(p, s);
    return ((col >> L) << (w + L)) | (col & ((1u << L) - 1u));
  }
  // last pass: col = sum_{q < s} f_q 2^(H_q); its row holds f_q at bit L_q of the index
  uint32_t idx = 0, H = 0;
  for (uint32_t q = 0; q < s; q++) {
    const uint32_t wq = p.width[q];
    const uint32_t f = (col >> H) & ((1u << wq) - 1u);
    H += wq;
    idx |= f << (p.k - H);  // L_q = k - H_{q+1}
  }
  return idx;
}
SV_HD uint32_t ntt_src_stride_log(const NttPlan& p, uint32_t s) { return ntt_is_last(p, s) ? 0 : ntt_lo_bits(p, s); }
// ... and on the store side
SV_HD uint32_t ntt_dst_base(const NttPlan& p, uint32_t s, uint32_t col) {
  return ntt_is_last(p, s) ? col : ntt_src_base(p, s, col);
}
SV_HD uint32_t ntt_dst_stride_log(const NttPlan& p, uint32_t s) {
  return ntt_is_last(p, s) ? ntt_cols_log(p, s) : ntt_lo_bits(p, s);
}

// Exponent of omega_n in the twiddle that pass s puts on frequency f of column col on the way out
// (below 2^k, so no reduction; 0 in the last pass, where lo = 0).
SV_HD uint32_t ntt_twiddle_exp(const NttPlan& p, uint32_t s, uint32_t col, uint32_t f) {
  const uint32_t L = ntt_lo_bits(p, s);
  return (f << ntt_hi_bits(p, s)) * (col & ((1u << L) - 1u));
}
// The same exponent for the root of order 2^root_log the tables hold (root_log >= k).
SV_HD uint32_t ntt_root_exp(const NttPlan& p, uint32_t e, uint32_t root_log) { return e << (root_log - p.k); }

// Radix-2 stage `st` (st = w-1 down to 0, span d = 2^st) of a tile: butterfly number b < 2^(w-1)
// pairs the entries m and m + d, and the difference takes omega_{2d}^j.
SV_HD void ntt_stage_pair(uint32_t b, uint32_t st, uint32_t* m, uint32_t* j) {
  *j = b & ((1u << st) - 1u);
  *m = ((b >> st) << (st + 1)) | *j;
}
// omega_{2d}^j as a power of the root of order 2^root_log
SV_HD uint32_t ntt_stage_exp(uint32_t j, uint32_t st, uint32_t root_log) { return j << (root_log - 1 - st); }
// the stages leave frequency f at tile entry bitrev_w(f)
SV_HD uint32_t ntt_bitrev(uint32_t f, uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return w ? __brev(f) >> (32 - w) : 0u;
#else
  uint32_t r = 0;
  for (uint32_t b = 0; b < w; b++) r |= ((f >> b) & 1u) << (w - 1 - b);
  return r;
#endif
}

// A block's 2^(w + c) elements, c = ntt_block_cols_log: element x is tile entry x >> c of the
// block's column x & (2^c - 1) -- columns fastest, so that a wave's 16-B lanes run along addresses.

}  // namespace sv
