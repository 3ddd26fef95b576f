// Test harness (not part of libsvgpu): one dispatch over every operation of csrc/field29.hpp and
// csrc/curve29.hpp, shared by the host build (field29check.cpp, "cases" mode) and the device build
// (field29dev.hip), so both run the same calls on the cases of tests/f29_cases.py.
//
// A case is n_in(op) input slots and n_out(op) output slots of 9 x u32 each, plus one flag word.
// A slot holds 9 x 29-bit limbs, or 8 x 32-bit words and a zero where the operation takes or
// gives words (from_words / to_r29 in, to_words / to_r32 out).  The flag carries the sign in
// (bit 0: sub_sgn, madd, maddl) and a result out (is_zero16: the answer; maddl: `special`).
// The numbers below are the `id`s of tests/f29_cases.py's OPS table.
#pragma once
#include <cstdint>
#include <type_traits>

#include "curve29.hpp"

namespace f29t {
using namespace sv::r29;

enum Op {
  OP_MUL = 0, OP_MUL_ILP, OP_SQR, OP_MUL_SUM2, OP_MUL_SUM3, OP_MUL_SUB8, OP_SQR_SUB2C6, OP_ADD, OP_SUB2, OP_SUB4,
  OP_SUB8, OP_SUB_2C6, OP_SUB_SGN4, OP_CSUB1, OP_CSUB2, OP_CSUB4, OP_CSUB8, OP_FROM_WORDS, OP_TO_WORDS, OP_TO_R29,
  OP_TO_R32, OP_IS_ZERO16, OP_MADD, OP_MADDL, OP_XADD, OP_XADD8, OP_COUNT
};
constexpr int SLOT = 9;
constexpr int MAX_IN = 8, MAX_OUT = 4;

SV29_HD constexpr int n_in(int op) {
  constexpr int N[OP_COUNT] = {2, 2, 1, 4, 6, 3, 3, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 6, 6, 8, 8};
  return N[op];
}
SV29_HD constexpr int n_out(int op) { return op >= OP_MADD ? 4 : 1; }
// the curve operations and is_zero_mod_p_16p exist over Fq only
SV29_HD constexpr bool fq_only(int op) { return op >= OP_IS_ZERO16; }

template <class M>
SV29_HD F29<M> ld(const uint32_t* in, int slot) {
  F29<M> r;
#pragma unroll
  for (int i = 0; i < L; i++) r.v[i] = in[SLOT * slot + i];
  return r;
}
template <class M>
SV29_HD void st(uint32_t* out, int slot, const F29<M>& a) {
#pragma unroll
  for (int i = 0; i < L; i++) out[SLOT * slot + i] = a.v[i];
}
SV29_HD void st_words(uint32_t* out, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = w[i];
  out[8] = 0;
}
SV29_HD Xyzz ld_pt(const uint32_t* in, int slot) {
  return {ld<FqM29>(in, slot), ld<FqM29>(in, slot + 1), ld<FqM29>(in, slot + 2), ld<FqM29>(in, slot + 3)};
}
SV29_HD void st_pt(uint32_t* out, const Xyzz& p) { st(out, 0, p.X), st(out, 1, p.Y), st(out, 2, p.ZZ), st(out, 3, p.ZZZ); }

template <int OP, class M>
SV29_HD void run(const uint32_t* in, uint32_t* out, uint32_t& flag) {
  const bool neg = flag & 1;
  if constexpr (OP == OP_MUL) st(out, 0, mul(ld<M>(in, 0), ld<M>(in, 1)));
  else if constexpr (OP == OP_MUL_ILP) st(out, 0, mul_ilp(ld<M>(in, 0), ld<M>(in, 1)));
  else if constexpr (OP == OP_SQR) st(out, 0, sqr(ld<M>(in, 0)));
  else if constexpr (OP == OP_MUL_SUM2) st(out, 0, mul_sum2(ld<M>(in, 0), ld<M>(in, 1), ld<M>(in, 2), ld<M>(in, 3)));
  else if constexpr (OP == OP_MUL_SUM3)
    st(out, 0, mul_sum3(ld<M>(in, 0), ld<M>(in, 1), ld<M>(in, 2), ld<M>(in, 3), ld<M>(in, 4), ld<M>(in, 5)));
  else if constexpr (OP == OP_MUL_SUB8) st(out, 0, mul_sub<8>(ld<M>(in, 0), ld<M>(in, 1), ld<M>(in, 2)));
  else if constexpr (OP == OP_SQR_SUB2C6) st(out, 0, sqr_sub2c<6>(ld<M>(in, 0), ld<M>(in, 1), ld<M>(in, 2)));
  else if constexpr (OP == OP_ADD) st(out, 0, add(ld<M>(in, 0), ld<M>(in, 1)));
  else if constexpr (OP == OP_SUB2) st(out, 0, sub<2>(ld<M>(in, 0), ld<M>(in, 1)));
  else if constexpr (OP == OP_SUB4) st(out, 0, sub<4>(ld<M>(in, 0), ld<M>(in, 1)));
  else if constexpr (OP == OP_SUB8) st(out, 0, sub<8>(ld<M>(in, 0), ld<M>(in, 1)));
  else if constexpr (OP == OP_SUB_2C6) st(out, 0, sub_2c<6>(ld<M>(in, 0), ld<M>(in, 1), ld<M>(in, 2)));
  else if constexpr (OP == OP_SUB_SGN4) st(out, 0, sub_sgn<4>(ld<M>(in, 0), neg, ld<M>(in, 1)));
  else if constexpr (OP == OP_CSUB1) st(out, 0, csub<1>(ld<M>(in, 0)));
  else if constexpr (OP == OP_CSUB2) st(out, 0, csub<2>(ld<M>(in, 0)));
  else if constexpr (OP == OP_CSUB4) st(out, 0, csub<4>(ld<M>(in, 0)));
  else if constexpr (OP == OP_CSUB8) st(out, 0, csub<8>(ld<M>(in, 0)));
  else if constexpr (OP == OP_FROM_WORDS) st(out, 0, from_words<M>(in));
  else if constexpr (OP == OP_TO_WORDS) {
    uint32_t w[8];
    to_words(ld<M>(in, 0), w);
    st_words(out, w);
  } else if constexpr (OP == OP_TO_R29) st(out, 0, to_r29<M>(in));
  else if constexpr (OP == OP_TO_R32) {
    uint32_t w[8];
    to_r32(ld<M>(in, 0), w);
    st_words(out, w);
  } else if constexpr (std::is_same<M, FqM29>::value) {
    if constexpr (OP == OP_IS_ZERO16) {
      flag = is_zero_mod_p_16p(ld<M>(in, 0)) ? 1 : 0;
      st(out, 0, zero<M>());
    } else if constexpr (OP == OP_MADD) {
      st_pt(out, madd(ld_pt(in, 0), ld<M>(in, 4), ld<M>(in, 5), neg));
    } else if constexpr (OP == OP_MADDL) {
      // the loop's triple, as k_accumulate runs it: an identity state takes start; madd_live's
      // doubling is replaced by dbl_start, its cancellation zeroes ZZ (the chain is marked empty
      // and a stored empty chain reads as the identity by ZZ == 0)
      const Xyzz s = ld_pt(in, 0);
      const F x2 = ld<M>(in, 4), y2 = ld<M>(in, 5);
      int special = 0;
      Xyzz r;
      if (is_identity(s)) {
        r = start(x2, y2, neg);
      } else {
        r = madd_live(s, x2, y2, neg, special);
        if (special == 2) r = dbl_start(x2, y2, neg);
        else if (special == 1) r.ZZ = zero();
      }
      flag = (uint32_t)special;
      st_pt(out, r);
    } else if constexpr (OP == OP_XADD) {
      st_pt(out, sv::r29::add(ld_pt(in, 0), ld_pt(in, 4)));
    } else if constexpr (OP == OP_XADD8) {
      st_pt(out, sv::r29::add_x8(ld_pt(in, 0), ld_pt(in, 4)));
    }
  }
}

// F(op) for every operation, for a switch over a run-time op
#define F29T_FOR_EACH_OP(F)                                                                                         \
  F(OP_MUL) F(OP_MUL_ILP) F(OP_SQR) F(OP_MUL_SUM2) F(OP_MUL_SUM3) F(OP_MUL_SUB8) F(OP_SQR_SUB2C6) F(OP_ADD)         \
  F(OP_SUB2) F(OP_SUB4) F(OP_SUB8) F(OP_SUB_2C6) F(OP_SUB_SGN4) F(OP_CSUB1) F(OP_CSUB2) F(OP_CSUB4) F(OP_CSUB8)     \
  F(OP_FROM_WORDS) F(OP_TO_WORDS) F(OP_TO_R29) F(OP_TO_R32) F(OP_IS_ZERO16) F(OP_MADD) F(OP_MADDL) F(OP_XADD) F(OP_XADD8)

}  // namespace f29t
