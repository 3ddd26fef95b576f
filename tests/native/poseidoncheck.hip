// Test-only device harness for the stages of csrc/poseidon.hip's permutation, one stage per launch
// and one lane per case (tests/test_gpu_poseidon_stages.py checks them against Python integers):
//   8 x 32-bit form (field.hpp words, R = 2^256):
//     PC_POW5       pow5                                          1 word  -> 1 word
//     PC_ROW3       mds_row<3> (lazy) against one row             3 words -> 1 word
//     PC_FULL3      full_round<3>                                 3 words -> 3 words
//     PC_PARTIAL3   partial_round<3>                              3 words -> 3 words
//     PC_LAST3      full_round<3, false> without constants, then fe_canon2p
//                                                                 3 words -> 3 raw + 3 canonical
//     PC_ROW5       mds_row<5> against one row                    5 words -> 1 word
//     PC_PARTIAL5   partial_round<5>                              5 words -> 5 words
//     PC_LAST5      full_round<5, false> without constants, then fe_canon2p
//                                                                 5 words -> 5 raw + 5 canonical
//     PC_CANON      fe_canon2p                                    1 word  -> 1 word
//   9 x 29-bit form (field29.hpp limbs, R' = 2^261; a word is 9 limbs):
//     PC29_POW5     p29::pow5                                     1 word  -> 1 word
//     PC29_ROW      p29::row against one row                      3 words -> 1 word
//     PC29_FULL     p29::full                                     3 words -> 3 words
//     PC29_PARTIAL  p29::partial (one partial round, with its two csub<4>)
//                                                                 3 words -> 3 words
//     PC29_OUT      r29::to_r32                                   1 word  -> 8 x 32-bit words
//     PC29_IN       r29::to_r29                                   8 x 32-bit words -> 1 word
// The stage's constants are chosen by `sel`:
//   rows    sel = mat | index << 8: mat 0 the dense MDS, 1 the pre-sparse matrix (index = row),
//           mat 2 the sparse matrix of partial round `index` (its `row`);
//   full    sel = kind | r << 8: kind 0 round r of the first half (constants start[r], 1 <= r < R_F / 2,
//           the dense MDS), kind 1 the last round of the first half (start[R_F / 2], the pre-sparse
//           matrix), kind 2 round r of the second half (end[r], r < R_F / 2 - 1, the dense MDS);
//   partial sel = the round.
// Inputs and outputs are raw limbs: nothing is reduced or canonicalised on the way in or out, so a
// case may hold any value the stage's contract allows.  sel is validated on the host and uniform
// over the launch; every index comes from it and the lane number, nothing is addressed by data.
// pc_stage returns 0, or the hipError_t (hipErrorInvalidValue for a malformed call).  Not part of
// libsvgpu.
#include "../../snark-verifier-axiom_amd/csrc/poseidon.hip"

#include <cstdint>

using namespace sv;

namespace {

enum {
  PC_POW5 = 0, PC_ROW3, PC_FULL3, PC_PARTIAL3, PC_LAST3, PC_ROW5, PC_PARTIAL5, PC_LAST5, PC_CANON,
  PC29_POW5, PC29_ROW, PC29_FULL, PC29_PARTIAL, PC29_OUT, PC29_IN, PC_STAGES
};

struct Shape {
  int in, out;  // u32 per case
};
__host__ __device__ constexpr Shape shape(int stage) {
  switch (stage) {
    case PC_POW5: return {8, 8};
    case PC_ROW3: return {24, 8};
    case PC_FULL3: return {24, 24};
    case PC_PARTIAL3: return {24, 24};
    case PC_LAST3: return {24, 48};
    case PC_ROW5: return {40, 8};
    case PC_PARTIAL5: return {40, 40};
    case PC_LAST5: return {40, 80};
    case PC_CANON: return {8, 8};
    case PC29_POW5: return {9, 9};
    case PC29_ROW: return {27, 9};
    case PC29_FULL: return {27, 27};
    case PC29_PARTIAL: return {27, 27};
    case PC29_OUT: return {9, 8};
    case PC29_IN: return {8, 9};
    default: return {0, 0};
  }
}

template <int T>
__device__ __forceinline__ void ld_state(Fr (&s)[T], const uint32_t* p) {
#pragma unroll
  for (int k = 0; k < T; k++)
#pragma unroll
    for (int j = 0; j < 8; j++) s[k].v[j] = p[8 * k + j];
}
template <int T>
__device__ __forceinline__ void st_state(const Fr (&s)[T], uint32_t* p) {
#pragma unroll
  for (int k = 0; k < T; k++)
#pragma unroll
    for (int j = 0; j < 8; j++) p[8 * k + j] = s[k].v[j];
}
__device__ __forceinline__ p29::E ld29(const uint32_t* p) {
  p29::E r;
#pragma unroll
  for (int i = 0; i < r29::L; i++) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void st29(const p29::E& a, uint32_t* p) {
#pragma unroll
  for (int i = 0; i < r29::L; i++) p[i] = a.v[i];
}

// the row of the 8 x 32-bit tables that `sel` names (T * 8 words per dense row, (2 T - 1) * 8 per sparse matrix)
template <int T>
__device__ __forceinline__ const uint32_t* row32(int sel) {
  const int mat = sel & 0xff, idx = sel >> 8;
  if (mat == 0) return PSpec<T>::mds() + idx * T * 8;
  if (mat == 1) return PSpec<T>::pre() + idx * T * 8;
  return PSpec<T>::sparse() + idx * (2 * T - 1) * 8;
}

template <int T>
__device__ __forceinline__ void last32(Fr (&s)[T], uint32_t* o) {
  full_round<T, false>(s, nullptr, PSpec<T>::mds());
  st_state<T>(s, o);
#pragma unroll
  for (int i = 0; i < T; i++) s[i] = fe_canon2p(s[i]);
  st_state<T>(s, o + 8 * T);
}

__global__ void __launch_bounds__(256) k_pc_stage(int stage, int sel, const uint32_t* __restrict__ in,
                                                  uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Shape sh = shape(stage);
  const uint32_t* p = in + (size_t)i * sh.in;
  uint32_t* o = out + (size_t)i * sh.out;
  constexpr int H = SV_POSEIDON_T3_RF / 2;
  switch (stage) {  // launch-uniform
    case PC_POW5: {
      Fr s[1];
      ld_state<1>(s, p);
      s[0] = pow5(s[0]);
      st_state<1>(s, o);
      break;
    }
    case PC_ROW3: {
      Fr s[3], r[1];
      ld_state<3>(s, p);
      r[0] = mds_row<3>(s, row32<3>(sel));
      st_state<1>(r, o);
      break;
    }
    case PC_FULL3: {
      Fr s[3];
      ld_state<3>(s, p);
      const int kind = sel & 0xff, r = sel >> 8;
      if (kind == 0) full_round<3>(s, c_start3 + r * 24, c_mds3);
      else if (kind == 1) full_round<3>(s, c_start3 + H * 24, c_pre3);
      else full_round<3>(s, c_end3 + r * 24, c_mds3);
      st_state<3>(s, o);
      break;
    }
    case PC_PARTIAL3: {
      Fr s[3];
      ld_state<3>(s, p);
      partial_round<3>(s, sel);
      st_state<3>(s, o);
      break;
    }
    case PC_LAST3: {
      Fr s[3];
      ld_state<3>(s, p);
      last32<3>(s, o);
      break;
    }
    case PC_ROW5: {
      Fr s[5], r[1];
      ld_state<5>(s, p);
      r[0] = mds_row<5>(s, row32<5>(sel));
      st_state<1>(r, o);
      break;
    }
    case PC_PARTIAL5: {
      Fr s[5];
      ld_state<5>(s, p);
      partial_round<5>(s, sel);
      st_state<5>(s, o);
      break;
    }
    case PC_LAST5: {
      Fr s[5];
      ld_state<5>(s, p);
      last32<5>(s, o);
      break;
    }
    case PC_CANON: {
      Fr s[1];
      ld_state<1>(s, p);
      s[0] = fe_canon2p(s[0]);
      st_state<1>(s, o);
      break;
    }
    case PC29_POW5: st29(p29::pow5(ld29(p)), o); break;
    case PC29_ROW: {
      const int mat = sel & 0xff, idx = sel >> 8;
      const uint32_t* m = mat == 0 ? c_mds3_29 + idx * 27 : mat == 1 ? c_pre3_29 + idx * 27 : c_sparse3_29 + idx * 45;
      st29(p29::row(ld29(p), ld29(p + 9), ld29(p + 18), m), o);
      break;
    }
    case PC29_FULL: {
      p29::E a = ld29(p), b = ld29(p + 9), c = ld29(p + 18);
      const int kind = sel & 0xff, r = sel >> 8;
      if (kind == 0) p29::full(a, b, c, c_start3_29 + r * 27, c_mds3_29);
      else if (kind == 1) p29::full(a, b, c, c_start3_29 + H * 27, c_pre3_29);
      else p29::full(a, b, c, c_end3_29 + r * 27, c_mds3_29);
      st29(a, o), st29(b, o + 9), st29(c, o + 18);
      break;
    }
    case PC29_PARTIAL: {
      p29::E a = ld29(p), b = ld29(p + 9), c = ld29(p + 18);
      p29::partial(a, b, c, sel);
      st29(a, o), st29(b, o + 9), st29(c, o + 18);
      break;
    }
    case PC29_OUT: r29::to_r32(ld29(p), o); break;
    default: st29(r29::to_r29<r29::FrM29>(p), o); break;  // PC29_IN
  }
}

bool sel_ok(int stage, int sel) {
  constexpr int H = SV_POSEIDON_T3_RF / 2;
  const int lo = sel & 0xff, hi = sel >> 8;
  if (sel < 0) return false;
  switch (stage) {
    case PC_ROW3:
    case PC29_ROW: return lo <= 1 ? hi < 3 : (lo == 2 && hi < SV_POSEIDON_T3_RP);
    case PC_ROW5: return lo <= 1 ? hi < 5 : (lo == 2 && hi < SV_POSEIDON_T5_RP);
    case PC_FULL3:
    case PC29_FULL: return lo == 0 ? (hi >= 1 && hi < H) : lo == 1 ? hi == 0 : (lo == 2 && hi < H - 1);
    case PC_PARTIAL3:
    case PC29_PARTIAL: return sel < SV_POSEIDON_T3_RP;
    case PC_PARTIAL5: return sel < SV_POSEIDON_T5_RP;
    default: return sel == 0;
  }
}

}  // namespace

// u32 per case on the way in (which = 0) and out (which = 1) of `stage`; -1 for an unknown stage
extern "C" int pc_words(int stage, int which) {
  if (stage < 0 || stage >= PC_STAGES) return -1;
  return which ? shape(stage).out : shape(stage).in;
}

// in: n cases of pc_words(stage, 0) u32; out: n cases of pc_words(stage, 1) u32
extern "C" int pc_stage(int stage, int sel, const void* in, void* out, size_t n) {
  if (stage < 0 || stage >= PC_STAGES || !sel_ok(stage, sel) || n > (1u << 20) || !in || !out)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const Shape sh = shape(stage);
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, n * sh.in * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, n * sh.out * 4);
  if (e == hipSuccess) e = hipMemcpy(din, in, n * sh.in * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, n * sh.out * 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_pc_stage, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, stage, sel, din, dout, (uint32_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, n * sh.out * 4, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}
