// Test-only device harness for csrc/field29.hpp and csrc/curve29.hpp: the device build of the
// 29-bit layer differs from the host build (fused float multiply-add in is_zero_mod_p_16p,
// v_mad_u64_u32 columns, the compiler's own scheduling of the carry chains), and the MSM, Poseidon
// and decider tests reach it only with the values random points produce.  tests/test_gpu_field29.py
// runs the cases of tests/f29_cases.py through it, one thread per case, one kernel per operation
// (f29_ops.hpp holds the dispatch, shared with the host harness field29check.cpp), and checks them
// against Python big integers.  Not part of libsvgpu.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "f29_ops.hpp"

template <int OP, class M>
__global__ void k_f29(const uint32_t* in, uint32_t* out, uint32_t* flags, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NI = f29t::n_in(OP) * f29t::SLOT, NO = f29t::n_out(OP) * f29t::SLOT;
  uint32_t a[NI], r[NO];
#pragma unroll
  for (int k = 0; k < NI; k++) a[k] = in[(size_t)i * NI + k];
  uint32_t flag = flags[i];
  f29t::run<OP, M>(a, r, flag);
#pragma unroll
  for (int k = 0; k < NO; k++) out[(size_t)i * NO + k] = r[k];
  flags[i] = flag;
}

// op: f29_ops.hpp's number; field: 0 = Fq, 1 = Fr.  in: n cases of n_in(op) slots, out: n cases of
// n_out(op) slots (9 x u32 each), flags: n words, read and written -- all host arrays.
// Returns 0 on success, the hipError_t otherwise.
extern "C" int f29_run(int op, int field, const void* in, void* out, void* flags, size_t n) {
  if (op < 0 || op >= f29t::OP_COUNT || field < 0 || field > 1 || (field == 1 && f29t::fq_only(op)) ||
      n > (1u << 24))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bi = n * f29t::n_in(op) * f29t::SLOT * 4, bo = n * f29t::n_out(op) * f29t::SLOT * 4, bf = n * 4;
  uint32_t *din = nullptr, *dout = nullptr, *dfl = nullptr;
  hipError_t e = hipMalloc(&din, bi);
  if (e == hipSuccess) e = hipMalloc(&dout, bo);
  if (e == hipSuccess) e = hipMalloc(&dfl, bf);
  if (e == hipSuccess) e = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dfl, flags, bf, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((n + 63) / 64)), blk(64);
    switch (op) {
#define CASE(OP)                                                                                        \
  case f29t::OP:                                                                                        \
    if (field == 0)                                                                                     \
      hipLaunchKernelGGL((k_f29<f29t::OP, sv::r29::FqM29>), grid, blk, 0, 0, din, dout, dfl, (uint32_t)n); \
    else                                                                                                \
      hipLaunchKernelGGL((k_f29<f29t::OP, sv::r29::FrM29>), grid, blk, 0, 0, din, dout, dfl, (uint32_t)n); \
    break;
      F29T_FOR_EACH_OP(CASE)
#undef CASE
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, dfl, bf, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(dfl);
  return (int)e;
}
