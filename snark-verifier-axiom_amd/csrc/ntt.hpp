// Number-theoretic transforms over BN254 Fr on the device: forward, inverse and coset, natural
// order on both sides (see ntt.hip; the plan and every index map: ntt_plan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgpu.h"
#include "ntt_plan.hpp"

namespace sv {

// Widest digit a pass transforms (T): a transform of 2^k points takes ceil(k / T) launches.
// SVGPU_NTT_TILE_LOG = 1 .. kNttTileLog lowers it per call (a test switch: the multi-pass paths
// then run at tiny sizes).
constexpr uint32_t kNttTileLog = 10;
static_assert(kNttTileLog <= kNttBlockLog, "a tile fits the block's LDS image");
static_assert(kNttTileLog <= 13, "a tile's roots come from the hi table alone");

// omega_k = ROOT_OF_UNITY^(2^(28 - k)) in `form` (host only)
int fr_root_of_unity(uint32_t log_n, int form, sv_fe* out);

struct NttCall {
  const void* d_in;
  void* d_out;
  uint32_t log_n;
  size_t count;
  bool inverse;
  bool has_shift;  // a shift other than 1
  sv_fe shift;     // in `form`, below r, not zero
  int form;
  uint32_t tile_log;
};

// Device scratch of one call: the error flag (u32: an element not below r) at offset 0, the first
// pass's per-block flags from kNttHeadBytes, and -- with two or more passes -- one image of the
// data (count 2^log_n elements), which every pass but the last writes and every pass but the first
// reads, so that the input is only read and in place is as good as out of place.
constexpr size_t kNttErrOffset = 0, kNttHeadBytes = 256;
size_t ntt_scratch_bytes(uint32_t log_n, size_t count, uint32_t tile_log);

// Enqueues the passes and the flag fold on `st` (device index `device`, whose root tables are built
// on first use).  Nothing is synchronised: the caller reads the head of d_scratch after the stream
// has drained.
int ntt_enqueue(const NttCall& call, int device, void* d_scratch, hipStream_t st);

// ---- the extended-domain round trip (predicates: ext_plan.hpp) ----
// Coset LDE: `count` polynomials of 2^log_n coefficients, back to back, to 2^(log_n + log_ext)
// evaluations each on g omega_K^j.  Nothing beyond count 2^log_n elements of d_coeffs is read.
struct LdeCall {
  const void* d_coeffs;
  void* d_evals;
  uint32_t log_n, log_ext;
  size_t count;
  bool has_shift;
  sv_fe shift;
  int form;
  uint32_t tile_log;
};
// The scratch is the NTT's at K = log_n + log_ext (the error flag at kNttErrOffset).
size_t lde_scratch_bytes(uint32_t log_n, uint32_t log_ext, size_t count, uint32_t tile_log);
int lde_enqueue(const LdeCall& call, int device, void* d_scratch, hipStream_t st);

// Quotient: N(g omega_K^j) / t(g omega_K^j), interpolated, cut to pieces 2^log_n coefficients.
// Nothing outside [0, pieces 2^log_n) of d_out is written; d_out == d_numer is in place.
struct QuotCall {
  const void* d_numer;
  void* d_out;
  uint32_t log_n, log_ext;
  size_t pieces;
  sv_fe shift;  // in `form`, below r, g^(2^K) != 1
  int form;
  uint32_t tile_log;
};
// The scratch is the NTT's with the 1 / t table (2^log_ext elements) between the head and the
// flags; h_stage is quotient_stage_bytes of pinned host memory that stays valid until the stream
// has drained (the table's one small copy starts there).
size_t quotient_scratch_bytes(uint32_t log_n, uint32_t log_ext, uint32_t tile_log);
size_t quotient_stage_bytes(uint32_t log_ext);
int quotient_enqueue(const QuotCall& call, int device, void* d_scratch, void* h_stage, hipStream_t st);
// g^(2^log_size) == 1: t vanishes somewhere on the coset (host only, log_size squarings)
bool coset_meets_domain(const sv_fe& shift, int form, uint32_t log_size);

}  // namespace sv
