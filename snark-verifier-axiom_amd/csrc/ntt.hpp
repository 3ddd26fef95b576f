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

}  // namespace sv
