// Host-side planning of the batched-MSM drivers (msm_batch.hip): the constants the kernels and the
// host share, the SVGPU_BATCH_* switches, the route of one call, the workspace layouts of the three
// drivers, the small / big partition of the host-array entry point and the fused-launch slot.  No
// HIP here: plain C++17, so the route table and the arithmetic that sizes every buffer can be built
// and checked on their own (tests/native/msm_batch_plan_check.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "msm_plan.hpp"  // MsmLayout, kSmallMsmTerms, the element sizes

namespace sv {

constexpr int kBatchThreads = 256;  // threads per block of the 256-thread batch kernels

// GLV (glv.hpp): every term k P is split into k1 P + k2 phi(P) with |k_i| < 2^127, so the windows
// cover 128 bits and the per-MSM Horner chain is ~128 doublings instead of ~255.
template <int C>
struct BatchCfg {
  static constexpr int W = (128 + C - 1) / C;  // signed digits of a < 2^127 half scalar
  static constexpr int B = 1 << (C - 1);
  static constexpr int G = B < 64 ? B : 64;  // lanes per window
  static constexpr int BPL = B / G;          // buckets per lane
  static constexpr int WPB = kBatchThreads / G;   // windows per block
  static constexpr int WG = (W + WPB - 1) / WPB;  // window groups (blockIdx.y)
  static constexpr int NCH = C <= 6 ? 128 : 256;
};

constexpr int kQC = 5;                       // window bits of the quad path
constexpr int kQB = 1 << (kQC - 1);          // 16 buckets: one quad each in a 64-lane wave
constexpr int kQW = BatchCfg<kQC>::W;        // 26 windows of a 128-bit GLV half
constexpr int kQMaxTerms = 256;              // half-terms of one window sorted in LDS at once
constexpr int kUPerWin = kQC;                // k_batch_uwin's partial sums per window: U_0 .. U_4

// The error word the kernels raise (atomicOr) and the drivers decode (batch_error, msm_batch.hip)
constexpr uint32_t kErrBase = 1;    // a base coordinate >= p
constexpr uint32_t kErrScalar = 2;  // a scalar >= r
constexpr uint32_t kErrIndex = 4;   // a base index past the table
constexpr uint32_t kErrWait = 8;    // a Horner wave of k_batch_fused gave up waiting: redone, never reported

// k_batch_fused runs only while the Horner waves (one per MSM) are a small fraction of the
// resident-wave capacity, so its bucket blocks always find slots and every wait ends
constexpr uint32_t kFuseMax = 512;
// bucket-wise Horner: 16 bucket sums per window instead of one window sum, 53 KB per MSM, so very
// large batches keep the per-window weighting of k_batch_windows_q
constexpr size_t kBucketHornerMax = 4096;
constexpr uint32_t kFuseBw = 4;             // bucket waves per MSM of a fused launch
constexpr uint32_t kFuseSpinMax = 1u << 22;  // sleeps a Horner wave waits for one window (~1 s)

// Small plain batches (round 5): the window sums on the device and one host Horner per MSM on the
// host pool (msm_batch_windows_host) instead of the fused kernel, whose one-wave Horner chain takes
// ~0.65 ms whatever the batch size (one 64-term MSM as long as 128 of them,
// profiles/r05_batch_floor_probe.log).  The host costs ~35 us per MSM, spread over the pool:
// 0.17-0.20 ms for 1-16 MSMs of 64 terms, 0.47 at 64, even at ~100, slower at 128
// (profiles/r05_batch_host_route_ab.log).  SVGPU_BATCH_HOST_MAX sets the largest such batch (0: never).
constexpr size_t kBatchHostMax = 64;
// msm_batch_windows_host takes at most this many MSMs
constexpr size_t kWindowsHostMaxCount = 0xffff;

// sv_bn254_g1_msm_batch (batch_split): longer MSMs leave the batch for the single-MSM pipeline; in a
// batch of at most kBatchSeqMax MSMs so does every MSM above kSmallMsmTerms terms
constexpr size_t kBatchMaxTerms = 4096, kBatchSeqMax = 4;

// ---------------------------------------------------------------------------------------------
// The SVGPU_BATCH_* switches, read in one place and once per call, so a caller (or a test's
// monkeypatch.setenv) may change them between calls.  Nothing is read during a call.
// ---------------------------------------------------------------------------------------------
struct BatchTuning {
  int window_bits = 0;               // SVGPU_BATCH_WINDOW_BITS: 5 or 8 forces c; anything else is ignored (0)
  size_t host_max = kBatchHostMax;   // SVGPU_BATCH_HOST_MAX: the largest batch on the host-Horner route
  // SVGPU_BATCH_QUAD=0: the round-2 kernels (per-lane window sums, one-wave Horner)
  bool quad = true;
  // SVGPU_BATCH_BUCKETS=0: the per-window weighting of k_batch_windows_q instead of the bucket-wise
  // Horner (k_batch_buckets_q + k_batch_horner_b)
  bool buckets = true;
  bool fuse = true;                  // SVGPU_BATCH_FUSE=0: the bucket sums and the Horner as two kernels, back to back
  uint32_t bw = kFuseBw;             // SVGPU_BATCH_BW: bucket waves per MSM of a fused launch, clamped to [1, kQW]
  // SVGPU_BATCH_WAIT_SPINS: the fused launch's wait bound; tests set it to 0 to force the timeout
  // and the two-kernel redo
  uint32_t spin_max = kFuseSpinMax;
  size_t max_terms = kBatchMaxTerms; // SVGPU_BATCH_MAX: see batch_split
  size_t seq_max = kBatchSeqMax;     // SVGPU_BATCH_SEQ_MAX: see batch_split
};

inline BatchTuning batch_tuning() {
  auto on = [](const char* name) {  // default on
    const char* e = getenv(name);
    return !e || atoi(e) != 0;
  };
  BatchTuning t;
  if (const char* e = getenv("SVGPU_BATCH_WINDOW_BITS")) {
    const int c = atoi(e);
    if (c == 5 || c == 8) t.window_bits = c;
  }
  if (const char* e = getenv("SVGPU_BATCH_HOST_MAX")) t.host_max = (size_t)strtoull(e, nullptr, 10);
  t.quad = on("SVGPU_BATCH_QUAD");
  t.buckets = on("SVGPU_BATCH_BUCKETS");
  t.fuse = on("SVGPU_BATCH_FUSE");
  if (const char* e = getenv("SVGPU_BATCH_BW")) t.bw = std::min<uint32_t>(kQW, std::max(1, atoi(e)));
  if (const char* e = getenv("SVGPU_BATCH_WAIT_SPINS")) t.spin_max = (uint32_t)strtoul(e, nullptr, 10);
  if (const char* e = getenv("SVGPU_BATCH_MAX")) t.max_terms = strtoull(e, nullptr, 10);
  if (const char* e = getenv("SVGPU_BATCH_SEQ_MAX")) t.seq_max = strtoull(e, nullptr, 10);
  return t;
}

inline int batch_window_bits(size_t max_terms, const BatchTuning& t) {
  return t.window_bits ? t.window_bits : (max_terms <= (size_t)kQMaxTerms ? 5 : 8);
}

// ---------------------------------------------------------------------------------------------
// The route of one msm_batch_device call
// ---------------------------------------------------------------------------------------------
enum class BatchRoute {
  HostHorner,    // k_batch_prep + k_batch_uwin, the Horners on the host (msm_batch_windows_host)
  Fused,         // k_batch_prep + k_batch_fused; wants the device's fused-launch slot (FuseSlot)
  BucketHorner,  // k_batch_prep + k_batch_buckets_q + k_batch_horner_b
  QuadWindows,   // k_batch_prep + k_batch_windows_q + k_msm_batch_horner_q<5>
  LaneWindows,   // k_msm_batch_windows<c> + k_msm_batch_horner_q<c> or k_msm_batch_horner<c>
};

struct BatchPlan {
  BatchRoute route;
  size_t count, max_terms;
  int c;             // window bits
  uint32_t W, WG;    // windows, and the window groups of k_msm_batch_windows<c> (its blockIdx.y)
  bool quad_horner;  // LaneWindows: k_msm_batch_horner_q<c> (else the one-wave k_msm_batch_horner<c>)
  uint32_t bw, spin_max;  // Fused: bucket waves per MSM, the wait bound
  size_t nT;         // sums the window kernels leave: per bucket, per window, or HostHorner's U_k
  size_t nflag;      // Fused: one ready flag per (MSM, window)
  size_t dig_bytes, pts_bytes;  // k_batch_prep's digits and points (0 on LaneWindows)
};

inline size_t batch_nflag(BatchRoute r, size_t count) { return r == BatchRoute::Fused ? count * kQW : 0; }

inline BatchPlan batch_plan(size_t count, size_t max_terms, bool has_ids, bool has_bidx, const BatchTuning& t) {
  BatchPlan p;
  p.count = count;
  p.max_terms = max_terms;
  p.c = batch_window_bits(max_terms, t);
  p.W = p.c == 5 ? BatchCfg<5>::W : BatchCfg<8>::W;
  p.WG = p.c == 5 ? BatchCfg<5>::WG : BatchCfg<8>::WG;
  p.quad_horner = t.quad;
  p.bw = t.bw;
  p.spin_max = t.spin_max;
  const bool prep = p.c == kQC && max_terms <= (size_t)kQMaxTerms;  // k_batch_prep's digits fit its users' LDS
  // Known quirk, kept: with SVGPU_BATCH_HOST_MAX above kWindowsHostMaxCount a plain batch of more
  // MSMs than that still takes this route and ends in msm_batch_windows_host's argument error.
  if (!has_ids && !has_bidx && count <= t.host_max && max_terms >= 1 && prep) p.route = BatchRoute::HostHorner;
  else if (!(t.quad && prep)) p.route = BatchRoute::LaneWindows;
  else if (!(t.buckets && count <= kBucketHornerMax)) p.route = BatchRoute::QuadWindows;
  else if (!(t.fuse && count <= kFuseMax)) p.route = BatchRoute::BucketHorner;
  else p.route = BatchRoute::Fused;
  const bool buckets = p.route == BatchRoute::Fused || p.route == BatchRoute::BucketHorner;
  p.nT = p.route == BatchRoute::HostHorner ? count * kQW * kUPerWin : buckets ? count * kQB * kQW : count * p.W;
  p.nflag = batch_nflag(p.route, count);
  p.dig_bytes = p.route == BatchRoute::LaneWindows ? 0 : count * kQW * 2 * max_terms;
  p.pts_bytes = p.route == BatchRoute::LaneWindows ? 0 : count * 2 * max_terms * kAffBytes;
  return p;
}

// A Fused plan whose slot is held by another call: the same buffers, two kernels, no flags
inline BatchPlan batch_without_slot(BatchPlan p) {
  p.route = BatchRoute::BucketHorner;
  p.nflag = batch_nflag(p.route, p.count);
  return p;
}

// ---------------------------------------------------------------------------------------------
// Workspace layouts (MsmLayout, msm_plan.hpp): every buffer is declared once, the reserved size is
// the end of the last one; ws are offsets into Workspace::buf, pin into Workspace::pinned.  A
// buffer no kernel of the route reads is absent (kAbsent).
// ---------------------------------------------------------------------------------------------
struct BatchBuffers {
  MsmLayout ws, pin;
  size_t flags;     // the error word, then (Fused) the window flags: zeroed by one memset
  size_t T, dig, pts;
  size_t off;       // msm_batch_windows_host with one MSM and no offsets of the caller's: {0, max_terms}
  size_t pin_back;  // what is copied back: the error word (and msm_batch_windows_host's sums)
  size_t pin_off;   // the host's copy of `off`
  size_t back_bytes;
};

// msm_batch_device on every route but HostHorner
inline BatchBuffers batch_buffers(const BatchPlan& p) {
  BatchBuffers b;
  b.flags = b.ws.put("flags", 1 + p.nflag, 4);
  b.T = b.ws.put("T", p.nT, kXyzzBytes);
  b.dig = b.ws.put("dig", p.dig_bytes, 1);
  b.pts = b.ws.put("pts", p.pts_bytes / kAffBytes, kAffBytes);
  b.off = b.pin_off = MsmLayout::kAbsent;
  b.back_bytes = 4;
  b.pin_back = b.pin.put("back", 1, 4);
  return b;
}

// msm_batch_windows_host: the error word on a line of its own, then the partial sums U, so ONE copy
// brings both back (T is U's offset, in the workspace and in the pinned copy alike)
constexpr size_t kWindowsHostErrBytes = 256;
inline bool batch_windows_host_ok(size_t count, size_t max_terms) {
  return max_terms >= 1 && max_terms <= (size_t)kQMaxTerms && count <= kWindowsHostMaxCount;
}
inline BatchBuffers batch_windows_host_buffers(size_t count, size_t max_terms, bool single) {
  BatchBuffers b;
  b.back_bytes = kWindowsHostErrBytes + count * kQW * kUPerWin * kXyzzBytes;
  b.flags = b.ws.put("block", b.back_bytes, 1);
  b.T = b.flags + kWindowsHostErrBytes;
  b.dig = b.ws.put("dig", count * kQW * 2 * max_terms, 1);
  b.pts = b.ws.put("pts", count * 2 * max_terms, kAffBytes);
  b.off = b.ws.put("off", single ? 2 : 0, 8);
  b.pin_back = b.pin.put("back", b.back_bytes, 1);
  b.pin_off = b.pin.put("off", 2, 8);
  return b;
}

// msm_batch_fixed_device: the error word alone
inline BatchBuffers batch_fixed_buffers() {
  BatchBuffers b;
  b.flags = b.ws.put("flags", 1, 4);
  b.T = b.dig = b.pts = b.off = b.pin_off = MsmLayout::kAbsent;
  b.back_bytes = 4;
  b.pin_back = b.pin.put("back", 1, 4);
  return b;
}

// ---------------------------------------------------------------------------------------------
// sv_bn254_g1_msm_batch: MSMs of more than the limit's terms (big_ids) go through the single-MSM
// pipeline one by one, the others (small_ids, the longest of max_small terms) stay in the batch.
// The fused batch kernel costs about one Horner chain (~0.65 ms) whatever the batch size, so in a
// tiny batch (at most SVGPU_BATCH_SEQ_MAX MSMs) the limit drops from SVGPU_BATCH_MAX to
// kSmallMsmTerms.  MSMs of at most kSmallMsmTerms terms always stay: a batch of only such MSMs
// passes no id map, so msm_batch_device can take its HostHorner route (0.17-0.20 ms for 1-16 MSMs
// of 64 terms).
// ---------------------------------------------------------------------------------------------
inline void batch_split(const uint64_t* offsets, size_t count, const BatchTuning& t, std::vector<uint32_t>* small_ids,
                        std::vector<uint32_t>* big_ids, size_t* max_small) {
  const size_t limit = count <= t.seq_max ? std::min(t.max_terms, kSmallMsmTerms) : t.max_terms;
  *max_small = 0;
  for (size_t k = 0; k < count; k++) {
    const size_t m = offsets[k + 1] - offsets[k];
    if (m > limit) {
      big_ids->push_back((uint32_t)k);
    } else {
      small_ids->push_back((uint32_t)k);
      *max_small = std::max(*max_small, m);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The fused-launch slot.  HIP promises no co-residency between workgroups of a launch, and the
// Horner waves of a fused launch hold their slots while they wait: one fused launch (count <=
// kFuseMax waves) leaves most of the chip's wave slots to its bucket blocks, but several at once on
// one GPU (concurrent callers, a logical device map with repeats) could fill it with waiting waves.  So at
// most ONE fused launch is in flight per physical device; a call that finds the slot held takes
// BucketHorner.  Devices share slots modulo 64.
// ---------------------------------------------------------------------------------------------
class FuseSlot {
 public:
  FuseSlot() = default;
  FuseSlot(const FuseSlot&) = delete;
  FuseSlot& operator=(const FuseSlot&) = delete;
  ~FuseSlot() { release(); }
  // false: another call holds the device's slot
  bool acquire(int device) {
    static std::atomic<int> inflight[64];
    std::atomic<int>& f = inflight[device & 63];
    if (f.fetch_add(1, std::memory_order_acq_rel) != 0) {
      f.fetch_sub(1, std::memory_order_acq_rel);
      return false;
    }
    slot_ = &f;
    return true;
  }
  void release() {
    if (slot_) slot_->fetch_sub(1, std::memory_order_acq_rel);
    slot_ = nullptr;
  }

 private:
  std::atomic<int>* slot_ = nullptr;
};

}  // namespace sv
