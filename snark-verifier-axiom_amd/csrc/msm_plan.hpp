// Host-side planning of the single-MSM pipeline (msm.hip): the plan, the SVGPU_* switches, the
// per-call shape, the workspace layout and the event slots.  No HIP here: plain C++17, so the
// arithmetic that sizes every buffer can be built and checked on its own
// (tests/native/msm_layout_check.cpp).  The constants below are the ones the kernels use too.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "field29.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define SV_PLAN_HD __host__ __device__
#define SV_PLAN_HDI __host__ __device__ __forceinline__
#else
#define SV_PLAN_HD
#define SV_PLAN_HDI inline
#endif

namespace sv {

constexpr int kBlock = 256;

// MSMs of at most this many terms skip the pipeline: window sums on the device, the window Horner on
// the host (msm_batch_windows_host); SVGPU_SMALL_MSM=0 keeps the pipeline for them.
constexpr size_t kSmallMsmTerms = 256;

// element sizes of the device types (curve.hpp; msm.hip asserts that they agree)
constexpr size_t kFrBytes = 32, kAffBytes = 64, kXyzzBytes = 128;

// Bucket-sum records (bsum, pfirst, plast): canonical G1Xyzz (128 B) for the 32-bit chain, the
// 29-bit chain's own 4 x 9 limbs (144 B) otherwise -- see msm.hip
constexpr uint32_t kRec29Words = 4 * r29::L;  // 36
SV_PLAN_HDI size_t bucket_rec_bytes(int r29) { return r29 ? 4 * kRec29Words : kXyzzBytes; }

// uint4 per point of the r29 table (its buffer is carved in uint4): GLV two 72-B records, else one
// (padded to 80 B per point so host-fed pieces' table slices stay uint4-aligned)
SV_PLAN_HD constexpr size_t vtab_uint4_per_point(bool glv) { return glv ? 9 : 5; }

// Points per block of the histogram / scatter passes (ep: entries per point).  1024 (round 3) halves
// the block count, so each (window, bin) run a scatter block writes is ~16 entries (64 B) instead of
// ~8: sort 0.221 -> 0.206 ms at 2^20.  LDS: the scatter stages CH * ep u32 entries (2048 spilled
// the scatter's digit registers: 336 B scratch, one wave per SIMD).
#ifndef SV_SORT_CHUNK
#define SV_SORT_CHUNK 1024
#endif
SV_PLAN_HD constexpr uint32_t sort_chunk(int ep) {
  return ep > 20 ? 256u : (ep > 16 && SV_SORT_CHUNK > 1024 ? 1024u : (uint32_t)SV_SORT_CHUNK);
}
// coarse bits: 2^CB bins per window, so that W * 2^CB ~ 1024 fine-sort regions of ~16K entries at
// 2^20 (LDS-staged in k_fine_sort) -- 64 bins for the 16 full-width windows, 128 for the 8 GLV ones
SV_PLAN_HD constexpr int coarse_bits(int c, int nb) { return c - 1 < (nb == 128 ? 7 : 6) ? c - 1 : (nb == 128 ? 7 : 6); }

// k_wsum_tree (msm.hip)
constexpr int kTreeLog = 8, kTreeN = 1 << kTreeLog;  // segments per block (= threads)
constexpr int kTreeOut = 2 + kTreeLog;               // per-block outputs

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// ---------------------------------------------------------------------------------------------
// The SVGPU_* switches of the single-MSM host path, read in one place (msm_tuning).  sort_xcd,
// sort_bm and msm_stats are read once per process; every other one once per call, so a caller (or a
// test's monkeypatch.setenv) may change it between calls.  Nothing is read during a call.
// ---------------------------------------------------------------------------------------------
struct MsmTuning {
  struct Opt {  // a switch without a fixed default: unset leaves the planned value
    bool set = false;
    int v = 0;
  };
  Opt acc_k;            // SVGPU_ACC_K: sorted entries per accumulate thread, forced (pieces too)
  Opt glv;              // SVGPU_GLV: forces the GLV split on (n >= 2) or off, see msm_plan
  int glv_max_log = 21; // SVGPU_GLV_MAX_LOG: GLV up to 2^this points, see msm_plan
  Opt glv_phi64;        // SVGPU_GLV_PHI64: whole phi(P) records or beta x only, see msm_plan
  Opt window_bits;      // SVGPU_WINDOW_BITS: c, clamped to [4, 16]
  Opt red_log;          // SVGPU_RED_LOG: log2 of the buckets per running-sum segment, see msm_plan
  int group_tree = 1;   // SVGPU_GROUP_TREE: the bucket reduction, see msm_plan
  // SVGPU_GROUP_QUAD=0: k_group_sum instead of k_group_sum_q (the reduction without the tree)
  bool group_quad = true;
  Opt group_p;          // SVGPU_GROUP_P: k_group_sum blocks per group (default 2 below 256 group sums, else 1)
  // SVGPU_ACC_R29=0: k_accumulate's 32-bit chain (AccChain).  Fixed per call, so the accumulate,
  // fixup and reduction launches of one MSM agree on the stored form.  (A resident base set holds
  // only the 29-bit table, so its calls use that chain whatever the switch says.)
  bool acc_r29 = true;
  bool sort_e32 = true; // SVGPU_SORT_E32=0: u64 sort entries even where every point index fits u32
  bool sort_xcd = true; // SVGPU_SORT_XCD=0 (per process): the sort passes without the XCD-aware block map
  // SVGPU_SORT_BM=0 (per process): key-major per-block counts (k_bin_scan_chunks) instead of
  // block-major ones + the tiled scan
  bool sort_bm = true;
  bool hist_pf = true;  // SVGPU_HIST_PF=0: the histogram pass without the one-ahead loads (29-bit table path)
  int scan_keys = 32;   // SVGPU_SCAN_KEYS=16: tiles of 16 keys (twice the blocks, 64 row groups per key); default 32
  // SVGPU_FINE_SPLIT=1: the round-2 pair of k_fine_sort launches instead of one launch for both
  // region kinds (the large regions optionally on a side stream, sort_fork)
  bool fine_split = false;
  bool sort_fork = false;  // SVGPU_SORT_FORK=1: off, measured slower (the join delays the accumulate)
  // SVGPU_SORT_HALVES=0: the scatter recomputes the digits instead of reading the histogram pass's
  // stored halves (32 B per point; the device path without window halves only)
  bool sort_halves = true;
  // SVGPU_MSM_SPLIT=1 (device-resident inputs; off by default): the windows in two halves
  // A = [0, WA), B = [WA, W), each sorted, accumulated and reduced on its own, so that half B's sort
  // runs on the sort stream beside half A's accumulate and half A's reduction beside half B's
  // accumulate.  Measured slower at 2^20 (round 4, two A/B pairs: 1.89-1.92 vs 1.81-1.82 ms/step):
  // a half sort costs 0.155 ms, not half of 0.195 (every point's GLV split and digits are still
  // computed), and the two accumulate launches barely overlap (span 1.47 ms, their own durations
  // 1.52 ms): k_accumulate holds two 256-thread blocks per CU, so half A's 512 blocks already fill
  // the chip and half B's wait for them -- one round of blocks each, as the whole launch's two.
  bool msm_split = false;
  // each event record between kernels costs ~5.5 us of idle GPU (rocprof trace): the accumulate is
  // always bracketed (bench.py's live roofline), the sort / fixup splits only with
  // SVGPU_MSM_STATS=1 (per process)
  bool msm_stats = false;
  bool msm_lean = false;  // SVGPU_MSM_LEAN=1: only the accumulate's two events, no sort / reduce split
  // The landed bases' preparation (conversion / check / the piece's phi table) runs on the sort
  // stream behind the piece's sort (round 3: off the compute stream, whose back-to-back accumulates
  // are the host-fed path's critical path once the first piece has landed); SVGPU_FED_PREP=0 keeps
  // it on the compute stream
  bool fed_prep = true;
  // Small MSMs (round 5): the window sums on the device, the window Horner on the host
  // (msm_batch_windows_host, msm_batch.hip): the pipeline is latency-bound there (a 64-term MSM took
  // ~0.35 ms: a dozen launches, serial accumulate chunks, the reduction kernels and a host Horner
  // over 52 windows).  SVGPU_SMALL_MSM=0 keeps the pipeline.
  bool small_msm = true;
  std::vector<double> h2d_split;  // SVGPU_H2D_SPLIT: comma-separated piece weights, see piece_bounds
};

inline MsmTuning msm_tuning() {
  auto opt = [](const char* name) {
    MsmTuning::Opt o;
    if (const char* e = getenv(name)) o.set = true, o.v = atoi(e);
    return o;
  };
  auto on = [](const char* name) { return !getenv(name) || atoi(getenv(name)) != 0; };    // default on
  auto off = [](const char* name) { return getenv(name) && atoi(getenv(name)) != 0; };    // default off
  MsmTuning t;
  t.acc_k = opt("SVGPU_ACC_K");
  t.glv = opt("SVGPU_GLV");
  if (const char* e = getenv("SVGPU_GLV_MAX_LOG")) t.glv_max_log = atoi(e);
  t.glv_phi64 = opt("SVGPU_GLV_PHI64");
  t.window_bits = opt("SVGPU_WINDOW_BITS");
  t.red_log = opt("SVGPU_RED_LOG");
  if (const char* e = getenv("SVGPU_GROUP_TREE")) t.group_tree = atoi(e);
  t.group_quad = on("SVGPU_GROUP_QUAD");
  t.group_p = opt("SVGPU_GROUP_P");
  t.acc_r29 = on("SVGPU_ACC_R29");
  t.sort_e32 = on("SVGPU_SORT_E32");
  static const bool xcd = on("SVGPU_SORT_XCD"), bm = on("SVGPU_SORT_BM"), stats = off("SVGPU_MSM_STATS");
  t.sort_xcd = xcd;
  t.sort_bm = bm;
  t.msm_stats = stats;
  t.hist_pf = on("SVGPU_HIST_PF");
  if (const char* e = getenv("SVGPU_SCAN_KEYS")) t.scan_keys = atoi(e) == 16 ? 16 : 32;
  t.fine_split = off("SVGPU_FINE_SPLIT");
  t.sort_fork = off("SVGPU_SORT_FORK");
  t.sort_halves = on("SVGPU_SORT_HALVES");
  t.msm_split = off("SVGPU_MSM_SPLIT");
  t.msm_lean = off("SVGPU_MSM_LEAN");
  t.fed_prep = on("SVGPU_FED_PREP");
  t.small_msm = on("SVGPU_SMALL_MSM");
  if (const char* e = getenv("SVGPU_H2D_SPLIT")) {
    for (const char* q = e; *q;) {
      char* end = nullptr;
      const double v = strtod(q, &end);
      if (end == q) break;
      if (v > 0) t.h2d_split.push_back(v);
      q = *end == ',' ? end + 1 : end;
      if (*end && *end != ',') break;
    }
  }
  return t;
}

// ---------------------------------------------------------------------------------------------
struct MsmPlan {
  int c;            // window bits (signed digits: 2^(c-1) buckets per window)
  uint32_t W;       // windows = ceil(255 / c)
  uint32_t B;       // buckets per window
  uint32_t nbt;     // W * B
  uint32_t K;       // sorted entries per accumulate thread
  uint32_t T;       // accumulate threads
  uint32_t logL;    // log2 of the buckets per running-sum segment
  uint32_t J;       // running-sum segments per window (B >> logL)
  uint32_t logJ;    // log2(J)
  uint32_t NG;      // subset-sum groups per window: 2 + logJ
  bool glv;         // GLV split: 2n virtual points (P, phi(P)) with 128-bit scalar halves
  size_t npts;      // virtual points: n, or 2n with GLV
  int phi64;        // GLV table: whole phi(P) records (1) or beta x only (0)
  int tree;         // bucket reduction: 0 k_wsum + k_group_sum, 1 running sums + tree, 2 tree over buckets
  int r29;          // k_accumulate's chain: 29-bit limbs, sums stored as x R' words (1) or 32-bit (0)
};

// Sorted entries per accumulate thread for `entries` entries over nbt buckets (SVGPU_ACC_K forces it)
inline uint32_t plan_K(uint64_t entries, uint32_t nbt, const MsmTuning& t) {
  uint64_t K = entries / (1u << 18);
  if (K < 4) K = 4;
  if (K > 32) K = 32;
  // large n: buckets average entries / nbt > 32 entries; a chunk of about one average bucket keeps
  // most crossing buckets at two pieces (joined inside k_accumulate), capped at 256 entries so the
  // grid still has many rounds of waves (swept, tools/gpu_sweep_big.sh: 2^21 K = 64 4.47 -> 4.41 ms;
  // 2^24 K = 256 32.0 ms, 512 32.4, 1024 33.4)
  const uint64_t avg_bucket = entries / nbt;
  if (K < avg_bucket) K = avg_bucket < 256 ? avg_bucket : 256;
  if (t.acc_k.set) K = (uint64_t)t.acc_k.v;
  if (K < 1) K = 1;
  return (uint32_t)K;
}

// Host-fed pieces (a fraction of the points over the whole bucket set, so few entries per bucket):
// chunks of about one average bucket, a multiple of 8, at least 16.  Round 3 (the 32-bit chain,
// measured device-resident at the 2^20 plan's window) had found about two average buckets best while
// that stayed <= 32 entries: a segment end then cost ~110 VALU instructions.  With the round-6
// chain's raw-record segment ends, a quarter-size piece's accumulate at K = 32 filled only half the
// chip's block slots; one average bucket (K = 24, 16, 16, 16 for the 2^20 pieces 5,4,4,3) measured
// 2.538-2.570 ms per host-fed 2^20 MSM against 2.602-2.609 (SVGPU_ACC_K = 16 for every piece, two
// passes, profiles/r06_host_piece_k.log).
inline uint32_t piece_K(uint64_t entries, uint32_t nbt, const MsmTuning& t) {
  if (t.acc_k.set) return plan_K(entries, nbt, t);
  const uint64_t avg = entries / nbt;
  const uint64_t K = std::min<uint64_t>(std::max<uint64_t>((avg + 7) / 8 * 8, 16), 256);
  return (uint32_t)K;
}

inline MsmPlan msm_plan(size_t n, const MsmTuning& t) {
  MsmPlan p;
  // GLV (k P = k1 P + k2 phi(P), 128-bit halves, split on the fly by the sort passes) halves the
  // buckets, the bucket reduction and the host Horner for the same number of bucket entries, at the
  // cost of a 32-B beta-x table per point.  Measured (r02, med ms, GLV off -> on): 2^14 0.79 -> 0.74,
  // 2^16 0.98 -> 0.82, 2^18 1.75 -> 1.54, 2^20 2.11 -> 2.05, 2^21 3.74 -> 3.62; at 2^22 (6.88 ->
  // 7.39) and 2^24 (27.3 -> 31.1) the larger gather working set (bases + beta-x beyond the 256 MiB
  // Infinity Cache) slows the fill, so it is on up to 2^SVGPU_GLV_MAX_LOG points (default 21);
  // SVGPU_GLV forces it.
  p.glv = n >= (size_t(1) << 14) && n <= (size_t(1) << t.glv_max_log);
  if (t.glv.set) p.glv = t.glv.v != 0 && n >= 2;
  p.npts = p.glv ? 2 * n : n;
  // whole phi(P) records (one 64-B gather per k2 entry) while bases + table stay well inside the
  // Infinity Cache; beta-x only above (measured at 2^20: 1.97-2.01 vs 2.01-2.15 ms, k_accumulate
  // 1.39 vs 1.39-1.50 ms)
  p.phi64 = n <= (size_t(1) << 20);
  if (t.glv_phi64.set) p.phi64 = t.glv_phi64.v != 0;
  const int nb = p.glv ? 128 : 255;
  int lg = 0;
  while ((size_t(1) << (lg + 1)) <= p.npts) lg++;
  int c = lg - 4;
  if (t.window_bits.set) c = t.window_bits.v;
  if (c < 4) c = 4;
  if (c > 16) c = 16;
  p.c = c;
  p.W = (nb + c - 1) / c;
  p.B = 1u << (c - 1);
  p.nbt = p.B * p.W;
  uint64_t entries = (uint64_t)p.npts * p.W;
  p.K = plan_K(entries, p.nbt, t);
  p.T = cdiv(entries, p.K);
  // reduction: J running-sum segments per window, NG subset groups of H = J/2 points
  // 8 buckets per running-sum segment (swept: tools/gpu_sweep_red.sh); 4 with GLV, whose W / 2
  // windows would otherwise leave half the SIMDs without a k_wsum wave
  p.logL = p.glv ? 2 : 3;
  if (t.red_log.set) p.logL = t.red_log.v;
  if (p.logL < 1) p.logL = 1;
  if (p.logL > (uint32_t)(p.c - 3)) p.logL = p.c - 3 > 1 ? p.c - 3 : 1;
  // bucket reduction (SVGPU_GROUP_TREE): 1 (default) running sums + in-block subset-sum tree
  // (k_wsum_tree<true>) when a window's segments fill whole 256-segment blocks, at most 64 of them;
  // 2 the tree straight over the buckets (k_wsum_tree<false>, no running sums: L = 1); 0 k_wsum +
  // k_group_sum(_q)
  p.tree = t.group_tree;
  p.r29 = t.acc_r29;  // see MsmTuning
  if (p.tree == 2 && p.B % kTreeN == 0 && p.B / kTreeN <= 128) p.logL = 0;
  else if (p.tree == 2) p.tree = 1;
  p.J = p.B >> p.logL;
  if (p.tree == 1 && !(p.J % kTreeN == 0 && p.J / kTreeN <= 64)) p.tree = 0;
  p.logJ = 0;
  while ((1u << p.logJ) < p.J) p.logJ++;
  p.NG = 2 + p.logJ;
  return p;
}
inline MsmPlan msm_plan(size_t n) { return msm_plan(n, msm_tuning()); }

// Host-fed piece boundaries: SVGPU_H2D_SPLIT = comma-separated weights, else `pieces` equal pieces
// (SVGPU_H2D_PIECES), else the default schedule: 4 equal pieces from 2^18 points.  A piece's
// accumulate runs once its bases have landed (96 B per point at ~52 GB/s), and once the first piece
// is in, the compute stream is the bottleneck (a piece's accumulate + fixup outlasts the next
// piece's transfer), so what counts is the total accumulate work -- smaller pieces are less efficient
// -- against starting early and leaving little after the last byte.  Measured at 2^20 (3 boxes,
// tools/host_api_bench.py): 4 equal pieces 2.73-2.92 ms, 2,2,3,3,3,3 2.74-3.06, 2,3,3,3,3,2
// 2.74-3.09, 3 pieces 3.41-3.47, 6 3.17-4.20 (before per-piece K), 1 piece 3.76-3.95.
constexpr int kMaxPieces = 16;  // every piece has three event slots (ev_slot)
inline std::vector<size_t> piece_bounds(size_t n, int pieces, const std::vector<double>& dflt,
                                        const MsmTuning& t) {
  std::vector<double> wts = t.h2d_split;
  if (wts.empty()) {
    if (pieces > 0) {
      wts.assign(std::min(pieces, kMaxPieces), 1.0);
    } else if (n >= (size_t(1) << 18) && !dflt.empty()) {
      wts = dflt;
    } else if (n >= (size_t(1) << 18)) {
      // decreasing: the copy (1.7 ns per point) outpaces the pieces' accumulates (~1.3 ns), so the
      // last piece -- whose accumulate is the call's tail -- is the smallest (round 4, 2^20, three
      // A/B pairs: 5,4,4,3 2.594-2.597 ms vs 4 equal 2.639-2.657; 5,4,4,2,1 2.669-2.670)
      wts = {5, 4, 4, 3};
    } else if (n >= (size_t(1) << 15)) {
      wts = {1, 1};
    } else {
      wts = {1};
    }
  }
  if (wts.size() > (size_t)kMaxPieces) wts.resize(kMaxPieces);
  // pieces below 4096 points are not worth a launch sequence
  while (wts.size() > 1 && n < wts.size() * 4096) wts.pop_back();
  double tot = 0;
  for (double v : wts) tot += v;
  std::vector<size_t> b{0};
  double cum = 0;
  for (size_t k = 0; k + 1 < wts.size(); k++) {
    cum += wts[k];
    // boundaries on multiples of 1024 points: every piece's copies start 32-KiB aligned (5 equal
    // pieces, boundaries 32-B aligned, measured 3.13-3.17 ms vs 2.73-2.76 for 4 and 6)
    const size_t at = ((size_t)((double)n * cum / tot)) & ~size_t(1023);
    b.push_back(std::max(b.back(), std::min(n, at)));
  }
  b.push_back(n);
  b.erase(std::unique(b.begin(), b.end()), b.end());
  if (b.size() < 2) b = {0, n};
  return b;
}

// ---------------------------------------------------------------------------------------------
// Event slots of Workspace::ev (msm.hip asserts kCount <= Workspace::kEvents)
// ---------------------------------------------------------------------------------------------
namespace ev_slot {
enum : int {
  kStart = 0,     // stats: the call's first record on the compute stream
  kSortMid = 1,   // stats (detail): after the histogram pass
  kAccBegin = 2,  // before the (first piece's / half A's) accumulate
  kAccEnd = 3,    // after the (last piece's / half A's) accumulate
  kFixEnd = 4,    // stats (detail): after the fixup
  kEnd = 5,       // stats: after the reduction
  kFedFork = 6,   // host-fed: the copy and sort streams start behind the compute stream's memsets
  kPiece0 = 8,    // three per piece, see below
  kSortFork = 60, kSortJoin = 61,    // SVGPU_SORT_FORK: the large fine-sort regions' side stream
  kHalfBAccBegin = 62, kHalfBAccEnd = 63,  // SVGPU_MSM_SPLIT: half B's accumulate
  kCount = 64,
  // the small route's staging of a fed call's inputs (nothing else is recorded there)
  kSmallScalars = 0, kSmallBases = 1,
};
constexpr int piece_scalars(int k) { return kPiece0 + 3 * k; }  // piece k's scalars have landed
constexpr int piece_bases(int k) { return kPiece0 + 3 * k + 1; }  // its bases have landed
constexpr int piece_sorted(int k) { return kPiece0 + 3 * k + 2; }  // its sort (and preparation) is done
constexpr int kHalfBEnd = piece_scalars(0);  // SVGPU_MSM_SPLIT: half B's fixup done (device inputs: no pieces)
static_assert(kFedFork < kPiece0 && piece_sorted(kMaxPieces - 1) < kSortFork && kHalfBAccEnd < kCount,
              "event slots overlap");
}  // namespace ev_slot

// ---------------------------------------------------------------------------------------------
// The shape of one call: everything the buffer sizes and the launch sequence depend on
// ---------------------------------------------------------------------------------------------
struct MsmMode {
  bool canonical = false;  // SV_CANONICAL input (bases converted into a workspace copy)
  bool fed = false;        // host-fed: inputs arrive in pieces
  bool resident = false;   // bases are rows of a resident set: nothing per call but the scalars
  int pieces = 0;          // MsmFeed::pieces, MsmFeed::split
  std::vector<double> split;
};
struct MsmShape {
  // host-fed inputs arrive in pieces (piece_bounds): piece k is sorted on the sort stream once its
  // scalars have landed and accumulated on the compute stream once its bases have, while later
  // pieces are still in flight.  Device inputs: one piece.
  std::vector<size_t> pb;
  int pieces;
  std::vector<uint32_t> K, T;  // per piece: entries per accumulate thread (for its own size), threads
  uint32_t ep;                 // entries per real point
  size_t max_piece;
  uint64_t tst_total;          // tstart words of all pieces (T + 1 each)
  uint32_t Tmax;
  uint64_t entries;            // all pieces
  uint64_t piece_entries;      // the sort scratch, reused per piece
  bool split;                  // MsmTuning::msm_split, where it applies
  uint32_t nwh[2], Th[2];      // the halves' windows and accumulate threads
  uint32_t nwb, nblk;          // (window, bin) keys and histogram blocks of the largest piece
  bool conv;
  size_t tab4;                 // uint4 per point of the GLV / 29-bit table (0: none)
  size_t nfinal;               // group sums: W * NG
  uint32_t gparts;             // k_group_sum blocks per group (see there)
  size_t nerr;                 // err flag, heavy/multi queue counters, group counters
  bool keep_halves;            // MsmTuning::sort_halves, where it applies
  size_t rec_bytes;            // bucket-sum records (29-bit chain: 144 B)
  size_t ntree;                // per-block tree outputs (0 without the tree)
};

inline MsmShape msm_shape(size_t n, const MsmMode& m, const MsmPlan& p, const MsmTuning& t) {
  MsmShape s;
  s.pb = m.fed ? piece_bounds(n, m.pieces, m.split, t) : std::vector<size_t>{0, n};
  s.pieces = (int)s.pb.size() - 1;
  s.ep = p.glv ? 2 * p.W : p.W;
  s.max_piece = 0;
  s.tst_total = 0;
  s.Tmax = 0;
  s.K.resize(s.pieces);
  s.T.resize(s.pieces);
  for (int k = 0; k < s.pieces; k++) {
    const uint64_t e = (uint64_t)(s.pb[k + 1] - s.pb[k]) * s.ep;
    s.max_piece = std::max(s.max_piece, s.pb[k + 1] - s.pb[k]);
    s.K[k] = m.fed ? piece_K(e, p.nbt, t) : p.K;
    s.T[k] = cdiv(e, s.K[k]);
    s.tst_total += (uint64_t)s.T[k] + 1;
    s.Tmax = std::max(s.Tmax, s.T[k]);
  }
  s.entries = (uint64_t)n * s.ep;
  s.piece_entries = (uint64_t)s.max_piece * s.ep;
  s.split = !m.fed && !m.resident && t.msm_split && p.W >= 2 && p.tree == 1 && n >= (size_t(1) << 16);
  s.nwh[0] = s.split ? p.W / 2 : p.W;
  s.nwh[1] = s.split ? p.W - p.W / 2 : 0;
  s.Th[0] = s.Th[1] = 0;
  if (s.split) {
    for (int h = 0; h < 2; h++) s.Th[h] = cdiv((uint64_t)p.npts * s.nwh[h], p.K);
    s.tst_total = (uint64_t)s.Th[0] + 1 + s.Th[1] + 1;
    s.Tmax = s.Th[0] + s.Th[1];
  }
  const int nb = p.glv ? 128 : 255;
  s.nwb = p.W * (1u << coarse_bits(p.c, nb));
  s.nblk = cdiv(s.max_piece, sort_chunk((int)s.ep));
  s.conv = m.canonical && !m.resident;
  // GLV: beta x (or phi(P)) per point; the 29-bit chain: its table of every virtual point instead
  // (none for a resident set: the accumulate reads the set's own table)
  s.tab4 = m.resident ? 0 : p.r29 ? vtab_uint4_per_point(p.glv) : (p.glv ? (p.phi64 ? 4 : 2) : 0);
  s.nfinal = (size_t)p.W * p.NG;
  s.gparts = s.nfinal < 256 ? 2 : 1;
  if (t.group_p.set) s.gparts = (uint32_t)std::max(1, t.group_p.v);
  if (s.gparts > p.J / 2) s.gparts = p.J / 2;
  s.nerr = 64 + s.nfinal;
  s.keep_halves = !m.fed && !s.split && t.sort_halves;
  s.rec_bytes = bucket_rec_bytes(p.r29);
  s.ntree = p.tree != 0 ? (size_t)p.W * (p.J / kTreeN) * kTreeOut : 0;
  return s;
}

// ---------------------------------------------------------------------------------------------
// Workspace layout: every buffer is declared once (put), which gives its offset and moves the
// total, so the reserved size is the end of the last buffer.  Offsets are 256-B aligned.
// ---------------------------------------------------------------------------------------------
struct MsmLayout {
  static constexpr size_t kAbsent = ~size_t(0);
  struct Buf {
    const char* name;
    size_t off, bytes;
  };
  Buf bufs[24];
  int count = 0;
  size_t total = 0;
  // count elements of elem bytes; a buffer of no elements is absent
  size_t put(const char* name, size_t n, size_t elem) {
    if (n == 0) return kAbsent;
    bufs[count++] = {name, total, n * elem};
    const size_t off = total;
    total += (n * elem + 255) & ~size_t(255);
    return off;
  }
};

// Offsets into Workspace::buf (ws) and Workspace::inbuf (in)
struct MsmBuffers {
  MsmLayout ws, in;
  size_t bases_m, phix, ping, err, bcnt, btot, bstart, tmp, stored, gst, ent, tstart, pfirst, plast, bsum, heavy,
      multi, racc, rtot, gpart, tree_out;
  size_t in_bases, in_scalars;
};

inline MsmBuffers msm_buffers(size_t n, const MsmMode& m, const MsmPlan& p, const MsmShape& s) {
  MsmBuffers b;
  MsmLayout& L = b.ws;
  b.bases_m = L.put("bases_m", s.conv ? n : 0, kAffBytes);
  b.phix = L.put("phix", s.tab4 * n, 16);
  // the group sums and the error flag / counters share one region: one D2H copy reads both.  The
  // error words (the flag, the fixup queue counters of every piece, the group counters from word
  // 64) are zeroed by one memset and end on a 256-B line of their own.
  const size_t err_bytes = (s.nerr * 4 + 255) & ~size_t(255);
  b.ping = L.put("ping", s.nfinal * kXyzzBytes + err_bytes, 1);
  b.err = b.ping + s.nfinal * kXyzzBytes;
  b.bcnt = L.put("bcnt", (size_t)s.nwb * s.nblk, 4);
  b.btot = L.put("btot", s.nwb, 4);
  b.bstart = L.put("bstart", (size_t)s.nwb + 1, 4);
  b.tmp = L.put("tmp", s.piece_entries, 8);  // coarse-binned entries
  // the histogram pass's digits source for the scatter (32 B per point)
  b.stored = L.put("stored", s.keep_halves ? n : 0, 32);
  b.gst = L.put("gst", ((size_t)p.nbt + 1) * s.pieces + 1, 4);  // per piece (+ 1: two window halves)
  b.ent = L.put("ent", s.entries, 4);                           // every piece's sorted entries
  b.tstart = L.put("tstart", s.tst_total, 4);                   // per piece
  b.pfirst = L.put("pfirst", s.Tmax, s.rec_bytes);
  b.plast = L.put("plast", s.Tmax, s.rec_bytes);
  b.bsum = L.put("bsum", p.nbt, s.rec_bytes);
  b.heavy = L.put("heavy", p.nbt, 4);  // heavy-bucket queue
  b.multi = L.put("multi", p.nbt, 4);  // multi-thread-bucket queue
  b.racc = L.put("racc", (size_t)p.J * p.W, kXyzzBytes);  // acc_j
  b.rtot = L.put("rtot", (size_t)p.J * p.W, kXyzzBytes);  // T_j
  b.gpart = L.put("gpart", s.nfinal * s.gparts, kXyzzBytes);  // group slice sums
  b.tree_out = L.put("tree_out", s.ntree, kXyzzBytes);
  // staging of a host-fed call's inputs: bases (none for a resident set), then scalars
  b.in_bases = b.in.put("in_bases", m.fed && !m.resident ? n : 0, kAffBytes);
  b.in_scalars = b.in.put("in_scalars", m.fed ? n : 0, kFrBytes);
  return b;
}

}  // namespace sv
