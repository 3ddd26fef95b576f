// C ABI of libsvgpu (include/svgpu.h).  Every entry point is noexcept and maps failures to
// sv_status codes with a thread-local message (sv_last_error).  No CPU fallback: compute entry
// points need a GPU and return SV_ERR_DEVICE without one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <unordered_map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/svgpu.h"
#include "codec.hpp"
#include "decider.hpp"
#include "gen.hpp"
#include "grand_product.hpp"
#include "host_ec.hpp"
#include "host_poseidon.hpp"
#include "kzg_open.hpp"
#include "lookup_permute.hpp"
#include "lp_batch_plan.hpp"
#include "msm.hpp"
#include "msm_batch.hpp"
#include "msm_batch_plan.hpp"
#include "ntt.hpp"
#include "poseidon.hpp"
#include "quotient_terms.hpp"
#include "expressions.hpp"
#include "runtime.hpp"

using namespace sv;
using sv::host::F;
using sv::host::Xyzz;

namespace {

F fe_in(const sv_fe& a) {
  F r;
  memcpy(r.l, a.l, 32);
  return r;
}
sv_fe fe_out(const F& a) {
  sv_fe r;
  memcpy(r.l, a.l, 32);
  return r;
}

void affine_out(const Xyzz& p, int form, sv_g1_affine* out) {
  F x, y;
  host::x_to_affine(p, x, y);
  if (form == SV_CANONICAL && !host::x_is_identity(p)) {
    x = host::f_from_mont(x);
    y = host::f_from_mont(y);
  }
  out->x = fe_out(x);
  out->y = fe_out(y);
}

void jacobian_out(const Xyzz& p, sv_g1_jacobian* out) {
  F X, Y, Z;
  host::x_to_jacobian(p, X, Y, Z);
  out->x = fe_out(host::f_from_mont(X));
  out->y = fe_out(host::f_from_mont(Y));
  out->z = fe_out(host::f_from_mont(Z));
}

int resolve_gpus(int num_gpus) {
  int have = runtime_device_count();
  if (have == 0) {
    if (runtime_init(0) != SV_OK) return 0;
    have = runtime_device_count();
  }
  if (num_gpus <= 0 || num_gpus > have) return have;
  return num_gpus;
}

// Runs fn(shard_index, device) on one host thread per device; returns the first non-OK status.
template <class Fn>
int for_each_device(int ndev, Fn fn) {
  std::vector<int> rc(ndev, SV_OK);
  std::vector<std::string> msg(ndev);
  if (ndev == 1) return fn(0, runtime_device_id(0));
  std::vector<std::thread> th;
  for (int d = 0; d < ndev; d++)
    th.emplace_back([&, d] {
      rc[d] = fn(d, runtime_device_id(d));
      if (rc[d] != SV_OK) msg[d] = sv::last_error();
    });
  for (auto& t : th) t.join();
  for (int d = 0; d < ndev; d++)
    if (rc[d] != SV_OK) {
      sv::set_error("device %d: %s", d, msg[d].c_str());
      return rc[d];
    }
  return SV_OK;
}

// Pooled device staging for the host-buffer entry points: the regions live in a leased
// workspace's grow-only input buffer (no per-call hipMalloc / hipFree); copies run on the lease's
// stream and are synchronised before the call returns.
struct Staging {
  WsLease lease;
  std::vector<char*> d;
  bool pending = false;  // async copies queued since the last sync (they may read caller memory)
  explicit Staging(int device) : lease(device, nullptr) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  // An early error return must not hand the workspace back to the pool (or free the host memory
  // a queued copy reads) while copies are still in flight.
  ~Staging() {
    if (pending && lease.ok()) (void)hipStreamSynchronize(lease.get()->stream);
  }
  int init(std::initializer_list<size_t> sizes) {
    if (!lease.ok()) return SV_ERR_DEVICE;
    size_t tot = 0;
    for (size_t s : sizes) tot += Workspace::aligned(s ? s : 1);
    SV_TRY(lease.get()->reserve_in(tot));
    char* p = lease.get()->inbuf;
    for (size_t s : sizes) {
      d.push_back(p);
      p += Workspace::aligned(s ? s : 1);
    }
    return SV_OK;
  }
  template <class T = void>
  T* at(int i) const {
    return reinterpret_cast<T*>(d[i]);
  }
  int put(int i, const void* h, size_t bytes) {
    pending = true;
    if (bytes) SV_HIP(hipMemcpyAsync(d[i], h, bytes, hipMemcpyHostToDevice, lease.get()->stream));
    return SV_OK;
  }
  int put_at(int i, size_t offset, const void* h, size_t bytes) {
    pending = true;
    if (bytes) SV_HIP(hipMemcpyAsync(d[i] + offset, h, bytes, hipMemcpyHostToDevice, lease.get()->stream));
    return SV_OK;
  }
  int get(void* h, int i, size_t bytes) {
    pending = true;
    if (bytes) SV_HIP(hipMemcpyAsync(h, d[i], bytes, hipMemcpyDeviceToHost, lease.get()->stream));
    return SV_OK;
  }
  int sync() {
    SV_HIP(hipStreamSynchronize(lease.get()->stream));
    pending = false;
    return SV_OK;
  }
};

// Small MSMs (at most kSmallMsmTerms terms each, msm.hpp) go through msm_batch_windows_host: window
// sums on the device, the window Horner on the host.  SVGPU_SMALL_MSM=0 keeps the single-MSM
// pipeline (read per call; results identical).
bool small_msm_off() {
  const char* e = getenv("SVGPU_SMALL_MSM");
  return e && atoi(e) == 0;
}

// pieces of a host-fed MSM (SVGPU_H2D_PIECES; unset = 0: the MSM plan picks, see msm_run_impl):
// piece k + 1's transfer overlaps piece k's sort and accumulation
int h2d_pieces() {
  const char* e = getenv("SVGPU_H2D_PIECES");
  if (!e) return 0;
  const int p = atoi(e);
  return p < 1 ? 1 : p;
}

#define SV_GUARD_BEGIN try {
#define SV_GUARD_END                                    \
  }                                                     \
  catch (const std::exception& e) {                     \
    sv::set_error("internal error: %s", e.what());      \
    return SV_ERR_DEVICE;                               \
  }                                                     \
  catch (...) {                                         \
    sv::set_error("internal error");                    \
    return SV_ERR_DEVICE;                               \
  }

int check_form(int form) {
  if (form != SV_CANONICAL && form != SV_MONTGOMERY) {
    sv::set_error("bad form %d", form);
    return SV_ERR_ARG;
  }
  return SV_OK;
}

}  // namespace

extern "C" {

int sv_init(int num_devices) noexcept {
  SV_GUARD_BEGIN
  return runtime_init(num_devices);
  SV_GUARD_END
}

int sv_device_count(void) noexcept {
  SV_GUARD_BEGIN
  return runtime_device_count();
  SV_GUARD_END
}

const char* sv_last_error(void) noexcept { return sv::last_error(); }

const char* sv_version(void) noexcept { return "svgpu 0.1.0 (abi 1, gfx950)"; }

int sv_bn254_g1_msm(const sv_g1_affine* bases, const sv_fe* scalars, size_t n, int form, int num_gpus,
                    sv_g1_affine* out) noexcept {
  SV_GUARD_BEGIN
  if (n == 0) {
    sv::set_error("pairs should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!bases || !scalars || !out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(form));
  int ndev = resolve_gpus(num_gpus);
  if (ndev == 0) return SV_ERR_DEVICE;
  if ((size_t)ndev > n) ndev = (int)n;
  std::vector<Xyzz> part(ndev, host::x_identity());
  size_t per = (n + ndev - 1) / ndev;
  int rc = for_each_device(ndev, [&](int k, int dev) -> int {
    size_t lo = k * per, hi = std::min(n, lo + per);
    if (lo >= hi) return SV_OK;
    MsmFeed feed;
    feed.pieces = h2d_pieces();
    // pageable caller memory: the runtime's staged DMA measured at the pinned rate (tools/ubench_h2d.cpp)
    feed.stage_scalars = [&, lo](size_t a, size_t b, void* ds, hipStream_t cs, hipEvent_t ready) -> int {
      SV_HIP(hipMemcpyAsync(ds, scalars + lo + a, (b - a) * sizeof(sv_fe), hipMemcpyHostToDevice, cs));
      SV_HIP(hipEventRecord(ready, cs));
      return SV_OK;
    };
    feed.stage_bases = [&, lo](size_t a, size_t b, void* db, hipStream_t cs, hipEvent_t ready) -> int {
      SV_HIP(hipMemcpyAsync(db, bases + lo + a, (b - a) * sizeof(sv_g1_affine), hipMemcpyHostToDevice, cs));
      SV_HIP(hipEventRecord(ready, cs));
      return SV_OK;
    };
    return msm_run_fed(hi - lo, form, dev, feed, &part[k]);
  });
  if (rc != SV_OK) return rc;
  Xyzz acc = host::x_identity();
  for (auto& p : part) acc = host::x_add(acc, p);
  affine_out(acc, form, out);
  return SV_OK;
  SV_GUARD_END
}

// references gathered this far ahead are prefetched (random 32/64-B reads are DRAM-latency bound);
// SVGPU_GATHER_AHEAD overrides (read once)
static size_t gather_ahead() {
  static const size_t a = getenv("SVGPU_GATHER_AHEAD") ? (size_t)std::max(1, atoi(getenv("SVGPU_GATHER_AHEAD"))) : 16;
  return a;
}

int sv_bn254_g1_msm_refs(const sv_msm_ref* pairs, size_t n, int form, int num_gpus, sv_g1_affine* out) noexcept {
  SV_GUARD_BEGIN
  if (n == 0) {
    sv::set_error("pairs should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!pairs || !out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(form));
  int ndev = resolve_gpus(num_gpus);
  if (ndev == 0) return SV_ERR_DEVICE;
  if ((size_t)ndev > n) ndev = (int)n;
  std::vector<Xyzz> part(ndev, host::x_identity());
  size_t per = (n + ndev - 1) / ndev;
  int rc = for_each_device(ndev, [&](int k, int dev) -> int {
    size_t lo = k * per, hi = std::min(n, lo + per);
    if (lo >= hi) return SV_OK;
    const size_t m = hi - lo;
    // the gather target: pinned staging of a leased workspace (grow-only, reused across calls)
    WsLease st_lease(dev, nullptr);
    if (!st_lease.ok()) return SV_ERR_DEVICE;
    Workspace* sw = st_lease.get();
    SV_TRY(sw->reserve_stage(m * (sizeof(sv_fe) + sizeof(sv_g1_affine))));
    sv_fe* hs = reinterpret_cast<sv_fe*>(sw->stage);
    sv_g1_affine* hb = reinterpret_cast<sv_g1_affine*>(sw->stage + m * sizeof(sv_fe));
    std::atomic<int> null_ref{0};
    MsmFeed feed;
    feed.pieces = h2d_pieces();
    // the gather paces this path: smaller first and middle pieces keep the gather, the DMA and the
    // accumulates overlapped (2^20: 2,2,3,3,3,3 3.67-3.73 ms, 4 equal pieces 3.95)
    feed.split = {2, 2, 3, 3, 3, 3};
    // gather piece [a, b) on the host pool (scalars, then bases: the scalar DMA and the piece's
    // sort overlap the base gather, and this piece's DMA the next piece's gather).  (Gathering both
    // in one pass per piece was measured slower: 3.7 -> 4.2-4.9 ms at 2^20, the sort then waits for
    // the whole piece.)
    const size_t kGatherAhead = gather_ahead();
    feed.stage_scalars = [&, lo](size_t a, size_t b, void* ds, hipStream_t cs, hipEvent_t ready) -> int {
      host_parallel_for(b - a, 8192, [&](size_t x, size_t y) {
        for (size_t i = a + x; i < a + y; i++) {
          if (i + kGatherAhead < a + y) __builtin_prefetch(pairs[lo + i + kGatherAhead].scalar);
          const sv_fe* sp = pairs[lo + i].scalar;
          if (!sp) {
            null_ref.store(1, std::memory_order_relaxed);
            memset(&hs[i], 0, sizeof(sv_fe));
          } else {
            hs[i] = *sp;
          }
        }
      });
      SV_HIP(hipMemcpyAsync(ds, hs + a, (b - a) * sizeof(sv_fe), hipMemcpyHostToDevice, cs));
      SV_HIP(hipEventRecord(ready, cs));
      return SV_OK;
    };
    feed.stage_bases = [&, lo](size_t a, size_t b, void* db, hipStream_t cs, hipEvent_t ready) -> int {
      host_parallel_for(b - a, 8192, [&](size_t x, size_t y) {
        for (size_t i = a + x; i < a + y; i++) {
          if (i + kGatherAhead < a + y) {
            const char* q = reinterpret_cast<const char*>(pairs[lo + i + kGatherAhead].base);
            __builtin_prefetch(q);
            __builtin_prefetch(q + 63);  // a 64-B point may straddle two lines
          }
          const sv_g1_affine* bp = pairs[lo + i].base;
          if (!bp) {
            null_ref.store(1, std::memory_order_relaxed);
            memset(&hb[i], 0, sizeof(sv_g1_affine));
          } else {
            hb[i] = *bp;
          }
        }
      });
      SV_HIP(hipMemcpyAsync(db, hb + a, (b - a) * sizeof(sv_g1_affine), hipMemcpyHostToDevice, cs));
      SV_HIP(hipEventRecord(ready, cs));
      return SV_OK;
    };
    int r = msm_run_fed(m, form, dev, feed, &part[k]);
    if (r == SV_OK && null_ref.load()) {
      sv::set_error("null scalar or base reference");
      return SV_ERR_ARG;
    }
    return r;
  });
  if (rc != SV_OK) return rc;
  Xyzz acc = host::x_identity();
  for (auto& p : part) acc = host::x_add(acc, p);
  affine_out(acc, form, out);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_device(const sv_g1_affine* d_bases, const sv_fe* d_scalars, size_t n, int form,
                           int device, void* stream, sv_g1_jacobian* out_partial) noexcept {
  SV_GUARD_BEGIN
  if (n == 0) {
    sv::set_error("pairs should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!d_bases || !d_scalars || !out_partial) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(form));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  Xyzz r;
  SV_TRY(msm_run_device(d_bases, d_scalars, n, form, device, caller_stream(stream), &r));
  jacobian_out(r, out_partial);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_fold(const sv_g1_jacobian* partials, size_t k, sv_g1_affine* out, int out_form) noexcept {
  SV_GUARD_BEGIN
  if (k == 0) {
    sv::set_error("no partials");
    return SV_ERR_EMPTY;
  }
  if (!partials || !out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(out_form));
  Xyzz acc = host::x_identity();
  for (size_t i = 0; i < k; i++) {
    F X = fe_in(partials[i].x), Y = fe_in(partials[i].y), Z = fe_in(partials[i].z);
    if (!host::f_is_reduced(X) || !host::f_is_reduced(Y) || !host::f_is_reduced(Z)) {
      sv::set_error("partial %zu: coordinate not reduced", i);
      return SV_ERR_ARG;
    }
    acc = host::x_add(acc, host::x_from_jacobian(host::f_to_mont(X), host::f_to_mont(Y), host::f_to_mont(Z)));
  }
  affine_out(acc, out_form, out);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_kzg_decide(const sv_g2_affine* g2, const sv_g2_affine* s_g2, const sv_g1_affine* lhs,
                        const sv_g1_affine* rhs, size_t n, int form, int num_gpus, int32_t* first_fail) noexcept {
  SV_GUARD_BEGIN
  if (n == 0) {
    sv::set_error("accumulators should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!g2 || !s_g2 || !lhs || !rhs || !first_fail) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(form));
  int ndev = resolve_gpus(num_gpus);
  if (ndev == 0) return SV_ERR_DEVICE;
  if ((size_t)ndev > n) ndev = (int)n;
  size_t per = (n + ndev - 1) / ndev;
  std::vector<int32_t> ff(ndev, -1);
  int rc = for_each_device(ndev, [&](int k, int dev) -> int {
    size_t lo = k * per, hi = std::min(n, lo + per);
    if (lo >= hi) return SV_OK;
    size_t m = hi - lo;
    Staging sg(dev);
    SV_TRY(sg.init({m * sizeof(sv_g1_affine), m * sizeof(sv_g1_affine)}));
    SV_TRY(sg.put(0, lhs + lo, m * sizeof(sv_g1_affine)));
    SV_TRY(sg.put(1, rhs + lo, m * sizeof(sv_g1_affine)));
    SV_TRY(sg.sync());
    int32_t f = -1;
    SV_TRY(decide_run_device(g2, s_g2, sg.at(0), sg.at(1), m, form, dev, nullptr, &f, nullptr, nullptr));
    ff[k] = f < 0 ? -1 : (int32_t)(lo + f);
    return SV_OK;
  });
  if (rc != SV_OK) return rc;
  *first_fail = -1;
  for (int k = 0; k < ndev; k++)
    if (ff[k] >= 0) {
      *first_fail = ff[k];
      break;
    }
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_kzg_decide_device(const sv_g2_affine* g2, const sv_g2_affine* s_g2, const sv_g1_affine* d_lhs,
                               const sv_g1_affine* d_rhs, size_t n, int form, int device, void* stream,
                               int32_t* first_fail, int32_t* verdicts, sv_fq12* gt) noexcept {
  SV_GUARD_BEGIN
  if (!g2 || !s_g2 || !d_lhs || !d_rhs) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  return decide_run_device(g2, s_g2, d_lhs, d_rhs, n, form, device, caller_stream(stream), first_fail,
                           verdicts, gt);
  SV_GUARD_END
}

int sv_bn254_kzg_accumulate(const sv_g1_affine* lhs, const sv_g1_affine* rhs, size_t n, const sv_fe* r,
                            int form, int num_gpus, sv_g1_affine* out_lhs, sv_g1_affine* out_rhs) noexcept {
  SV_GUARD_BEGIN
  (void)num_gpus;  // n is small (one scalar per accumulator): a single device suffices
  if (n == 0) {
    sv::set_error("accumulators should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!lhs || !rhs || !r || !out_lhs || !out_rhs) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(form));
  if (!host::f_is_reduced(fe_in(*r), host::R64)) {
    sv::set_error("r not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  int dev = runtime_device_id(0);
  if (n <= kSmallMsmTerms && !small_msm_off()) {
    // Round 5: the two MSMs as ONE small batch (msm_batch_windows_host): r^i on the host (n Fr
    // products, ~1 us; k_powers was a 28 us serial chain on one lane plus a synchronisation), the
    // window sums of both MSMs in one launch, the window Horner of both on the host.
    namespace fr = sv::host::fr;
    fr::E rm;
    memcpy(rm.l, r->l, 32);
    if (form != SV_MONTGOMERY) rm = fr::to_mont(rm);
    std::vector<sv_fe> pw(2 * n);
    fr::E acc = fr::one();
    for (size_t i = 0; i < n; i++) {
      memcpy(pw[i].l, acc.l, 32);
      pw[n + i] = pw[i];
      acc = fr::mul(acc, rm);
    }
    const uint64_t off[3] = {0, n, 2 * n};
    Staging sg(dev);
    SV_TRY(sg.init({2 * n * sizeof(sv_g1_affine), 2 * n * sizeof(sv_fe), sizeof off}));
    SV_TRY(sg.put(0, lhs, n * sizeof(sv_g1_affine)));
    SV_TRY(sg.put_at(0, n * sizeof(sv_g1_affine), rhs, n * sizeof(sv_g1_affine)));
    SV_TRY(sg.put(1, pw.data(), 2 * n * sizeof(sv_fe)));
    SV_TRY(sg.put(2, off, sizeof off));
    Xyzz ab[2];
    SV_TRY(msm_batch_windows_host(sg.at(0), sg.at(1), sg.at<const uint64_t>(2), 2, n, SV_MONTGOMERY, form, dev,
                                  sg.lease.get()->stream, ab));
    sg.pending = false;  // msm_batch_windows_host synchronised the stream
    affine_out(ab[0], form, out_lhs);
    affine_out(ab[1], form, out_rhs);
    return SV_OK;
  }
  Staging sg(dev);
  SV_TRY(sg.init({n * sizeof(sv_g1_affine), n * sizeof(sv_g1_affine), n * sizeof(sv_fe), sizeof(sv_fe)}));
  SV_TRY(sg.put(0, lhs, n * sizeof(sv_g1_affine)));
  SV_TRY(sg.put(1, rhs, n * sizeof(sv_g1_affine)));
  SV_TRY(sg.put(3, r, sizeof(sv_fe)));
  SV_TRY(sg.sync());
  SV_TRY(powers_device(sg.at(3), form, n, form, sg.at(2), sg.lease.get()->stream));
  SV_TRY(sg.sync());
  // the lhs and rhs MSMs share the scalars and are independent: run them concurrently (each call
  // leases its own stream + workspace), one on the caller and one on a pool worker
  Xyzz ab[2];
  int rc2[2] = {SV_OK, SV_OK};
  std::string err2[2];
  host_parallel_for(2, 1, [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      rc2[k] = msm_run_device(sg.at(k == 0 ? 0 : 1), sg.at(2), n, form, dev, nullptr, &ab[k]);
      if (rc2[k] != SV_OK) err2[k] = sv::last_error();
    }
  });
  for (int k = 0; k < 2; k++)
    if (rc2[k] != SV_OK) {
      sv::set_error("%s", err2[k].c_str());
      return rc2[k];
    }
  const Xyzz& a = ab[0];
  const Xyzz& b = ab[1];
  affine_out(a, form, out_lhs);
  affine_out(b, form, out_rhs);
  return SV_OK;
  SV_GUARD_END
}

// KzgAs::create_proof without blind (accumulation.rs:146-195): a fresh PoseidonTranscript
// (T = 3, RATE = 2, R_F = 8, R_P = 57; snark-verifier-sdk/src/halo2.rs:52-55) absorbs every lhs_i,
// rhs_i through common_ec_point (transcript/halo2.rs:214-226: the affine x and y, each Fq -> Fr by
// fe_to_fe = reduction mod r) and squeezes r (:158-176); then the two r^i MSMs.  The sponge is one
// serial chain of n + 1 permutations and runs on the host (host_poseidon.hpp: a GPU lane would
// take ~20 ms for it at n = 64); the MSMs run on the device (sv_bn254_kzg_accumulate).
int sv_bn254_kzg_create_proof(const sv_g1_affine* lhs, const sv_g1_affine* rhs, size_t n, int form, int num_gpus,
                              sv_g1_affine* out_lhs, sv_g1_affine* out_rhs, sv_fe* sponge_state,
                              sv_fe* out_r) noexcept {
  SV_GUARD_BEGIN
  if (n == 0) {
    sv::set_error("accumulators should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!lhs || !rhs || !out_lhs || !out_rhs) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(check_form(form));
  namespace fr = sv::host::fr;
  fr::Sponge3 sponge;
  if (sponge_state) {
    for (int k = 0; k < 3; k++) {
      fr::E e;
      memcpy(e.l, sponge_state[k].l, 32);
      if (!fr::is_reduced(e)) {
        sv::set_error("sponge_state[%d] not reduced mod r", k);
        return SV_ERR_ARG;
      }
      sponge.st[k] = form == SV_MONTGOMERY ? e : fr::to_mont(e);
    }
  }
  sponge.buf.reserve(4 * n);
  for (size_t i = 0; i < n; i++) {
    for (const sv_g1_affine* pt : {&lhs[i], &rhs[i]}) {
      F x = fe_in(pt->x), y = fe_in(pt->y);
      if (host::f_is_zero(x) && host::f_is_zero(y)) {
        // coordinates() of the identity is None -> Error::Transcript (halo2.rs:215-223)
        sv::set_error("Invalid elliptic curve point encoding in proof (accumulator %zu is the identity)", i);
        return SV_ERR_ARG;
      }
      if (!host::f_is_reduced(x) || !host::f_is_reduced(y)) {
        sv::set_error("accumulator %zu: coordinate not reduced mod p", i);
        return SV_ERR_ARG;
      }
      if (form == SV_MONTGOMERY) x = host::f_from_mont(x), y = host::f_from_mont(y);
      for (const F& c : {x, y}) {
        fr::E e;
        memcpy(e.l, c.l, 32);
        sponge.update(fr::to_mont(fr::reduce_below_2r(e)));  // fe_to_fe: canonical Fq mod r
      }
    }
  }
  const fr::E rm = sponge.squeeze();
  const fr::E rv = form == SV_MONTGOMERY ? rm : fr::from_mont(rm);
  sv_fe r;
  memcpy(r.l, rv.l, 32);
  const int rc = sv_bn254_kzg_accumulate(lhs, rhs, n, &r, form, num_gpus, out_lhs, out_rhs);
  if (rc != SV_OK) return rc;
  if (out_r) *out_r = r;
  if (sponge_state)
    for (int k = 0; k < 3; k++) {
      const fr::E e = form == SV_MONTGOMERY ? sponge.st[k] : fr::from_mont(sponge.st[k]);
      memcpy(sponge_state[k].l, e.l, 32);
    }
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_batch(const sv_g1_affine* bases, const sv_fe* scalars, const uint64_t* offsets, size_t count,
                          int form, sv_g1_affine* out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (count == 0) return SV_OK;
  if (!offsets || !out) return SV_ERR_ARG;
  for (size_t k = 0; k < count; k++) {
    if (offsets[k + 1] < offsets[k]) {
      sv::set_error("msm_batch: offsets not non-decreasing at %zu", k);
      return SV_ERR_ARG;
    }
    if (offsets[k + 1] == offsets[k]) {
      sv::set_error("pairs should not be empty (msm %zu)", k);
      return SV_ERR_EMPTY;
    }
  }
  if (!bases || !scalars) return SV_ERR_ARG;
  if (count > 0x7fffffffull) return SV_ERR_LEN;
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  const int dev = runtime_device_id(0);
  const uint64_t base = offsets[0], total = offsets[count] - base;
  std::vector<uint64_t> off(offsets, offsets + count + 1);
  for (auto& o : off) o -= base;
  // the long MSMs go through the single-MSM pipeline one by one, the others stay in the batch
  std::vector<uint32_t> small_ids, big_ids;
  size_t max_small = 0;
  batch_split(off.data(), count, batch_tuning(), &small_ids, &big_ids, &max_small);
  Staging sg(dev);
  SV_TRY(sg.init({total * sizeof(sv_g1_affine), total * sizeof(sv_fe), (count + 1) * sizeof(uint64_t),
                  count * sizeof(uint32_t), count * sizeof(sv_g1_affine)}));
  SV_TRY(sg.put(0, bases + base, total * sizeof(sv_g1_affine)));
  SV_TRY(sg.put(1, scalars + base, total * sizeof(sv_fe)));
  SV_TRY(sg.put(2, off.data(), (count + 1) * sizeof(uint64_t)));
  SV_TRY(sg.put(3, small_ids.data(), small_ids.size() * sizeof(uint32_t)));
  SV_TRY(sg.sync());
  if (!small_ids.empty()) {
    // every MSM small: no id map (the ids would be the identity), which the small-batch route needs
    const uint32_t* ids = big_ids.empty() ? nullptr : sg.at<const uint32_t>(3);
    SV_TRY(msm_batch_device(sg.at(0), sg.at(1), sg.at<const uint64_t>(2), ids, small_ids.size(), max_small, form, dev,
                            nullptr, sg.at(4)));
    SV_TRY(sg.get(out, 4, count * sizeof(sv_g1_affine)));
    SV_TRY(sg.sync());
  }
  for (uint32_t k : big_ids) {
    Xyzz r;
    SV_TRY(msm_run_device(sg.at<const sv_g1_affine>(0) + off[k], sg.at<const sv_fe>(1) + off[k],
                          off[k + 1] - off[k], form, dev, nullptr, &r));
    affine_out(r, form, &out[k]);
  }
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_batch_device(const sv_g1_affine* d_bases, const sv_fe* d_scalars, const uint64_t* d_offsets,
                                 size_t count, size_t max_terms, int form, int device, void* stream,
                                 sv_g1_affine* d_out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (count == 0) return SV_OK;
  if (!d_bases || !d_scalars || !d_offsets || !d_out) return SV_ERR_ARG;
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  SV_HIP(hipSetDevice(device));
  return msm_batch_device(d_bases, d_scalars, d_offsets, nullptr, count, max_terms, form, device, caller_stream(stream),
                          d_out);
  SV_GUARD_END
}

// ---- fixed-base tables (device-resident constant bases for batched MSMs) -------------------
namespace {
struct BaseTable {
  int dev = 0;
  void* p = nullptr;    // rows (Montgomery affine)
  void* pre = nullptr;  // rows expanded to their window multiples 2^(8 w) P (msm_batch_fixed_device)
  size_t n = 0;
};
std::mutex g_tables_mu;
std::unordered_map<uint64_t, BaseTable> g_tables;
uint64_t g_next_table = 1;

bool table_lookup(uint64_t h, BaseTable* out) {
  std::lock_guard<std::mutex> lk(g_tables_mu);
  auto it = g_tables.find(h);
  if (it == g_tables.end()) return false;
  *out = it->second;
  return true;
}

int check_offsets(const uint64_t* offsets, size_t count) {
  for (size_t k = 0; k < count; k++) {
    if (offsets[k + 1] < offsets[k]) {
      sv::set_error("msm_batch: offsets not non-decreasing at %zu", k);
      return SV_ERR_ARG;
    }
    if (offsets[k + 1] == offsets[k]) {
      sv::set_error("pairs should not be empty (msm %zu)", k);
      return SV_ERR_EMPTY;
    }
  }
  return SV_OK;
}
}  // namespace

int sv_bn254_g1_table_create(const sv_g1_affine* bases, size_t n, int form, int device, uint64_t* handle) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!handle || (!bases && n)) return SV_ERR_ARG;
  if (n == 0) {
    sv::set_error("empty base table");
    return SV_ERR_EMPTY;
  }
  if (n > 0xffffffffull) return SV_ERR_LEN;
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  if (device < 0 || device >= runtime_device_count()) {
    sv::set_error("device %d not initialised", device);
    return SV_ERR_ARG;
  }
  const int dev = runtime_device_id(device);
  // Montgomery form on the device; coordinates must be reduced (as for every MSM input)
  std::vector<sv_g1_affine> mont(n);
  for (size_t i = 0; i < n; i++) {
    F x, y;
    memcpy(x.l, bases[i].x.l, 32);
    memcpy(y.l, bases[i].y.l, 32);
    if (!sv::host::f_is_reduced(x) || !sv::host::f_is_reduced(y)) {
      sv::set_error("base table row %zu: coordinate not reduced mod p", i);
      return SV_ERR_ARG;
    }
    const bool ident = sv::host::f_is_zero(x) && sv::host::f_is_zero(y);
    if (form == SV_CANONICAL && !ident) {
      x = sv::host::f_to_mont(x);
      y = sv::host::f_to_mont(y);
    }
    memcpy(mont[i].x.l, x.l, 32);
    memcpy(mont[i].y.l, y.l, 32);
  }
  BaseTable t;
  t.dev = dev;
  t.n = n;
  SV_HIP(hipSetDevice(dev));
  SV_HIP(hipMalloc(&t.p, n * sizeof(sv_g1_affine)));
  if (hipMalloc(&t.pre, table_precomputed_rows_bytes(n)) != hipSuccess) {
    (void)hipFree(t.p);
    sv::set_error("base table: precomputed rows hipMalloc failed");
    return SV_ERR_OOM;
  }
  int prc = hipMemcpy(t.p, mont.data(), n * sizeof(sv_g1_affine), hipMemcpyHostToDevice) == hipSuccess
                ? table_precompute_device(t.p, n, t.pre, dev)
                : SV_ERR_DEVICE;
  if (prc != SV_OK) {
    (void)hipFree(t.p);
    (void)hipFree(t.pre);
    sv::set_error("base table upload / precompute failed");
    return prc;
  }
  std::lock_guard<std::mutex> lk(g_tables_mu);
  *handle = g_next_table++;
  g_tables[*handle] = t;
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_table_destroy(uint64_t handle) noexcept {
  SV_GUARD_BEGIN
  BaseTable t;
  {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    auto it = g_tables.find(handle);
    if (it == g_tables.end()) {
      sv::set_error("unknown base table handle %llu", (unsigned long long)handle);
      return SV_ERR_ARG;
    }
    t = it->second;
    g_tables.erase(it);
  }
  SV_HIP(hipSetDevice(t.dev));
  SV_HIP(hipFree(t.p));
  SV_HIP(hipFree(t.pre));
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_batch_table(uint64_t handle, const uint32_t* base_idx, const sv_fe* scalars,
                                const uint64_t* offsets, size_t count, int form, sv_g1_affine* out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (count == 0) return SV_OK;
  if (!offsets || !out) return SV_ERR_ARG;
  SV_TRY(check_offsets(offsets, count));
  if (!base_idx || !scalars) return SV_ERR_ARG;
  if (count > 0x7fffffffull) return SV_ERR_LEN;
  BaseTable t;
  if (!table_lookup(handle, &t)) {
    sv::set_error("unknown base table handle %llu", (unsigned long long)handle);
    return SV_ERR_ARG;
  }
  const uint64_t base = offsets[0], total = offsets[count] - base;
  size_t max_terms = 0;
  std::vector<uint64_t> off(offsets, offsets + count + 1);
  for (auto& o : off) o -= base;
  for (size_t k = 0; k < count; k++) max_terms = std::max<size_t>(max_terms, off[k + 1] - off[k]);
  for (uint64_t i = 0; i < total; i++)
    if (base_idx[base + i] >= t.n) {
      sv::set_error("msm_batch: base index %u at term %llu out of the table (%zu rows)", base_idx[base + i],
                    (unsigned long long)(base + i), t.n);
      return SV_ERR_ARG;
    }
  Staging sg(t.dev);
  SV_TRY(sg.init({total * sizeof(uint32_t), total * sizeof(sv_fe), (count + 1) * sizeof(uint64_t),
                  count * sizeof(sv_g1_affine)}));
  SV_TRY(sg.put(0, base_idx + base, total * sizeof(uint32_t)));
  SV_TRY(sg.put(1, scalars + base, total * sizeof(sv_fe)));
  SV_TRY(sg.put(2, off.data(), (count + 1) * sizeof(uint64_t)));
  SV_TRY(sg.sync());
  (void)max_terms;
  SV_TRY(msm_batch_fixed_device(t.pre, t.n, sg.at<const uint32_t>(0), sg.at(1), sg.at<const uint64_t>(2), count, form,
                                t.dev, nullptr, sg.at(3)));
  SV_TRY(sg.get(out, 3, count * sizeof(sv_g1_affine)));
  SV_TRY(sg.sync());
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_batch_table_device(uint64_t handle, const uint32_t* d_base_idx, const sv_fe* d_scalars,
                                       const uint64_t* d_offsets, size_t count, int form, void* stream,
                                       sv_g1_affine* d_out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (count == 0) return SV_OK;
  if (!d_base_idx || !d_scalars || !d_offsets || !d_out) return SV_ERR_ARG;
  BaseTable t;
  if (!table_lookup(handle, &t)) {
    sv::set_error("unknown base table handle %llu", (unsigned long long)handle);
    return SV_ERR_ARG;
  }
  SV_HIP(hipSetDevice(t.dev));
  return msm_batch_fixed_device(t.pre, t.n, d_base_idx, d_scalars, d_offsets, count, form, t.dev,
                                caller_stream(stream), d_out);
  SV_GUARD_END
}

int sv_bn254_g1_table_device(uint64_t handle, int* device) noexcept {
  SV_GUARD_BEGIN
  BaseTable t;
  if (!device || !table_lookup(handle, &t)) {
    sv::set_error("unknown base table handle %llu", (unsigned long long)handle);
    return SV_ERR_ARG;
  }
  *device = t.dev;
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_batch_indexed_device(const sv_g1_affine* d_table, size_t table_len, int table_form,
                                         const uint32_t* d_base_idx, const sv_fe* d_scalars,
                                         const uint64_t* d_offsets, size_t count, size_t max_terms, int form,
                                         int device, void* stream, sv_g1_affine* d_out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  SV_TRY(check_form(table_form));
  if (count == 0) return SV_OK;
  if (!d_table || !d_base_idx || !d_scalars || !d_offsets || !d_out) return SV_ERR_ARG;
  if (table_len == 0) {
    sv::set_error("empty base table");
    return SV_ERR_EMPTY;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  SV_HIP(hipSetDevice(device));
  return msm_batch_device(d_table, d_scalars, d_offsets, nullptr, count, max_terms, form, device,
                          caller_stream(stream), d_out, d_base_idx, table_len, table_form);
  SV_GUARD_END
}

// ---- resident base sets (upload once, ship only scalars per MSM call) -----------------------
namespace {
struct BaseSet {
  int index = 0;         // the logical device the caller asked for
  int dev = 0;           // its HIP ordinal
  void* rows = nullptr;  // n Montgomery rows
  void* vtab = nullptr;  // 2 n records of the 29-bit table (msm.hpp)
  size_t n = 0;
};
// handles come from the base tables' counter, so no number is ever both a table and a set
std::unordered_map<uint64_t, BaseSet> g_sets;

constexpr size_t kMaxSetRows = size_t(1) << 26;

bool set_lookup(uint64_t h, BaseSet* out) {
  std::lock_guard<std::mutex> lk(g_tables_mu);
  auto it = g_sets.find(h);
  if (it == g_sets.end()) {
    sv::set_error("unknown base set handle %llu", (unsigned long long)h);
    return false;
  }
  *out = it->second;
  return true;
}

// checks shared by the two create variants; nothing touches a device before they pass
int set_create_args(const void* bases, size_t n, int form, const uint64_t* handle) {
  SV_TRY(check_form(form));
  if (!handle || !bases) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (n == 0) {
    sv::set_error("empty base set");
    return SV_ERR_EMPTY;
  }
  if (n > kMaxSetRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26 (one set per device over its shard)", n);
    return SV_ERR_LEN;
  }
  return SV_OK;
}

// rows: host rows (from_device = false, uploaded) or rows in HBM on the set's device
int set_create(const sv_g1_affine* rows, bool from_device, size_t n, int form, int device, hipStream_t stream,
               uint64_t* handle) {
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  if (device < 0 || device >= runtime_device_count()) {
    sv::set_error("device %d not initialised", device);
    return SV_ERR_ARG;
  }
  BaseSet t;
  t.index = device;
  t.dev = runtime_device_id(device);
  t.n = n;
  SV_HIP(hipSetDevice(t.dev));
  if (hipMalloc(&t.rows, n * kResidentRowBytes) != hipSuccess ||
      hipMalloc(&t.vtab, n * kResidentTabBytes) != hipSuccess) {
    (void)hipGetLastError();
    if (t.rows) (void)hipFree(t.rows);
    sv::set_error("base set: hipMalloc of %zu rows failed", n);
    return SV_ERR_OOM;
  }
  int rc = SV_OK;
  if (!from_device && hipMemcpy(t.rows, rows, n * sizeof(sv_g1_affine), hipMemcpyHostToDevice) != hipSuccess) {
    sv::set_error("base set upload failed");
    rc = SV_ERR_DEVICE;
  }
  if (rc == SV_OK) rc = msm_resident_prepare(from_device ? (const void*)rows : t.rows, n, form, t.dev, stream, t.rows, t.vtab);
  if (rc != SV_OK) {  // no handle, nothing kept
    (void)hipFree(t.rows);
    (void)hipFree(t.vtab);
    return rc;
  }
  std::lock_guard<std::mutex> lk(g_tables_mu);
  *handle = g_next_table++;
  g_sets[*handle] = t;
  return SV_OK;
}

// the MSM calls' checks, in order: form / null, empty, length, handle, range (no device touched)
int set_call_args(uint64_t handle, size_t offset, const void* scalars, size_t n, int form, const void* out,
                  BaseSet* t) {
  SV_TRY(check_form(form));
  if (!scalars || !out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (n == 0) {
    sv::set_error("pairs should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > kMaxSetRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26 (shard across devices/calls)", n);
    return SV_ERR_LEN;
  }
  if (!set_lookup(handle, t)) return SV_ERR_ARG;
  if (offset > t->n || n > t->n - offset) {  // offset + n > N without the sum
    sv::set_error("rows [%zu, %zu + %zu) reach past base set %llu (%zu rows)", offset, offset, n,
                  (unsigned long long)handle, t->n);
    return SV_ERR_ARG;
  }
  return SV_OK;
}
}  // namespace

int sv_bn254_g1_bases_create(const sv_g1_affine* bases, size_t n, int form, int device, uint64_t* handle) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(set_create_args(bases, n, form, handle));
  return set_create(bases, false, n, form, device, nullptr, handle);
  SV_GUARD_END
}

int sv_bn254_g1_bases_create_device(const sv_g1_affine* d_bases, size_t n, int form, int device, void* stream,
                                    uint64_t* handle) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(set_create_args(d_bases, n, form, handle));
  return set_create(d_bases, true, n, form, device, caller_stream(stream), handle);
  SV_GUARD_END
}

int sv_bn254_g1_bases_destroy(uint64_t handle) noexcept {
  SV_GUARD_BEGIN
  BaseSet t;
  {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    auto it = g_sets.find(handle);
    if (it == g_sets.end()) {
      sv::set_error("unknown base set handle %llu", (unsigned long long)handle);
      return SV_ERR_ARG;
    }
    t = it->second;
    g_sets.erase(it);
  }
  SV_HIP(hipSetDevice(t.dev));
  SV_HIP(hipFree(t.rows));
  SV_HIP(hipFree(t.vtab));
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_bases_info(uint64_t handle, uint64_t* n, int* device, uint64_t* device_bytes) noexcept {
  SV_GUARD_BEGIN
  BaseSet t;
  if (!set_lookup(handle, &t)) return SV_ERR_ARG;
  if (n) *n = t.n;
  if (device) *device = t.index;
  if (device_bytes) *device_bytes = (uint64_t)t.n * (kResidentRowBytes + kResidentTabBytes);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_bases(uint64_t handle, size_t offset, const sv_fe* scalars, size_t n, int form,
                          sv_g1_affine* out) noexcept {
  SV_GUARD_BEGIN
  BaseSet t;
  SV_TRY(set_call_args(handle, offset, scalars, n, form, out, &t));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  MsmFeed feed;
  feed.pieces = h2d_pieces();
  // Piece schedule.  sv_bn254_g1_msm's (5,4,4,3 from 2^18, 2 equal from 2^15) was tuned for a 96-B
  // copy that outlasts the accumulates; a 32-B copy does not, so what counts here is a small first
  // piece (the accumulates start early) and few pieces (each accumulate is more efficient).  Swept
  // with tools/resident_bench.py --sweep (profiles/resident_bases_ab.log, ms per call, three passes):
  //   2^20: 1,3,4 1.91-1.93  1,2,5 1.92-1.93  1,3 1.98-2.02  2 equal 2.03-2.06  4 equal 2.02-2.06
  //         5,4,4,3 2.12-2.15  1,7 2.14-2.17  1 piece 2.25-2.26
  //   2^18: 1,3 1.39  1,7 1.39-1.40  2 equal 1.42  1,2,5 1.43  1 piece 1.47  5,4,4,3 1.60
  //   2^16: 1 piece 0.74  1,2 0.78  1,7 0.78  1,3 0.82  2 equal 0.92  4 pieces 0.95
  // so: one piece below 2^18 terms, 1,3 from there, 1,3,4 from 2^20 (the sizes between were not
  // measured).  SVGPU_H2D_PIECES / SVGPU_H2D_SPLIT override it as for the other host entry points.
  if (feed.pieces == 0 && n < (size_t(1) << 18)) feed.pieces = 1;
  if (n >= (size_t(1) << 20)) feed.split = {1, 3, 4};
  else feed.split = {1, 3};
  feed.stage_scalars = [&](size_t a, size_t b, void* ds, hipStream_t cs, hipEvent_t ready) -> int {
    SV_HIP(hipMemcpyAsync(ds, scalars + a, (b - a) * sizeof(sv_fe), hipMemcpyHostToDevice, cs));
    SV_HIP(hipEventRecord(ready, cs));
    return SV_OK;
  };
  const MsmResident set{t.rows, t.vtab, t.n, offset};
  Xyzz r;
  SV_TRY(msm_run_resident_fed(set, n, form, t.dev, feed, &r));
  affine_out(r, form, out);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_msm_bases_device(uint64_t handle, size_t offset, const sv_fe* d_scalars, size_t n, int form,
                                 void* stream, sv_g1_jacobian* out_partial) noexcept {
  SV_GUARD_BEGIN
  BaseSet t;
  SV_TRY(set_call_args(handle, offset, d_scalars, n, form, out_partial, &t));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  const MsmResident set{t.rows, t.vtab, t.n, offset};
  Xyzz r;
  SV_TRY(msm_run_resident_device(set, d_scalars, n, form, t.dev, caller_stream(stream), &r));
  jacobian_out(r, out_partial);
  return SV_OK;
  SV_GUARD_END
}

// ---- KZG opening on a resident base set (division on the device, witness through the set's MSM) ----
namespace {
// the division's and the openings' checks up to z, in order: form / null, empty, length, z (no
// device touched); d_quotient is not among the pointers (NULL = evaluate only)
int div_call_args(const void* coeffs, size_t n, const sv_fe* z, int form, const void* out_eval, const void* out) {
  SV_TRY(check_form(form));
  if (!coeffs || !z || !out_eval || !out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (n == 0) {
    sv::set_error("polynomial should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > kMaxSetRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26", n);
    return SV_ERR_LEN;
  }
  if (!host::f_is_reduced(fe_in(*z), host::R64)) {
    sv::set_error("z not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  return SV_OK;
}

// then the handle and the range of the n - 1 quotient terms (offset + (n - 1) > N without the sum)
int open_call_args(uint64_t handle, size_t offset, const void* coeffs, size_t n, const sv_fe* z, int form,
                   const void* out_eval, const void* out, BaseSet* t) {
  SV_TRY(div_call_args(coeffs, n, z, form, out_eval, out));
  if (!set_lookup(handle, t)) return SV_ERR_ARG;
  if (offset > t->n || n - 1 > t->n - offset) {
    sv::set_error("rows [%zu, %zu + %zu) reach past base set %llu (%zu rows)", offset, offset, n - 1,
                  (unsigned long long)handle, t->n);
    return SV_ERR_ARG;
  }
  return SV_OK;
}

// A leased workspace whose stream is drained before the lease goes back to the pool, whatever the
// exit path: the division's kernels and copies may still be in flight on an early error return.
struct DrainedLease {
  WsLease lease;
  bool armed = true;
  DrainedLease(int device, hipStream_t stream) : lease(device, stream) {}
  ~DrainedLease() {
    if (armed && lease.ok()) (void)hipStreamSynchronize(lease.get()->stream);
  }
  Workspace* ws() { return lease.get(); }
};

// the division's head (kzg_open.hpp) once the stream has drained: the error flag, then p(z)
int div_result(const char* head, sv_fe* out_eval) {
  uint32_t errv;
  memcpy(&errv, head + kDivErrOffset, 4);
  if (errv) {
    sv::set_error("invalid input: coefficient not reduced mod r");
    return SV_ERR_ARG;
  }
  memcpy(out_eval->l, head + kDivEvalOffset, sizeof(sv_fe));
  return SV_OK;
}

// Both openings: coefficients from the host (one transfer into the pooled input buffer) or in HBM,
// the quotient into pooled scratch in Montgomery form, the set's MSM over it on the same stream.
int open_run(const BaseSet& t, size_t offset, const sv_fe* coeffs, bool from_device, size_t n, const sv_fe* z,
             int form, hipStream_t stream, sv_fe* out_eval, Xyzz* witness) {
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(t.dev, stream);
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  const size_t cbytes = from_device ? 0 : Workspace::aligned(n * sizeof(sv_fe));
  SV_TRY(ws->reserve_in(cbytes + Workspace::aligned((n - 1) * sizeof(sv_fe) + 1)));
  SV_TRY(ws->reserve(poly_div_scratch_bytes(n)));
  SV_TRY(ws->reserve_pinned(kDivHeadBytes));
  const void* d_coeffs = coeffs;
  if (!from_device) {
    SV_HIP(hipMemcpyAsync(ws->inbuf, coeffs, n * sizeof(sv_fe), hipMemcpyHostToDevice, ws->stream));
    d_coeffs = ws->inbuf;
  }
  void* d_quot = ws->inbuf + cbytes;
  SV_TRY(poly_div_linear_enqueue(d_coeffs, n, *z, form, SV_MONTGOMERY, d_quot, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf, kDivHeadBytes, hipMemcpyDeviceToHost, ws->stream));
  *witness = host::x_identity();
  if (n > 1) {  // the MSM synchronises the stream, so the head has landed when it returns
    const MsmResident set{t.rows, t.vtab, t.n, offset};
    SV_TRY(msm_run_resident_device(set, d_quot, n - 1, SV_MONTGOMERY, t.dev, ws->stream, witness));
  } else {
    SV_HIP(hipStreamSynchronize(ws->stream));
  }
  dl.armed = false;
  return div_result(ws->pinned, out_eval);
}
}  // namespace

int sv_bn254_fr_poly_div_linear_device(const sv_fe* d_coeffs, size_t n, const sv_fe* z, int form, int device,
                                       void* stream, sv_fe* d_quotient, sv_fe* out_eval) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(div_call_args(d_coeffs, n, z, form, out_eval, out_eval));
  const uintptr_t cb = (uintptr_t)d_coeffs, qb = (uintptr_t)d_quotient;
  if (d_quotient && qb < cb + n * sizeof(sv_fe) && cb < qb + (n - 1) * sizeof(sv_fe)) {
    sv::set_error("d_quotient overlaps d_coeffs (phase 3 reads the coefficients again while it writes)");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  SV_TRY(ws->reserve(poly_div_scratch_bytes(n)));
  SV_TRY(ws->reserve_pinned(kDivHeadBytes));
  SV_TRY(poly_div_linear_enqueue(d_coeffs, n, *z, form, form, d_quotient, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf, kDivHeadBytes, hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  return div_result(ws->pinned, out_eval);
  SV_GUARD_END
}

int sv_bn254_kzg_open(uint64_t handle, size_t offset, const sv_fe* coeffs, size_t n, const sv_fe* z, int form,
                      sv_fe* out_eval, sv_g1_affine* out_witness) noexcept {
  SV_GUARD_BEGIN
  BaseSet t;
  SV_TRY(open_call_args(handle, offset, coeffs, n, z, form, out_eval, out_witness, &t));
  Xyzz w;
  SV_TRY(open_run(t, offset, coeffs, false, n, z, form, nullptr, out_eval, &w));
  affine_out(w, form, out_witness);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_kzg_open_device(uint64_t handle, size_t offset, const sv_fe* d_coeffs, size_t n, const sv_fe* z,
                             int form, void* stream, sv_fe* out_eval, sv_g1_jacobian* out_witness_partial) noexcept {
  SV_GUARD_BEGIN
  BaseSet t;
  SV_TRY(open_call_args(handle, offset, d_coeffs, n, z, form, out_eval, out_witness_partial, &t));
  Xyzz w;
  SV_TRY(open_run(t, offset, d_coeffs, true, n, z, form, caller_stream(stream), out_eval, &w));
  jacobian_out(w, out_witness_partial);
  return SV_OK;
  SV_GUARD_END
}

// ---- several polynomials at one point (GWC19's point sets): one pass, one division, one witness MSM ----
namespace {
// the batch's checks up to v, in order: form / null / alignment, empty, length, z, v (no device
// touched).  Only the first SV_OPEN_BATCH_MAX entries of the arrays are looked at: a longer batch is
// refused by its m.  *N = the longest length.
int batch_call_args(const sv_fe* const* d_polys, const uint64_t* lens, size_t m, const sv_fe* z, const sv_fe* v,
                    int form, const void* out_evals, const void* out, size_t* N) {
  SV_TRY(check_form(form));
  if (!d_polys || !lens || !z || !v || !out_evals || !out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  const size_t seen = std::min<size_t>(m, SV_OPEN_BATCH_MAX);
  for (size_t j = 0; j < seen; j++) {
    if (!d_polys[j]) {
      sv::set_error("null pointer (polynomial %zu)", j);
      return SV_ERR_ARG;
    }
    if ((uintptr_t)d_polys[j] % 16) {
      sv::set_error("polynomial %zu is not 16-byte aligned", j);
      return SV_ERR_ARG;
    }
  }
  if (m == 0) {
    sv::set_error("batch should not be empty");
    return SV_ERR_EMPTY;
  }
  for (size_t j = 0; j < seen; j++)
    if (lens[j] == 0) {
      sv::set_error("polynomial should not be empty (polynomial %zu)", j);
      return SV_ERR_EMPTY;
    }
  if (m > SV_OPEN_BATCH_MAX) {
    sv::set_error("m = %zu exceeds the per-call limit of %d polynomials", m, SV_OPEN_BATCH_MAX);
    return SV_ERR_LEN;
  }
  size_t longest = 0;
  for (size_t j = 0; j < m; j++) {
    if (lens[j] > kMaxSetRows) {
      sv::set_error("n = %llu exceeds the per-device limit 2^26 (polynomial %zu)", (unsigned long long)lens[j], j);
      return SV_ERR_LEN;
    }
    longest = std::max<size_t>(longest, lens[j]);
  }
  if (!host::f_is_reduced(fe_in(*z), host::R64)) {
    sv::set_error("z not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  if (!host::f_is_reduced(fe_in(*v), host::R64)) {
    sv::set_error("v not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  *N = longest;
  return SV_OK;
}

// The pass on a leased workspace: the table goes up from pinned staging in one copy on the call's
// stream, the head (flag, evaluations) comes back behind the kernels.  ws->buf must hold
// batch_device_bytes(m, N) from `at`; the pinned staging is reserved here.  Nothing is synchronised:
// batch_result reads the head once the stream has drained.
size_t batch_table_bytes(size_t m) { return Workspace::aligned(m * sizeof(BatchRow)); }
size_t batch_device_bytes(size_t m, size_t N) {
  return batch_table_bytes(m) + Workspace::aligned(poly_batch_scratch_bytes(m, N));
}
int batch_enqueue(Workspace* ws, size_t at, const sv_fe* const* d_polys, const uint64_t* lens, size_t m, size_t N,
                  const sv_fe* z, const sv_fe* v, int form, int c_form, void* d_combined) {
  const size_t tb = batch_table_bytes(m);
  SV_TRY(ws->reserve_pinned(tb + poly_batch_head_bytes(m)));
  BatchRow* rows = reinterpret_cast<BatchRow*>(ws->pinned);
  poly_batch_fill_table(rows, d_polys, lens, m, *v, form);
  char* d_table = ws->buf + at;
  char* d_scratch = d_table + tb;
  SV_HIP(hipMemcpyAsync(d_table, rows, m * sizeof(BatchRow), hipMemcpyHostToDevice, ws->stream));
  SV_TRY(poly_combine_eval_enqueue(reinterpret_cast<const BatchRow*>(d_table), m, N, *z, form, c_form, d_combined,
                                   d_scratch, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned + tb, d_scratch, poly_batch_head_bytes(m), hipMemcpyDeviceToHost, ws->stream));
  return SV_OK;
}

int batch_result(const Workspace* ws, size_t m, sv_fe* out_evals) {
  const char* head = ws->pinned + batch_table_bytes(m);
  uint32_t errv;
  memcpy(&errv, head + kBatchErrOffset, 4);
  if (errv) {
    sv::set_error("invalid input: coefficient not reduced mod r");
    return SV_ERR_ARG;
  }
  memcpy(out_evals, head + kBatchEvalsOffset, m * sizeof(sv_fe));
  return SV_OK;
}
}  // namespace

int sv_bn254_fr_poly_combine_eval_device(const sv_fe* const* d_polys, const uint64_t* lens, size_t m, const sv_fe* z,
                                         const sv_fe* v, int form, int device, void* stream, sv_fe* d_combined,
                                         sv_fe* out_evals) noexcept {
  SV_GUARD_BEGIN
  size_t N = 0;
  SV_TRY(batch_call_args(d_polys, lens, m, z, v, form, out_evals, out_evals, &N));
  if (d_combined) {
    const uintptr_t cb = (uintptr_t)d_combined;
    if (cb % 16) {
      sv::set_error("d_combined is not 16-byte aligned");
      return SV_ERR_ARG;
    }
    for (size_t j = 0; j < m; j++) {
      const uintptr_t pb = (uintptr_t)d_polys[j];
      if (cb < pb + lens[j] * sizeof(sv_fe) && pb < cb + N * sizeof(sv_fe)) {
        sv::set_error("d_combined overlaps polynomial %zu (other blocks still read it while one writes)", j);
        return SV_ERR_ARG;
      }
    }
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  SV_TRY(ws->reserve(batch_device_bytes(m, N)));
  SV_TRY(batch_enqueue(ws, 0, d_polys, lens, m, N, z, v, form, form, d_combined));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  return batch_result(ws, m, out_evals);
  SV_GUARD_END
}

int sv_bn254_kzg_open_batch_device(uint64_t handle, size_t offset, const sv_fe* const* d_polys, const uint64_t* lens,
                                   size_t m, const sv_fe* z, const sv_fe* v, int form, void* stream, sv_fe* out_evals,
                                   sv_g1_jacobian* out_witness_partial) noexcept {
  SV_GUARD_BEGIN
  size_t N = 0;
  SV_TRY(batch_call_args(d_polys, lens, m, z, v, form, out_evals, out_witness_partial, &N));
  BaseSet t;
  if (!set_lookup(handle, &t)) return SV_ERR_ARG;
  if (offset > t.n || N - 1 > t.n - offset) {
    sv::set_error("rows [%zu, %zu + %zu) reach past base set %llu (%zu rows)", offset, offset, N - 1,
                  (unsigned long long)handle, t.n);
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(t.dev, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  // pooled scratch: the table and the pass's totals, then the division's; c and q side by side in
  // the input buffer (the division reads c again while it writes q), both in Montgomery form
  const size_t cbytes = Workspace::aligned(N * sizeof(sv_fe));
  const size_t bbytes = batch_device_bytes(m, N);
  SV_TRY(ws->reserve_in(cbytes + Workspace::aligned((N - 1) * sizeof(sv_fe) + 1)));
  SV_TRY(ws->reserve(bbytes + Workspace::aligned(poly_div_scratch_bytes(N))));
  void* d_comb = ws->inbuf;
  void* d_quot = ws->inbuf + cbytes;
  SV_TRY(batch_enqueue(ws, 0, d_polys, lens, m, N, z, v, form, SV_MONTGOMERY, N > 1 ? d_comb : nullptr));
  Xyzz w = host::x_identity();
  if (N > 1) {  // the MSM synchronises the stream, so the head has landed when it returns
    const sv_fe zm = form == SV_MONTGOMERY ? *z : poly_fr_to_mont(*z);  // c is Montgomery, so z goes with it
    SV_TRY(poly_div_linear_enqueue(d_comb, N, zm, SV_MONTGOMERY, SV_MONTGOMERY, d_quot, ws->buf + bbytes, ws->stream));
    const MsmResident set{t.rows, t.vtab, t.n, offset};
    SV_TRY(msm_run_resident_device(set, d_quot, N - 1, SV_MONTGOMERY, t.dev, ws->stream, &w));
  } else {
    SV_HIP(hipStreamSynchronize(ws->stream));
  }
  dl.armed = false;
  SV_TRY(batch_result(ws, m, out_evals));
  jacobian_out(w, out_witness_partial);
  return SV_OK;
  SV_GUARD_END
}

// ---- several points: the multi-point pass, division by several roots, the SHPLONK (bdfg21) opening ----
namespace {
// the checks on a table of polynomials, one function per status so that a call can put its own
// rules of the same status beside them: null / alignment, then emptiness, then the lengths
int polys_pointer_check(const sv_fe* const* d_polys, size_t m) {
  const size_t seen = std::min<size_t>(m, SV_OPEN_BATCH_MAX);
  for (size_t j = 0; j < seen; j++) {
    if (!d_polys[j]) {
      sv::set_error("null pointer (polynomial %zu)", j);
      return SV_ERR_ARG;
    }
    if ((uintptr_t)d_polys[j] % 16) {
      sv::set_error("polynomial %zu is not 16-byte aligned", j);
      return SV_ERR_ARG;
    }
  }
  return SV_OK;
}
int polys_empty_check(const uint64_t* lens, size_t m) {
  if (m == 0) {
    sv::set_error("batch should not be empty");
    return SV_ERR_EMPTY;
  }
  for (size_t j = 0; j < std::min<size_t>(m, SV_OPEN_BATCH_MAX); j++)
    if (lens[j] == 0) {
      sv::set_error("polynomial should not be empty (polynomial %zu)", j);
      return SV_ERR_EMPTY;
    }
  return SV_OK;
}
int polys_length_check(const uint64_t* lens, size_t m, size_t* N) {
  if (m > SV_OPEN_BATCH_MAX) {
    sv::set_error("m = %zu exceeds the per-call limit of %d polynomials", m, SV_OPEN_BATCH_MAX);
    return SV_ERR_LEN;
  }
  size_t longest = 0;
  for (size_t j = 0; j < m; j++) {
    if (lens[j] > kMaxSetRows) {
      sv::set_error("n = %llu exceeds the per-device limit 2^26 (polynomial %zu)", (unsigned long long)lens[j], j);
      return SV_ERR_LEN;
    }
    longest = std::max<size_t>(longest, lens[j]);
  }
  *N = longest;
  return SV_OK;
}
int points_reduced_check(const sv_fe* points, size_t K, const char* what) {
  for (size_t k = 0; k < K; k++)
    if (!host::f_is_reduced(fe_in(points[k]), host::R64)) {
      sv::set_error("%s %zu not reduced mod the scalar field order", what, k);
      return SV_ERR_ARG;
    }
  return SV_OK;
}
int points_count_check(size_t K) {
  if (K > SV_EVAL_POINTS_MAX) {
    sv::set_error("K = %zu exceeds the per-call limit of %d points", K, SV_EVAL_POINTS_MAX);
    return SV_ERR_LEN;
  }
  return SV_OK;
}
bool fe_same(const sv_fe& a, const sv_fe& b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }
sv_fe fe_mont(const sv_fe& a, int form) { return form == SV_MONTGOMERY ? a : poly_fr_to_mont(a); }
}  // namespace

int sv_bn254_fr_poly_eval_points_device(const sv_fe* const* d_polys, const uint64_t* lens, size_t m,
                                        const sv_fe* points, size_t K, int form, int device, void* stream,
                                        sv_fe* out_evals) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_polys || !lens || !points || !out_evals) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(polys_pointer_check(d_polys, m));
  SV_TRY(polys_empty_check(lens, m));
  if (K == 0) {
    sv::set_error("the points should not be empty");
    return SV_ERR_EMPTY;
  }
  SV_TRY(points_count_check(K));
  size_t N = 0;
  SV_TRY(polys_length_check(lens, m, &N));
  SV_TRY(points_reduced_check(points, K, "point"));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  // the table (the polynomials' rows, then the points' rows: one copy) and the pass's scratch
  const size_t rb = batch_table_bytes(m), tb = rb + Workspace::aligned(K * kPointRowBytes);
  const size_t hb = poly_points_head_bytes(m, K);
  SV_TRY(ws->reserve(tb + Workspace::aligned(poly_points_scratch_bytes(m, K, N))));
  SV_TRY(ws->reserve_pinned(tb + hb));
  std::vector<sv_fe> ones(m, poly_fr_one());  // the rows' weights play no part in an evaluation
  poly_batch_fill_table_weights(reinterpret_cast<BatchRow*>(ws->pinned), d_polys, lens, m, ones.data(), SV_MONTGOMERY);
  poly_points_fill_rows(ws->pinned + rb, points, K, form, N);
  char* d_scratch = ws->buf + tb;
  SV_HIP(hipMemcpyAsync(ws->buf, ws->pinned, rb + K * kPointRowBytes, hipMemcpyHostToDevice, ws->stream));
  SV_TRY(poly_eval_points_enqueue(reinterpret_cast<const BatchRow*>(ws->buf), m, N, ws->buf + rb, ws->pinned + rb, K,
                                  form, d_scratch, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned + tb, d_scratch, hb, hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  uint32_t errv;
  memcpy(&errv, ws->pinned + tb + kPointsErrOffset, 4);
  if (errv) {
    sv::set_error("invalid input: coefficient not reduced mod r");
    return SV_ERR_ARG;
  }
  memcpy(out_evals, ws->pinned + tb + kPointsEvalsOffset, m * K * sizeof(sv_fe));
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_fr_poly_div_roots_device(const sv_fe* d_coeffs, size_t n, const sv_fe* roots, size_t K, int form,
                                      int device, void* stream, sv_fe* d_quotient) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_coeffs || !roots || !d_quotient) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if ((uintptr_t)d_coeffs % 16 || (uintptr_t)d_quotient % 16) {
    sv::set_error("d_coeffs or d_quotient is not 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (n == 0 || K == 0) {
    sv::set_error(n == 0 ? "polynomial should not be empty" : "the roots should not be empty");
    return SV_ERR_EMPTY;
  }
  SV_TRY(points_count_check(K));
  if (n > kMaxSetRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26", n);
    return SV_ERR_LEN;
  }
  SV_TRY(points_reduced_check(roots, K, "root"));
  if (n <= K) {
    sv::set_error("n = %zu coefficients leave no quotient by %zu roots", n, K);
    return SV_ERR_ARG;
  }
  const uintptr_t cb = (uintptr_t)d_coeffs, qb = (uintptr_t)d_quotient;
  if (qb < cb + n * sizeof(sv_fe) && cb < qb + (n - K) * sizeof(sv_fe)) {
    sv::set_error("d_quotient overlaps d_coeffs (phase 3 reads the coefficients again while it writes)");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  const size_t tbytes = K > 1 ? Workspace::aligned((n - 1) * sizeof(sv_fe)) : 0;  // the quotients in between
  SV_TRY(ws->reserve_in(2 * tbytes + 1));
  SV_TRY(ws->reserve(poly_div_roots_scratch_bytes(n, K)));
  SV_TRY(ws->reserve_pinned(kDivHeadBytes));
  void* const tmp[2] = {ws->inbuf, ws->inbuf + tbytes};
  SV_TRY(poly_div_roots_enqueue(d_coeffs, n, roots, K, form, form, d_quotient, tmp, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf, kDivHeadBytes, hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  sv_fe unused;
  return div_result(ws->pinned, &unused);
  SV_GUARD_END
}

// ---- SHPLONK (bdfg21): W over h = sum_i gamma^i h_i, then W' over the linearisation's quotient ----
namespace {
// What both calls derive from the sets: N = the longest set, the rows of h, and per set N_i, K_i.
struct ShplonkShape {
  size_t N = 0, h_len = 0;
  std::vector<size_t> set_len;  // N_i
};

// The checks both calls share on sets and points, in the header's order.  `set_lens` are the N_i
// (the witness call's argument; the quotient call passes what it derived from lens).
int shplonk_set_pointer_rules(const sv_shplonk_set* sets, size_t n_sets, const sv_fe* points, size_t n_points) {
  if (n_sets == 0 || n_points == 0) {
    sv::set_error(n_sets == 0 ? "the sets should not be empty" : "the points should not be empty");
    return SV_ERR_EMPTY;
  }
  for (size_t i = 0; i < std::min<size_t>(n_sets, SV_OPEN_BATCH_MAX); i++)
    if (sets[i].num_polys == 0 || sets[i].num_points == 0) {
      sv::set_error("set %zu should not be empty", i);
      return SV_ERR_EMPTY;
    }
  (void)points;
  return SV_OK;
}
int shplonk_set_length_rules(const sv_shplonk_set* sets, size_t n_sets) {
  if (n_sets > SV_OPEN_BATCH_MAX) {
    sv::set_error("n_sets = %zu exceeds the per-call limit of %d", n_sets, SV_OPEN_BATCH_MAX);
    return SV_ERR_LEN;
  }
  for (size_t i = 0; i < n_sets; i++) SV_TRY(points_count_check(sets[i].num_points));
  return SV_OK;
}
// the sets partition [0, m) and [0, n_points) in order; no point twice inside a set
int shplonk_partition_rules(const sv_shplonk_set* sets, size_t n_sets, size_t m, const sv_fe* points,
                            size_t n_points) {
  uint64_t poly = 0, point = 0;
  for (size_t i = 0; i < n_sets; i++) {
    if (sets[i].first_poly != poly || sets[i].first_point != point) {
      sv::set_error("the sets do not partition the arrays (set %zu starts at polynomial %u, point %u)", i,
                    sets[i].first_poly, sets[i].first_point);
      return SV_ERR_ARG;
    }
    poly += sets[i].num_polys, point += sets[i].num_points;
  }
  if (poly != m || point != n_points) {
    sv::set_error("the sets do not partition the arrays (%llu polynomials of %zu, %llu points of %zu)",
                  (unsigned long long)poly, m, (unsigned long long)point, n_points);
    return SV_ERR_ARG;
  }
  for (size_t i = 0; i < n_sets; i++) {
    const sv_fe* p = points + sets[i].first_point;
    for (uint32_t a = 0; a < sets[i].num_points; a++)
      for (uint32_t b = a + 1; b < sets[i].num_points; b++)
        if (fe_same(p[a], p[b])) {
          sv::set_error("repeated point in set %zu (points %u and %u)", i, a, b);
          return SV_ERR_ARG;
        }
  }
  return SV_OK;
}
void shplonk_shape(const sv_shplonk_set* sets, size_t n_sets, ShplonkShape* s) {
  s->N = s->h_len = 0;
  for (size_t i = 0; i < n_sets; i++) {
    s->N = std::max(s->N, s->set_len[i]);
    if (s->set_len[i] > sets[i].num_points) s->h_len = std::max(s->h_len, s->set_len[i] - sets[i].num_points);
  }
}
int shplonk_work_rules(size_t n_sets, size_t N, const void* d_work, uint64_t work_elems) {
  if ((uint64_t)(n_sets + 1) * N > work_elems) {
    sv::set_error("work_elems = %llu is too small: %zu sets of up to %zu coefficients need %llu",
                  (unsigned long long)work_elems, n_sets, N, (unsigned long long)(n_sets + 1) * N);
    return SV_ERR_ARG;
  }
  (void)d_work;
  return SV_OK;
}
int shplonk_handle_rules(uint64_t handle, size_t offset, size_t rows, BaseSet* t) {
  if (!set_lookup(handle, t)) return SV_ERR_ARG;
  if (offset > t->n || rows > t->n - offset) {
    sv::set_error("rows [%zu, %zu + %zu) reach past base set %llu (%zu rows)", offset, offset, rows,
                  (unsigned long long)handle, t->n);
    return SV_ERR_ARG;
  }
  return SV_OK;
}
// one pass's flag, copied behind the kernels into its own 32-byte slot of the pinned staging
int shplonk_flag_copy(Workspace* ws, size_t pinned_at, const void* d_scratch) {
  SV_HIP(hipMemcpyAsync(ws->pinned + pinned_at, static_cast<const char*>(d_scratch) + kBatchErrOffset, 4,
                        hipMemcpyDeviceToHost, ws->stream));
  return SV_OK;
}
bool shplonk_any_flag(const Workspace* ws, size_t pinned_at, size_t count) {
  for (size_t i = 0; i < count; i++) {
    uint32_t errv;
    memcpy(&errv, ws->pinned + pinned_at + 32 * i, 4);
    if (errv) return true;
  }
  return false;
}
const sv_fe kFeZero = {{0, 0, 0, 0}};
}  // namespace

int sv_bn254_shplonk_work_elems(size_t n_sets, size_t N, uint64_t* elems) noexcept {
  SV_GUARD_BEGIN
  if (!elems) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (n_sets == 0 || N == 0) {
    sv::set_error("the sets should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n_sets > SV_OPEN_BATCH_MAX || N > kMaxSetRows) {
    sv::set_error("n_sets = %zu, N = %zu out of range", n_sets, N);
    return SV_ERR_LEN;
  }
  *elems = (uint64_t)(n_sets + 1) * N;  // c_1 .. c_s, then h, N elements apart
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_shplonk_quotient_device(uint64_t handle, size_t offset, const sv_fe* const* d_polys, const uint64_t* lens,
                                     size_t m, const sv_shplonk_set* sets, size_t n_sets, const sv_fe* points,
                                     size_t n_points, const sv_fe* mu, const sv_fe* gamma, int form, void* stream,
                                     sv_fe* d_work, uint64_t work_elems, sv_g1_jacobian* out_w_partial) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_polys || !lens || !sets || !points || !mu || !gamma || !d_work || !out_w_partial) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(polys_pointer_check(d_polys, m));
  if ((uintptr_t)d_work % 16) {
    sv::set_error("d_work is not 16-byte aligned");
    return SV_ERR_ARG;
  }
  SV_TRY(polys_empty_check(lens, m));
  SV_TRY(shplonk_set_pointer_rules(sets, n_sets, points, n_points));
  size_t longest = 0;
  SV_TRY(polys_length_check(lens, m, &longest));
  SV_TRY(shplonk_set_length_rules(sets, n_sets));
  SV_TRY(points_reduced_check(points, std::min<size_t>(n_points, (size_t)SV_OPEN_BATCH_MAX * SV_EVAL_POINTS_MAX), "point"));
  SV_TRY(points_reduced_check(mu, 1, "mu"));
  SV_TRY(points_reduced_check(gamma, 1, "gamma"));
  SV_TRY(shplonk_partition_rules(sets, n_sets, m, points, n_points));
  ShplonkShape sh;
  sh.set_len.assign(n_sets, 0);
  for (size_t i = 0; i < n_sets; i++)
    for (uint32_t j = 0; j < sets[i].num_polys; j++)
      sh.set_len[i] = std::max<size_t>(sh.set_len[i], lens[sets[i].first_poly + j]);
  shplonk_shape(sets, n_sets, &sh);
  const size_t N = sh.N;
  SV_TRY(shplonk_work_rules(n_sets, N, d_work, work_elems));
  for (size_t j = 0; j < m; j++) {  // the combinations are written while other blocks still read the polynomials
    const uintptr_t pb = (uintptr_t)d_polys[j], wb = (uintptr_t)d_work;
    if (wb < pb + lens[j] * sizeof(sv_fe) && pb < wb + (n_sets + 1) * N * sizeof(sv_fe)) {
      sv::set_error("d_work overlaps polynomial %zu", j);
      return SV_ERR_ARG;
    }
  }
  BaseSet t;
  SV_TRY(shplonk_handle_rules(handle, offset, sh.h_len, &t));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(t.dev, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();

  // The sets whose combination is longer than their number of points have a quotient h_i; the
  // others' is zero.  Device: the table (the m polynomials' rows with the powers of mu per set, then
  // one row per h_i with gamma^i), one pass's scratch per set and one for h's, the divisions'.
  // Input buffer: the h_i, N rows apart, then the two quotients in between.  Pinned: the table, then
  // one flag slot per pass.
  std::vector<size_t> live;
  for (size_t i = 0; i < n_sets; i++)
    if (sh.set_len[i] > sets[i].num_points) live.push_back(i);
  const size_t slot = Workspace::aligned(N * sizeof(sv_fe));
  const size_t tb = batch_table_bytes(m + n_sets);
  std::vector<size_t> scratch_at(n_sets + 1);
  size_t at = tb;
  for (size_t i = 0; i < n_sets; i++) {
    scratch_at[i] = at;
    at += Workspace::aligned(poly_batch_scratch_bytes(sets[i].num_polys, sh.set_len[i]));
  }
  scratch_at[n_sets] = at;
  at += Workspace::aligned(poly_batch_scratch_bytes(std::max<size_t>(live.size(), 1), std::max<size_t>(sh.h_len, 1)));
  const size_t div_at = at;
  at += Workspace::aligned(poly_div_roots_scratch_bytes(N, 2));
  SV_TRY(ws->reserve(at));
  SV_TRY(ws->reserve_in((n_sets + 2) * slot + 1));
  SV_TRY(ws->reserve_pinned(tb + 32 * (n_sets + 1)));
  memset(ws->pinned + tb, 0, 32 * (n_sets + 1));
  BatchRow* rows = reinterpret_cast<BatchRow*>(ws->pinned);
  for (size_t i = 0; i < n_sets; i++)
    poly_batch_fill_table(rows + sets[i].first_poly, d_polys + sets[i].first_poly, lens + sets[i].first_poly,
                          sets[i].num_polys, *mu, form);
  {
    const sv_fe g = fe_mont(*gamma, form);
    sv_fe gp = poly_fr_one();
    size_t r = 0;
    for (size_t i = 0; i < n_sets; i++) {
      if (r < live.size() && live[r] == i) {
        rows[m + r].coeffs = ws->inbuf + i * slot;
        rows[m + r].len = sh.set_len[i] - sets[i].num_points;
        rows[m + r].vpow = gp;
        r++;
      }
      gp = poly_fr_mul(gp, g);
    }
  }
  const BatchRow* d_table = reinterpret_cast<const BatchRow*>(ws->buf);
  SV_HIP(hipMemcpyAsync(ws->buf, rows, (m + live.size()) * sizeof(BatchRow), hipMemcpyHostToDevice, ws->stream));
  void* const tmp[2] = {ws->inbuf + n_sets * slot, ws->inbuf + (n_sets + 1) * slot};
  for (size_t i = 0; i < n_sets; i++) {
    sv_fe* c = d_work + i * N;
    SV_TRY(poly_combine_eval_enqueue(d_table + sets[i].first_poly, sets[i].num_polys, sh.set_len[i], kFeZero, form,
                                     SV_MONTGOMERY, c, ws->buf + scratch_at[i], ws->stream));
    SV_TRY(shplonk_flag_copy(ws, tb + 32 * i, ws->buf + scratch_at[i]));
    if (sh.set_len[i] <= sets[i].num_points) continue;
    sv_fe roots[SV_EVAL_POINTS_MAX];
    for (uint32_t k = 0; k < sets[i].num_points; k++) roots[k] = fe_mont(points[sets[i].first_point + k], form);
    SV_TRY(poly_div_roots_enqueue(c, sh.set_len[i], roots, sets[i].num_points, SV_MONTGOMERY, SV_MONTGOMERY,
                                  ws->inbuf + i * slot, tmp, ws->buf + div_at, ws->stream));
  }
  Xyzz w = host::x_identity();
  if (sh.h_len > 0) {  // the MSM synchronises the stream, so the flags have landed when it returns
    sv_fe* h = d_work + n_sets * N;
    SV_TRY(poly_combine_eval_enqueue(d_table + m, live.size(), sh.h_len, kFeZero, SV_MONTGOMERY, SV_MONTGOMERY, h,
                                     ws->buf + scratch_at[n_sets], ws->stream));
    const MsmResident set{t.rows, t.vtab, t.n, offset};
    SV_TRY(msm_run_resident_device(set, h, sh.h_len, SV_MONTGOMERY, t.dev, ws->stream, &w));
  } else {
    SV_HIP(hipStreamSynchronize(ws->stream));
  }
  dl.armed = false;
  if (shplonk_any_flag(ws, tb, n_sets)) {
    sv::set_error("invalid input: coefficient not reduced mod r");
    return SV_ERR_ARG;
  }
  jacobian_out(w, out_w_partial);
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_shplonk_witness_device(uint64_t handle, size_t offset, const sv_shplonk_set* sets, size_t n_sets,
                                    const sv_fe* points, size_t n_points, const uint64_t* set_lens,
                                    const sv_fe* gamma, const sv_fe* z_prime, int form, void* stream,
                                    const sv_fe* d_work, uint64_t work_elems,
                                    sv_g1_jacobian* out_w_prime_partial) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!sets || !points || !set_lens || !gamma || !z_prime || !d_work || !out_w_prime_partial) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if ((uintptr_t)d_work % 16) {
    sv::set_error("d_work is not 16-byte aligned");
    return SV_ERR_ARG;
  }
  SV_TRY(shplonk_set_pointer_rules(sets, n_sets, points, n_points));
  for (size_t i = 0; i < std::min<size_t>(n_sets, SV_OPEN_BATCH_MAX); i++)
    if (set_lens[i] == 0) {
      sv::set_error("polynomial should not be empty (set %zu)", i);
      return SV_ERR_EMPTY;
    }
  SV_TRY(shplonk_set_length_rules(sets, n_sets));
  for (size_t i = 0; i < n_sets; i++)
    if (set_lens[i] > kMaxSetRows) {
      sv::set_error("n = %llu exceeds the per-device limit 2^26 (set %zu)", (unsigned long long)set_lens[i], i);
      return SV_ERR_LEN;
    }
  SV_TRY(points_reduced_check(points, std::min<size_t>(n_points, (size_t)SV_OPEN_BATCH_MAX * SV_EVAL_POINTS_MAX), "point"));
  SV_TRY(points_reduced_check(gamma, 1, "gamma"));
  SV_TRY(points_reduced_check(z_prime, 1, "z_prime"));
  uint64_t polys = 0;
  for (size_t i = 0; i < n_sets; i++) polys += sets[i].num_polys;
  SV_TRY(shplonk_partition_rules(sets, n_sets, polys, points, n_points));
  for (size_t k = 0; k < n_points; k++)
    if (fe_same(points[k], *z_prime)) {
      sv::set_error("z_prime equals point %zu", k);
      return SV_ERR_ARG;
    }
  ShplonkShape sh;
  sh.set_len.assign(set_lens, set_lens + n_sets);
  shplonk_shape(sets, n_sets, &sh);
  const size_t N = sh.N;
  SV_TRY(shplonk_work_rules(n_sets, N, d_work, work_elems));
  BaseSet t;
  SV_TRY(shplonk_handle_rules(handle, offset, N - 1, &t));
  if (N == 1) {  // L is a constant: no quotient term, no MSM
    jacobian_out(host::x_identity(), out_w_prime_partial);
    return SV_OK;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(t.dev, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  // L = sum_i gamma^i Z_1(z') / Z_i(z') c_i - Z_1(z') h: one weighted pass over the rows of d_work,
  // then the single opening's division by (X - z') and the set's MSM
  const size_t n_rows = n_sets + (sh.h_len > 0 ? 1 : 0);
  std::vector<sv_fe> weights(n_rows);
  std::vector<const sv_fe*> ptrs(n_rows);
  std::vector<uint64_t> rlens(n_rows);
  const sv_fe zp = fe_mont(*z_prime, form), g = fe_mont(*gamma, form);
  sv_fe z1 = poly_fr_one(), gp = poly_fr_one();
  for (size_t i = 0; i < n_sets; i++) {
    sv_fe zi = poly_fr_one();
    for (uint32_t k = 0; k < sets[i].num_points; k++)
      zi = poly_fr_mul(zi, poly_fr_sub(zp, fe_mont(points[sets[i].first_point + k], form)));
    if (i == 0) z1 = zi;
    weights[i] = poly_fr_mul(gp, poly_fr_mul(z1, poly_fr_inv(zi)));
    ptrs[i] = d_work + i * N;
    rlens[i] = sh.set_len[i];
    gp = poly_fr_mul(gp, g);
  }
  if (sh.h_len > 0) {
    weights[n_sets] = poly_fr_sub(kFeZero, z1);
    ptrs[n_sets] = d_work + n_sets * N;
    rlens[n_sets] = sh.h_len;
  }
  const size_t tb = batch_table_bytes(n_rows);
  const size_t bbytes = tb + Workspace::aligned(poly_batch_scratch_bytes(n_rows, N));
  const size_t lbytes = Workspace::aligned(N * sizeof(sv_fe));
  SV_TRY(ws->reserve_in(lbytes + Workspace::aligned((N - 1) * sizeof(sv_fe) + 1)));
  SV_TRY(ws->reserve(bbytes + Workspace::aligned(poly_div_scratch_bytes(N))));
  SV_TRY(ws->reserve_pinned(tb + 32));
  BatchRow* rows = reinterpret_cast<BatchRow*>(ws->pinned);
  poly_batch_fill_table_weights(rows, ptrs.data(), rlens.data(), n_rows, weights.data(), SV_MONTGOMERY);
  SV_HIP(hipMemcpyAsync(ws->buf, rows, n_rows * sizeof(BatchRow), hipMemcpyHostToDevice, ws->stream));
  void* d_l = ws->inbuf;
  void* d_quot = ws->inbuf + lbytes;
  SV_TRY(poly_combine_eval_enqueue(reinterpret_cast<const BatchRow*>(ws->buf), n_rows, N, kFeZero, SV_MONTGOMERY,
                                   SV_MONTGOMERY, d_l, ws->buf + tb, ws->stream));
  SV_TRY(shplonk_flag_copy(ws, tb, ws->buf + tb));
  SV_TRY(poly_div_linear_enqueue(d_l, N, zp, SV_MONTGOMERY, SV_MONTGOMERY, d_quot, ws->buf + bbytes, ws->stream));
  Xyzz w = host::x_identity();
  const MsmResident set{t.rows, t.vtab, t.n, offset};
  SV_TRY(msm_run_resident_device(set, d_quot, N - 1, SV_MONTGOMERY, t.dev, ws->stream, &w));
  dl.armed = false;
  if (shplonk_any_flag(ws, tb, 1)) {
    sv::set_error("invalid input: the work buffer holds an element not below r");
    return SV_ERR_ARG;
  }
  jacobian_out(w, out_w_prime_partial);
  return SV_OK;
  SV_GUARD_END
}

// ---- Fr NTT on the device: forward, inverse and coset transforms (csrc/ntt.hip) ----
namespace {
// SVGPU_NTT_TILE_LOG = 1 .. kNttTileLog, read per call; anything else is the default
uint32_t ntt_tile_log() {
  const char* e = getenv("SVGPU_NTT_TILE_LOG");
  if (!e || !*e) return kNttTileLog;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  if (*end != '\0' || v < 1 || v > (long)kNttTileLog) return kNttTileLog;
  return (uint32_t)v;
}
}  // namespace

int sv_bn254_fr_root_of_unity(uint32_t log_n, int form, sv_fe* out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  return fr_root_of_unity(log_n, form, out);
  SV_GUARD_END
}

int sv_bn254_fr_ntt_device(const sv_fe* d_in, sv_fe* d_out, uint32_t log_n, size_t count, int direction,
                           const sv_fe* shift, int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (direction != SV_NTT_FORWARD && direction != SV_NTT_INVERSE) {
    sv::set_error("direction %d is neither SV_NTT_FORWARD nor SV_NTT_INVERSE", direction);
    return SV_ERR_ARG;
  }
  if (!d_in || !d_out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 15u) {
    sv::set_error("d_in and d_out must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (count == 0) {
    sv::set_error("the batch should not be empty");
    return SV_ERR_EMPTY;
  }
  if (log_n > SV_NTT_MAX_LOG || count > ((size_t(1) << 28) >> log_n)) {
    sv::set_error("log_n = %u, count = %zu: beyond 2^%d points per transform or 2^28 elements per call", log_n, count,
                  SV_NTT_MAX_LOG);
    return SV_ERR_LEN;
  }
  NttCall call{};
  call.has_shift = false;
  if (shift) {
    const F g = fe_in(*shift);
    if (!host::f_is_reduced(g, host::R64)) {
      sv::set_error("shift not reduced mod the scalar field order");
      return SV_ERR_ARG;
    }
    if ((shift->l[0] | shift->l[1] | shift->l[2] | shift->l[3]) == 0) {
      sv::set_error("shift is zero: the coset has no inverse");
      return SV_ERR_ARG;
    }
    sv_fe one = {{1, 0, 0, 0}};
    if (form == SV_MONTGOMERY) one = poly_fr_one();
    call.has_shift = memcmp(shift->l, one.l, sizeof one.l) != 0;
    call.shift = *shift;
  }
  const size_t bytes = (count << log_n) * sizeof(sv_fe);
  const uintptr_t ib = (uintptr_t)d_in, ob = (uintptr_t)d_out;
  if (ib != ob && ib < ob + bytes && ob < ib + bytes) {
    sv::set_error("d_out overlaps d_in without being d_in (in place is d_out == d_in)");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  call.d_in = d_in;
  call.d_out = d_out;
  call.log_n = log_n;
  call.count = count;
  call.inverse = direction == SV_NTT_INVERSE;
  call.form = form;
  call.tile_log = ntt_tile_log();
  SV_TRY(ws->reserve(ntt_scratch_bytes(log_n, count, call.tile_log)));
  SV_TRY(ws->reserve_pinned(kNttHeadBytes));
  SV_TRY(ntt_enqueue(call, device, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf + kNttErrOffset, sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  uint32_t errv;
  memcpy(&errv, ws->pinned, sizeof errv);
  if (errv) {
    sv::set_error("invalid input: element not reduced mod r");
    return SV_ERR_ARG;
  }
  return SV_OK;
  SV_GUARD_END
}

// ---- extended-domain quotient: coset LDE and division by X^n - 1 (csrc/ntt.hip, csrc/ext_plan.hpp) ----
namespace {
// rule 4 of both calls: a shift below r, then not zero
int ext_shift_rules(const sv_fe& shift) {
  if (!host::f_is_reduced(fe_in(shift), host::R64)) {
    sv::set_error("shift not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  if ((shift.l[0] | shift.l[1] | shift.l[2] | shift.l[3]) == 0) {
    sv::set_error("shift is zero: the coset has no inverse");
    return SV_ERR_ARG;
  }
  return SV_OK;
}

// both calls past their checks: the error flag after the stream has drained
int ext_finish(DrainedLease* dl) {
  Workspace* ws = dl->ws();
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf + kNttErrOffset, sizeof(uint32_t), hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl->armed = false;
  uint32_t errv;
  memcpy(&errv, ws->pinned, sizeof errv);
  if (errv) {
    sv::set_error("invalid input: element not reduced mod r");
    return SV_ERR_ARG;
  }
  return SV_OK;
}
}  // namespace

int sv_bn254_fr_coset_lde_device(const sv_fe* d_coeffs, sv_fe* d_evals, uint32_t log_n, uint32_t log_ext,
                                 size_t count, const sv_fe* shift, int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_coeffs || !d_evals) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (((uintptr_t)d_coeffs | (uintptr_t)d_evals) & 15u) {
    sv::set_error("d_coeffs and d_evals must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (count == 0) {
    sv::set_error("the batch should not be empty");
    return SV_ERR_EMPTY;
  }
  if (log_ext > SV_EXT_LOG_MAX || log_n > SV_NTT_MAX_LOG || log_n + log_ext > SV_NTT_MAX_LOG ||
      count > ((size_t(1) << 28) >> (log_n + log_ext))) {
    sv::set_error("log_n = %u, log_ext = %u, count = %zu: beyond log_ext %d, 2^%d points per transform or 2^28 "
                  "elements per call", log_n, log_ext, count, SV_EXT_LOG_MAX, SV_NTT_MAX_LOG);
    return SV_ERR_LEN;
  }
  LdeCall call{};
  call.has_shift = false;
  if (shift) {
    SV_TRY(ext_shift_rules(*shift));
    sv_fe one = {{1, 0, 0, 0}};
    if (form == SV_MONTGOMERY) one = poly_fr_one();
    call.has_shift = memcmp(shift->l, one.l, sizeof one.l) != 0;
    call.shift = *shift;
  }
  const size_t in_bytes = (count << log_n) * sizeof(sv_fe), out_bytes = (count << (log_n + log_ext)) * sizeof(sv_fe);
  const uintptr_t ib = (uintptr_t)d_coeffs, ob = (uintptr_t)d_evals;
  if (ib < ob + out_bytes && ob < ib + in_bytes) {
    sv::set_error("d_evals overlaps d_coeffs (the extension is never in place)");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  call.d_coeffs = d_coeffs;
  call.d_evals = d_evals;
  call.log_n = log_n;
  call.log_ext = log_ext;
  call.count = count;
  call.form = form;
  call.tile_log = ntt_tile_log();
  SV_TRY(ws->reserve(lde_scratch_bytes(log_n, log_ext, count, call.tile_log)));
  SV_TRY(ws->reserve_pinned(kNttHeadBytes));
  SV_TRY(lde_enqueue(call, device, ws->buf, ws->stream));
  return ext_finish(&dl);
  SV_GUARD_END
}

int sv_bn254_fr_quotient_coeffs_device(const sv_fe* d_numer, sv_fe* d_out, uint32_t log_n, uint32_t log_ext,
                                       size_t pieces, const sv_fe* shift, int form, int device,
                                       void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_numer || !d_out || !shift) {
    sv::set_error("null pointer (the quotient needs a coset: shift may not be NULL)");
    return SV_ERR_ARG;
  }
  if (((uintptr_t)d_numer | (uintptr_t)d_out) & 15u) {
    sv::set_error("d_numer and d_out must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (pieces == 0) {
    sv::set_error("the quotient should not be empty (pieces == 0)");
    return SV_ERR_EMPTY;
  }
  if (log_ext > SV_EXT_LOG_MAX || log_n > SV_NTT_MAX_LOG || log_n + log_ext > SV_NTT_MAX_LOG) {
    sv::set_error("log_n = %u, log_ext = %u: beyond log_ext %d or 2^%d points per transform", log_n, log_ext,
                  SV_EXT_LOG_MAX, SV_NTT_MAX_LOG);
    return SV_ERR_LEN;
  }
  if (pieces > (size_t(1) << log_ext)) {
    sv::set_error("pieces = %zu: the extended domain holds 2^%u pieces of 2^%u coefficients", pieces, log_ext, log_n);
    return SV_ERR_LEN;
  }
  SV_TRY(ext_shift_rules(*shift));
  const uint32_t K = log_n + log_ext;
  if (coset_meets_domain(*shift, form, K)) {
    sv::set_error("coset meets the domain: shift^(2^%u) == 1, so X^n - 1 vanishes on it", K);
    return SV_ERR_ARG;
  }
  const size_t in_bytes = (size_t(1) << K) * sizeof(sv_fe), out_bytes = (pieces << log_n) * sizeof(sv_fe);
  const uintptr_t ib = (uintptr_t)d_numer, ob = (uintptr_t)d_out;
  if (ib != ob && ib < ob + out_bytes && ob < ib + in_bytes) {
    sv::set_error("d_out overlaps d_numer without being d_numer (in place is d_out == d_numer)");
    return SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  QuotCall call{};
  call.d_numer = d_numer;
  call.d_out = d_out;
  call.log_n = log_n;
  call.log_ext = log_ext;
  call.pieces = pieces;
  call.shift = *shift;
  call.form = form;
  call.tile_log = ntt_tile_log();
  SV_TRY(ws->reserve(quotient_scratch_bytes(log_n, log_ext, call.tile_log)));
  SV_TRY(ws->reserve_pinned(kNttHeadBytes + quotient_stage_bytes(log_ext)));
  SV_TRY(quotient_enqueue(call, device, ws->buf, ws->pinned + kNttHeadBytes, ws->stream));
  return ext_finish(&dl);
  SV_GUARD_END
}

// ---- running products and batch inversion over Fr columns (csrc/grand_product.hip) ----
namespace {
bool fr_reduced(const sv_fe& a) { return host::f_is_reduced(fe_in(a), host::R64); }

// rule 1 for one side: the array, then per descriptor the kind, the pointers and their alignment
int factor_pointer_rules(const sv_fr_factor* f, size_t count, const char* side) {
  if (count && !f) {
    sv::set_error("null pointer (%s descriptors)", side);
    return SV_ERR_ARG;
  }
  for (size_t j = 0; j < std::min(count, (size_t)SV_PRODUCT_FACTORS_MAX); j++) {
    if (f[j].kind != SV_FACTOR_PLAIN && f[j].kind != SV_FACTOR_COLUMN && f[j].kind != SV_FACTOR_IDENTITY) {
      sv::set_error("%s factor %zu: kind %u is none of SV_FACTOR_PLAIN, _COLUMN, _IDENTITY", side, j, f[j].kind);
      return SV_ERR_ARG;
    }
    const bool column = f[j].kind == SV_FACTOR_COLUMN;
    if (!f[j].d_x || (column && !f[j].d_y)) {
      sv::set_error("null pointer (%s factor %zu)", side, j);
      return SV_ERR_ARG;
    }
    if (((uintptr_t)f[j].d_x | (column ? (uintptr_t)f[j].d_y : 0)) & 15u) {
      sv::set_error("%s factor %zu: columns must be 16-byte aligned", side, j);
      return SV_ERR_ARG;
    }
  }
  return SV_OK;
}

// rule 4 for one side: the s and c that the kernels read
int factor_scalar_rules(const sv_fr_factor* f, size_t count, const char* side) {
  for (size_t j = 0; j < count; j++)
    if (!fr_reduced(f[j].c) || (f[j].kind != SV_FACTOR_PLAIN && !fr_reduced(f[j].s))) {
      sv::set_error("%s factor %zu: s or c not reduced mod the scalar field order", side, j);
      return SV_ERR_ARG;
    }
  return SV_OK;
}

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// both entry points past their checks: the lease, the three launches, the head
int grand_product_run(const GpCall& call, int device, void* stream, sv_fe* out_total) {
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  SV_TRY(ws->reserve(grand_product_scratch_bytes(call.n, call.invert)));
  SV_TRY(ws->reserve_pinned(kGpHeadBytes));
  SV_TRY(grand_product_enqueue(call, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf, kGpHeadBytes, hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  uint32_t errv;
  memcpy(&errv, ws->pinned + kGpErrOffset, sizeof errv);
  if (errv) {
    sv::set_error("invalid input: element not reduced mod r");
    return SV_ERR_ARG;
  }
  if (out_total) memcpy(out_total->l, ws->pinned + kGpTotalOffset, sizeof(sv_fe));
  return SV_OK;
}
}  // namespace

int sv_bn254_fr_grand_product_device(const sv_fr_factor* num, size_t n_num, const sv_fr_factor* den, size_t n_den,
                                     size_t n, const sv_fe* z0, const sv_fe* omega, int form, sv_fe* d_z,
                                     sv_fe* out_total, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_z || !z0) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  SV_TRY(factor_pointer_rules(num, n_num, "numerator"));
  SV_TRY(factor_pointer_rules(den, n_den, "denominator"));
  if ((uintptr_t)d_z & 15u) {
    sv::set_error("d_z must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (n == 0 || (n_num == 0 && n_den == 0)) {
    sv::set_error("the product should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > kGpMaxRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26", n);
    return SV_ERR_LEN;
  }
  if (n_num > SV_PRODUCT_FACTORS_MAX || n_den > SV_PRODUCT_FACTORS_MAX) {
    sv::set_error("%zu + %zu factors: a side takes at most %d", n_num, n_den, SV_PRODUCT_FACTORS_MAX);
    return SV_ERR_LEN;
  }
  if (!fr_reduced(*z0)) {
    sv::set_error("z0 not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  SV_TRY(factor_scalar_rules(num, n_num, "numerator"));
  SV_TRY(factor_scalar_rules(den, n_den, "denominator"));
  bool identity = false;
  for (size_t j = 0; j < n_num + n_den; j++)
    identity |= (j < n_num ? num[j] : den[j - n_num]).kind == SV_FACTOR_IDENTITY;
  if (identity && omega && !fr_reduced(*omega)) {
    sv::set_error("omega not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  if (identity && !omega) {
    sv::set_error("null pointer (omega: a factor is SV_FACTOR_IDENTITY)");
    return SV_ERR_ARG;
  }
  for (size_t j = 0; j < n_num + n_den; j++) {
    const sv_fr_factor& f = j < n_num ? num[j] : den[j - n_num];
    if (ranges_overlap(d_z, f.d_x, n * sizeof(sv_fe)) ||
        (f.kind == SV_FACTOR_COLUMN && ranges_overlap(d_z, f.d_y, n * sizeof(sv_fe)))) {
      sv::set_error("d_z overlaps a column (the last launch reads the columns again while it writes)");
      return SV_ERR_ARG;
    }
  }
  GpCall call{};
  call.num = num, call.n_num = n_num;
  call.den = den, call.n_den = n_den;
  call.n = n;
  call.z0 = *z0;
  call.omega = omega;
  call.form = form;
  call.invert = false;
  call.d_out = d_z;
  return grand_product_run(call, device, stream, out_total);
  SV_GUARD_END
}

int sv_bn254_fr_batch_invert_device(const sv_fe* d_in, sv_fe* d_out, size_t n, int form, int device,
                                    void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_in || !d_out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 15u) {
    sv::set_error("d_in and d_out must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (n == 0) {
    sv::set_error("the column should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > kGpMaxRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26", n);
    return SV_ERR_LEN;
  }
  if (d_in != d_out && ranges_overlap(d_in, d_out, n * sizeof(sv_fe))) {
    sv::set_error("d_out overlaps d_in without being d_in (in place is d_out == d_in)");
    return SV_ERR_ARG;
  }
  sv_fr_factor column{};
  column.d_x = d_in;
  column.kind = SV_FACTOR_PLAIN;
  GpCall call{};
  call.num = &column, call.n_num = 1;
  call.n = n;
  call.form = form;
  call.invert = true;
  call.d_out = d_out;
  return grand_product_run(call, device, stream, nullptr);
  SV_GUARD_END
}

// ---- permutation and lookup terms of the quotient numerator (csrc/quotient_terms.hip) ----
namespace {
// What the two calls share: the l columns, the challenges, the accumulator and the output.
struct TermsCommon {
  const sv_fe *d_l0, *d_l_last, *d_l_active;
  const sv_fe *beta, *gamma, *y;
  const sv_fe* d_acc_in;
  sv_fe* d_out;
  uint32_t log_n, log_ext;
};

// rule 2, the shared part
int terms_null_rules(const TermsCommon& c) {
  if (!c.d_out || !c.d_l0 || !c.d_l_last || !c.d_l_active || !c.beta || !c.gamma || !c.y) {
    sv::set_error("null pointer (d_out, an l column, beta, gamma or y)");
    return SV_ERR_ARG;
  }
  return SV_OK;
}

// rule 4, the shared part
int terms_align_rules(const TermsCommon& c) {
  if (((uintptr_t)c.d_out | (uintptr_t)c.d_l0 | (uintptr_t)c.d_l_last | (uintptr_t)c.d_l_active |
       (uintptr_t)c.d_acc_in) & 15u) {
    sv::set_error("d_out, d_acc_in and the l columns must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  return SV_OK;
}

// rules 6 to 8
int terms_size_rules(const TermsCommon& c, size_t count, size_t cap, const char* what) {
  if (c.log_ext > SV_EXT_LOG_MAX) {
    sv::set_error("log_ext = %u: beyond log_ext %d", c.log_ext, SV_EXT_LOG_MAX);
    return SV_ERR_LEN;
  }
  if (c.log_n > SV_NTT_MAX_LOG || c.log_n + c.log_ext > SV_NTT_MAX_LOG) {
    sv::set_error("log_n = %u, log_ext = %u: beyond 2^%d rows per column", c.log_n, c.log_ext, SV_NTT_MAX_LOG);
    return SV_ERR_LEN;
  }
  if (count > cap) {
    sv::set_error("%zu %s: a call takes at most %zu (call again on the running accumulator)", count, what, cap);
    return SV_ERR_LEN;
  }
  return SV_OK;
}

// rule 9, the shared part
int terms_scalar_rules(const TermsCommon& c) {
  if (!fr_reduced(*c.beta) || !fr_reduced(*c.gamma) || !fr_reduced(*c.y)) {
    sv::set_error("beta, gamma or y not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  return SV_OK;
}

// rule 12 for one input column
int terms_overlap_rule(const TermsCommon& c, const void* column) {
  const size_t bytes = (size_t(1) << (c.log_n + c.log_ext)) * sizeof(sv_fe);
  if (ranges_overlap(c.d_out, column, bytes)) {
    sv::set_error("d_out overlaps an input column (in place is d_out == d_acc_in only)");
    return SV_ERR_ARG;
  }
  return SV_OK;
}
int terms_overlap_rules(const TermsCommon& c) {
  SV_TRY(terms_overlap_rule(c, c.d_l0));
  SV_TRY(terms_overlap_rule(c, c.d_l_last));
  SV_TRY(terms_overlap_rule(c, c.d_l_active));
  if (c.d_acc_in && c.d_acc_in != c.d_out) SV_TRY(terms_overlap_rule(c, c.d_acc_in));
  return SV_OK;
}

// both calls past their checks and their launch: the error flag after the stream has drained
int terms_finish(DrainedLease* dl, size_t pinned_at) {
  Workspace* ws = dl->ws();
  SV_HIP(hipMemcpyAsync(ws->pinned + pinned_at, ws->buf + kQtErrOffset, sizeof(uint32_t), hipMemcpyDeviceToHost,
                        ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl->armed = false;
  uint32_t errv;
  memcpy(&errv, ws->pinned + pinned_at, sizeof errv);
  if (errv) {
    sv::set_error("invalid input: element not reduced mod r");
    return SV_ERR_ARG;
  }
  return SV_OK;
}
}  // namespace

int sv_bn254_fr_permutation_terms_device(const sv_fe* const* d_cols, const sv_fe* const* d_sigmas, const sv_fe* s,
                                         size_t m, size_t chunk, const sv_fe* const* d_z, const sv_fe* d_l0,
                                         const sv_fe* d_l_last, const sv_fe* d_l_active, const sv_fe* beta,
                                         const sv_fe* gamma, const sv_fe* y, const sv_fe* shift, int32_t last_rotation,
                                         const sv_fe* d_acc_in, sv_fe* d_out, uint32_t log_n, uint32_t log_ext,
                                         int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  const TermsCommon c{d_l0, d_l_last, d_l_active, beta, gamma, y, d_acc_in, d_out, log_n, log_ext};
  SV_TRY(terms_null_rules(c));
  if (!d_cols || !d_sigmas || !d_z || !s) {
    sv::set_error("null pointer (d_cols, d_sigmas, d_z or s)");
    return SV_ERR_ARG;
  }
  const size_t seen = std::min(m, (size_t)SV_TERMS_COLUMNS_MAX);  // entries beyond the cap are not looked at
  const size_t seen_z = chunk ? (seen + chunk - 1) / chunk : 0;
  uintptr_t bits = 0;
  for (size_t j = 0; j < seen; j++) {
    if (!d_cols[j] || !d_sigmas[j]) {
      sv::set_error("null pointer (permutation column %zu)", j);
      return SV_ERR_ARG;
    }
    bits |= (uintptr_t)d_cols[j] | (uintptr_t)d_sigmas[j];
  }
  for (size_t i = 0; i < seen_z; i++) {
    if (!d_z[i]) {
      sv::set_error("null pointer (d_z[%zu])", i);
      return SV_ERR_ARG;
    }
    bits |= (uintptr_t)d_z[i];
  }
  if (chunk == 0) {
    sv::set_error("chunk == 0: a z column covers at least one permutation column");
    return SV_ERR_ARG;
  }
  if (bits & 15u) {
    sv::set_error("the permutation columns, sigmas and z must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  SV_TRY(terms_align_rules(c));
  if (m == 0) {
    sv::set_error("the permutation should not be empty (m == 0)");
    return SV_ERR_EMPTY;
  }
  SV_TRY(terms_size_rules(c, m, SV_TERMS_COLUMNS_MAX, "permutation columns"));
  SV_TRY(terms_scalar_rules(c));
  for (size_t j = 0; j < m; j++)
    if (!fr_reduced(s[j])) {
      sv::set_error("s[%zu] not reduced mod the scalar field order", j);
      return SV_ERR_ARG;
    }
  QtPermCall call{};
  call.has_shift = false;
  if (shift) {
    SV_TRY(ext_shift_rules(*shift));
    sv_fe one = {{1, 0, 0, 0}};
    if (form == SV_MONTGOMERY) one = poly_fr_one();
    call.has_shift = memcmp(shift->l, one.l, sizeof one.l) != 0;
    call.shift = *shift;
  }
  if (last_rotation >= 0 || -(int64_t)last_rotation >= (int64_t(1) << log_n)) {
    sv::set_error("last_rotation = %d: it must satisfy -2^%u < last_rotation < 0", last_rotation, log_n);
    return SV_ERR_ARG;
  }
  const size_t n_z = (m + chunk - 1) / chunk;
  SV_TRY(terms_overlap_rules(c));
  for (size_t j = 0; j < m; j++) {
    SV_TRY(terms_overlap_rule(c, d_cols[j]));
    SV_TRY(terms_overlap_rule(c, d_sigmas[j]));
  }
  for (size_t i = 0; i < n_z; i++) SV_TRY(terms_overlap_rule(c, d_z[i]));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  call.d_cols = d_cols, call.d_sigmas = d_sigmas, call.s = s;
  call.m = m, call.chunk = chunk;
  call.d_z = d_z;
  call.d_l0 = d_l0, call.d_l_last = d_l_last, call.d_l_active = d_l_active;
  call.beta = *beta, call.gamma = *gamma, call.y = *y;
  call.last_rotation = last_rotation;
  call.d_acc_in = d_acc_in, call.d_out = d_out;
  call.log_n = log_n, call.log_ext = log_ext;
  call.form = form;
  const size_t tb = Workspace::aligned(quotient_terms_table_bytes(false));
  SV_TRY(ws->reserve(tb));
  SV_TRY(ws->reserve_pinned(tb + 256));
  SV_TRY(permutation_terms_enqueue(call, ws->buf, ws->pinned, ws->stream));
  return terms_finish(&dl, tb);
  SV_GUARD_END
}

int sv_bn254_fr_lookup_terms_device(const sv_fr_lookup* lookups, size_t n_lookups, const sv_fe* d_l0,
                                    const sv_fe* d_l_last, const sv_fe* d_l_active, const sv_fe* beta,
                                    const sv_fe* gamma, const sv_fe* y, const sv_fe* d_acc_in, sv_fe* d_out,
                                    uint32_t log_n, uint32_t log_ext, int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  const TermsCommon c{d_l0, d_l_last, d_l_active, beta, gamma, y, d_acc_in, d_out, log_n, log_ext};
  SV_TRY(terms_null_rules(c));
  if (!lookups) {
    sv::set_error("null pointer (lookup descriptors)");
    return SV_ERR_ARG;
  }
  const size_t seen = std::min(n_lookups, (size_t)SV_TERMS_LOOKUPS_MAX);  // descriptors beyond the cap are not looked at
  uintptr_t bits = 0;
  for (size_t l = 0; l < seen; l++) {
    const sv_fr_lookup& d = lookups[l];
    if (!d.d_z || !d.d_permuted_input || !d.d_permuted_table || !d.d_input || !d.d_table) {
      sv::set_error("null pointer (lookup %zu)", l);
      return SV_ERR_ARG;
    }
    bits |= (uintptr_t)d.d_z | (uintptr_t)d.d_permuted_input | (uintptr_t)d.d_permuted_table | (uintptr_t)d.d_input |
            (uintptr_t)d.d_table;
  }
  if (bits & 15u) {
    sv::set_error("the lookup columns must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  SV_TRY(terms_align_rules(c));
  if (n_lookups == 0) {
    sv::set_error("the lookups should not be empty (n_lookups == 0)");
    return SV_ERR_EMPTY;
  }
  SV_TRY(terms_size_rules(c, n_lookups, SV_TERMS_LOOKUPS_MAX, "lookups"));
  SV_TRY(terms_scalar_rules(c));
  SV_TRY(terms_overlap_rules(c));
  for (size_t l = 0; l < n_lookups; l++) {
    const sv_fr_lookup& d = lookups[l];
    SV_TRY(terms_overlap_rule(c, d.d_z));
    SV_TRY(terms_overlap_rule(c, d.d_permuted_input));
    SV_TRY(terms_overlap_rule(c, d.d_permuted_table));
    SV_TRY(terms_overlap_rule(c, d.d_input));
    SV_TRY(terms_overlap_rule(c, d.d_table));
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  QtLookupCall call{};
  call.lookups = lookups, call.n_lookups = n_lookups;
  call.d_l0 = d_l0, call.d_l_last = d_l_last, call.d_l_active = d_l_active;
  call.beta = *beta, call.gamma = *gamma, call.y = *y;
  call.d_acc_in = d_acc_in, call.d_out = d_out;
  call.log_n = log_n, call.log_ext = log_ext;
  call.form = form;
  const size_t tb = Workspace::aligned(quotient_terms_table_bytes(true));
  SV_TRY(ws->reserve(tb));
  SV_TRY(ws->reserve_pinned(tb + 256));
  SV_TRY(lookup_terms_enqueue(call, ws->buf, ws->pinned, ws->stream));
  return terms_finish(&dl, tb);
  SV_GUARD_END
}

// ---- expression programs: custom gates and theta-compression (csrc/expressions.hip) ----
namespace {
static_assert(sizeof(sv_fr_expr_op) == sizeof(ExprOp) && offsetof(sv_fr_expr_op, op) == offsetof(ExprOp, op) &&
                  offsetof(sv_fr_expr_op, zero) == offsetof(ExprOp, zero) &&
                  offsetof(sv_fr_expr_op, index) == offsetof(ExprOp, index) &&
                  offsetof(sv_fr_expr_op, rotation) == offsetof(ExprOp, rotation),
              "expr_plan.hpp walks the ABI's ops");
static_assert(SV_EXPR_COLUMN == kExprColumn && SV_EXPR_CONST == kExprConst && SV_EXPR_NEG == kExprNeg &&
                  SV_EXPR_ADD == kExprAdd && SV_EXPR_SUB == kExprSub && SV_EXPR_RSUB == kExprRsub &&
                  SV_EXPR_MUL == kExprMul && SV_EXPR_FOLD == kExprFold && SV_EXPR_STORE == kExprStore,
              "expr_plan.hpp's opcodes are the header's");
static_assert(SV_EXPR_OPS_MAX == kExprOpsMax && SV_EXPR_COLUMNS_MAX == kExprColumnsMax &&
                  SV_EXPR_CONSTS_MAX == kExprConstsMax && SV_EXPR_STORES_MAX == kExprStoresMax &&
                  SV_EXPR_STACK_MAX == kExprStackMax,
              "expr_plan.hpp's caps are the header's");

// rule 9 for one output against one other range of the call
int expr_overlap_rule(const void* out, const char* what, const void* other, size_t bytes) {
  if (ranges_overlap(out, other, bytes)) {
    sv::set_error("%s overlaps something else passed to the call (in place is d_out == d_acc_in only)", what);
    return SV_ERR_ARG;
  }
  return SV_OK;
}
}  // namespace

int sv_bn254_fr_expressions_device(const sv_fr_expr_op* program, size_t n_ops, const sv_fe* const* d_cols,
                                   size_t n_cols, const sv_fe* consts, size_t n_consts, sv_fe* const* d_stores,
                                   size_t n_stores, const sv_fe* y, const sv_fe* d_acc_in, sv_fe* d_out,
                                   uint32_t log_n, uint32_t log_ext, int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!program || (n_cols && !d_cols) || (n_consts && !consts) || (n_stores && !d_stores)) {
    sv::set_error("null pointer (program, d_cols, consts or d_stores)");
    return SV_ERR_ARG;
  }
  // entries beyond a cap are not looked at
  const size_t seen_cols = std::min(n_cols, (size_t)SV_EXPR_COLUMNS_MAX);
  const size_t seen_stores = std::min(n_stores, (size_t)SV_EXPR_STORES_MAX);
  uintptr_t bits = (uintptr_t)d_acc_in | (uintptr_t)d_out;
  for (size_t j = 0; j < seen_cols; j++) {
    if (!d_cols[j]) {
      sv::set_error("null pointer (d_cols[%zu])", j);
      return SV_ERR_ARG;
    }
    bits |= (uintptr_t)d_cols[j];
  }
  for (size_t j = 0; j < seen_stores; j++) {
    if (!d_stores[j]) {
      sv::set_error("null pointer (d_stores[%zu])", j);
      return SV_ERR_ARG;
    }
    bits |= (uintptr_t)d_stores[j];
  }
  if (bits & 15u) {
    sv::set_error("the columns, the stores, d_acc_in and d_out must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (n_ops == 0) {
    sv::set_error("the program should not be empty (n_ops == 0)");
    return SV_ERR_EMPTY;
  }
  if (log_ext > SV_EXT_LOG_MAX) {
    sv::set_error("log_ext = %u: beyond log_ext %d", log_ext, SV_EXT_LOG_MAX);
    return SV_ERR_LEN;
  }
  if (log_n > SV_NTT_MAX_LOG || log_n + log_ext > SV_NTT_MAX_LOG) {
    sv::set_error("log_n = %u, log_ext = %u: beyond 2^%d rows per column", log_n, log_ext, SV_NTT_MAX_LOG);
    return SV_ERR_LEN;
  }
  const struct { size_t count, cap; const char* what; } counts[] = {{n_ops, SV_EXPR_OPS_MAX, "ops"},
                                                                     {n_cols, SV_EXPR_COLUMNS_MAX, "columns"},
                                                                     {n_consts, SV_EXPR_CONSTS_MAX, "constants"},
                                                                     {n_stores, SV_EXPR_STORES_MAX, "stores"}};
  for (const auto& c : counts)
    if (c.count > c.cap) {
      sv::set_error("%zu %s: a call takes at most %zu", c.count, c.what, c.cap);
      return SV_ERR_LEN;
    }
  ExprPlan plan;
  size_t at = 0;
  const ExprFault fault = expr_walk(reinterpret_cast<const ExprOp*>(program), n_ops, n_cols, n_consts, n_stores, log_n,
                                    &plan, &at);
  if (fault != kExprOk) {
    if (at < n_ops)
      sv::set_error("op %zu (opcode %u, index %u, rotation %d): %s", at, (unsigned)program[at].op,
                    (unsigned)program[at].index, (int)program[at].rotation, expr_fault_text(fault));
    else
      sv::set_error("after op %zu, the last: %s", n_ops - 1, expr_fault_text(fault));
    return SV_ERR_ARG;
  }
  if (plan.folds && (!y || !d_out)) {
    sv::set_error("null pointer (y or d_out of a program that folds)");
    return SV_ERR_ARG;
  }
  if (plan.folds && !fr_reduced(*y)) {
    sv::set_error("y not reduced mod the scalar field order");
    return SV_ERR_ARG;
  }
  for (size_t j = 0; j < n_consts; j++)
    if (plan.const_used[j] && !fr_reduced(consts[j])) {
      sv::set_error("consts[%zu] not reduced mod the scalar field order", j);
      return SV_ERR_ARG;
    }
  const size_t bytes = (size_t(1) << (log_n + log_ext)) * sizeof(sv_fe);
  for (size_t k = 0; k <= n_stores; k++) {  // the written stores, then d_out
    const bool is_out = k == n_stores;
    if (is_out ? !plan.folds : !plan.store_used[k]) continue;
    const void* o = is_out ? (const void*)d_out : (const void*)d_stores[k];
    const char* what = is_out ? "d_out" : "a store";
    for (size_t j = 0; j < n_cols; j++) SV_TRY(expr_overlap_rule(o, what, d_cols[j], bytes));
    for (size_t j = 0; j < n_stores; j++)
      if (j != k) SV_TRY(expr_overlap_rule(o, what, d_stores[j], bytes));
    if (plan.folds && !is_out) SV_TRY(expr_overlap_rule(o, what, d_out, bytes));
    if (plan.folds && d_acc_in && !(is_out && d_acc_in == d_out)) SV_TRY(expr_overlap_rule(o, what, d_acc_in, bytes));
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  ExprCall call{};
  call.program = program, call.n_ops = n_ops;
  call.d_cols = d_cols, call.n_cols = n_cols;
  call.consts = consts, call.n_consts = n_consts;
  call.d_stores = d_stores, call.n_stores = n_stores;
  call.y = y;
  call.d_acc_in = plan.folds ? d_acc_in : nullptr, call.d_out = d_out;
  call.log_n = log_n, call.log_ext = log_ext;
  call.form = form;
  call.plan = &plan;
  const size_t tb = Workspace::aligned(expressions_table_bytes(n_ops));
  SV_TRY(ws->reserve(tb));
  SV_TRY(ws->reserve_pinned(tb + 256));
  SV_TRY(expressions_enqueue(call, ws->buf, ws->pinned, ws->stream));
  static_assert(kExprErrOffset == kQtErrOffset, "terms_finish reads the flag where this table keeps it");
  return terms_finish(&dl, tb);
  SV_GUARD_END
}

// ---- Fr sort and a lookup's permuted columns (csrc/lookup_permute.hip) ----
namespace {
// both entry points past their checks: the lease, the launches, the head
int lookup_permute_run(const LpCall& call, int device, void* stream, uint64_t* out_missing_row) {
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  SV_TRY(ws->reserve(lookup_permute_scratch_bytes(call.n, call.permute)));
  SV_TRY(ws->reserve_pinned(kLpHeadBytes));
  SV_TRY(lookup_permute_enqueue(call, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf, kLpHeadBytes, hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  uint32_t errv;
  uint64_t missing;
  memcpy(&errv, ws->pinned + kLpErrOffset, sizeof errv);
  memcpy(&missing, ws->pinned + kLpMissingOffset, sizeof missing);
  if (errv) {
    sv::set_error("invalid input: element not reduced mod r");
    return SV_ERR_ARG;
  }
  if (out_missing_row) *out_missing_row = missing ? UINT64_MAX - missing : UINT64_MAX;
  if (missing) {
    sv::set_error("row %llu of the permuted input holds a value that is not in table",
                  (unsigned long long)(UINT64_MAX - missing));
    return SV_ERR_ARG;
  }
  return SV_OK;
}
}  // namespace

int sv_bn254_fr_sort_device(const sv_fe* d_in, sv_fe* d_out, size_t n, int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_in || !d_out) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 15u) {
    sv::set_error("d_in and d_out must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (n == 0) {
    sv::set_error("the column should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > kLpMaxRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26", n);
    return SV_ERR_LEN;
  }
  if (d_in != d_out && ranges_overlap(d_in, d_out, n * sizeof(sv_fe))) {
    sv::set_error("d_out overlaps d_in without being d_in (in place is d_out == d_in)");
    return SV_ERR_ARG;
  }
  LpCall call{};
  call.d_in = d_in;
  call.n = n;
  call.form = form;
  call.permute = false;
  call.d_out = d_out;
  return lookup_permute_run(call, device, stream, nullptr);
  SV_GUARD_END
}

int sv_bn254_fr_lookup_permute_device(const sv_fe* d_input, const sv_fe* d_table, size_t n, int form,
                                      sv_fe* d_permuted_input, sv_fe* d_permuted_table, uint64_t* out_missing_row,
                                      int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (!d_input || !d_table || !d_permuted_input || !d_permuted_table) {
    sv::set_error("null pointer");
    return SV_ERR_ARG;
  }
  if (((uintptr_t)d_input | (uintptr_t)d_table | (uintptr_t)d_permuted_input | (uintptr_t)d_permuted_table) & 15u) {
    sv::set_error("the columns must be 16-byte aligned");
    return SV_ERR_ARG;
  }
  if (n == 0) {
    sv::set_error("the columns should not be empty");
    return SV_ERR_EMPTY;
  }
  if (n > kLpMaxRows) {
    sv::set_error("n = %zu exceeds the per-device limit 2^26", n);
    return SV_ERR_LEN;
  }
  const size_t bytes = n * sizeof(sv_fe);
  if (ranges_overlap(d_permuted_input, d_input, bytes) || ranges_overlap(d_permuted_input, d_table, bytes) ||
      ranges_overlap(d_permuted_table, d_input, bytes) || ranges_overlap(d_permuted_table, d_table, bytes)) {
    sv::set_error("an output overlaps an input column (the inputs are only read)");
    return SV_ERR_ARG;
  }
  if (ranges_overlap(d_permuted_input, d_permuted_table, bytes)) {
    sv::set_error("d_permuted_table overlaps d_permuted_input");
    return SV_ERR_ARG;
  }
  LpCall call{};
  call.d_in = d_input;
  call.d_table = d_table;
  call.n = n;
  call.form = form;
  call.permute = true;
  call.d_out = d_permuted_input;
  call.d_out_table = d_permuted_table;
  return lookup_permute_run(call, device, stream, out_missing_row);
  SV_GUARD_END
}

int sv_bn254_fr_lookup_permute_batch_device(const sv_fe* const* d_inputs, const sv_fe* const* d_tables, size_t count,
                                            size_t n, int form, uint32_t flags, sv_fe* const* d_permuted_inputs,
                                            sv_fe* const* d_permuted_tables, uint64_t* out_missing_rows,
                                            uint64_t* out_failed, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  // rules 1-4, the table slots and the scratch layout (csrc/lp_batch_plan.hpp)
  const LpBatchPlan plan = lp_batch_plan(reinterpret_cast<const void* const*>(d_inputs),
                                         reinterpret_cast<const void* const*>(d_tables), count, n, form, flags,
                                         reinterpret_cast<void* const*>(d_permuted_inputs),
                                         reinterpret_cast<void* const*>(d_permuted_tables));
  if (plan.rule != kLpbOk) {
    if (plan.rule == kLpbRuleArg && form != SV_CANONICAL && form != SV_MONTGOMERY) sv::set_error("bad form %d", form);
    else if (plan.rule == kLpbRuleOverlap) sv::set_error("%s: overlaps", plan.why);
    else sv::set_error("%s (count = %zu, n = %zu)", plan.why, count, n);
    return plan.rule == kLpbRuleEmpty ? SV_ERR_EMPTY : plan.rule == kLpbRuleLen ? SV_ERR_LEN : SV_ERR_ARG;
  }
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  DrainedLease dl(device, caller_stream(stream));
  if (!dl.lease.ok()) return SV_ERR_DEVICE;
  Workspace* ws = dl.ws();
  const size_t heads = count * kLpHeadBytes;
  SV_TRY(ws->reserve(plan.total));
  SV_TRY(ws->reserve_pinned(heads));
  LpBatchCall call{};
  call.plan = &plan;
  call.d_inputs = d_inputs;
  call.n = n;
  call.form = form;
  call.d_out_inputs = d_permuted_inputs;
  call.d_out_tables = d_permuted_tables;
  SV_TRY(lookup_permute_batch_enqueue(call, ws->buf, ws->stream));
  SV_HIP(hipMemcpyAsync(ws->pinned, ws->buf + plan.heads, heads, hipMemcpyDeviceToHost, ws->stream));
  SV_HIP(hipStreamSynchronize(ws->stream));
  dl.armed = false;
  uint32_t errv;
  memcpy(&errv, ws->pinned + kLpErrOffset, sizeof errv);
  if (errv & kLpErrNotReduced) {
    sv::set_error("invalid input: element not reduced mod r");
    return SV_ERR_ARG;
  }
  if (errv & kLpErrNotSorted) {
    sv::set_error("table not sorted: SV_LOOKUP_TABLES_SORTED promises ascending canonical order");
    return SV_ERR_ARG;
  }
  uint64_t failed = UINT64_MAX, failed_row = 0;
  for (size_t j = count; j-- > 0;) {
    uint64_t missing;
    memcpy(&missing, ws->pinned + j * kLpHeadBytes + kLpMissingOffset, sizeof missing);
    if (out_missing_rows) out_missing_rows[j] = missing ? UINT64_MAX - missing : UINT64_MAX;
    if (missing) failed = j, failed_row = UINT64_MAX - missing;
  }
  if (out_failed) *out_failed = failed;
  if (failed != UINT64_MAX) {
    sv::set_error("lookup %llu: row %llu of the permuted input holds a value that is not in table",
                  (unsigned long long)failed, (unsigned long long)failed_row);
    return SV_ERR_ARG;
  }
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_poseidon_permute(sv_fe* states, size_t n, int t, int form) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (t != 3 && t != 5) {
    sv::set_error("poseidon: unsupported width t = %d (3 or 5)", t);
    return SV_ERR_ARG;
  }
  if (n == 0) return SV_OK;
  if (!states) return SV_ERR_ARG;
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  const int dev = runtime_device_id(0);
  const size_t bytes = n * (size_t)t * sizeof(sv_fe);
  Staging sg(dev);
  SV_TRY(sg.init({bytes}));
  SV_TRY(sg.put(0, states, bytes));
  SV_TRY(poseidon_permute_device(sg.at(0), n, t, form, sg.lease.get()->stream));
  SV_TRY(sg.get(states, 0, bytes));
  SV_TRY(sg.sync());
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_poseidon_permute_device(sv_fe* d_states, size_t n, int t, int form, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  SV_HIP(hipSetDevice(device));
  return poseidon_permute_device(d_states, n, t, form, (hipStream_t)stream);
  SV_GUARD_END
}

int sv_bn254_poseidon_squeeze(sv_fe* states, const sv_fe* elements, const uint64_t* offsets, size_t n, int t,
                              int form, sv_fe* out) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (t != 3 && t != 5) {
    sv::set_error("poseidon: unsupported width t = %d (3 or 5)", t);
    return SV_ERR_ARG;
  }
  if (n == 0) return SV_OK;
  if (!states || !offsets) return SV_ERR_ARG;
  for (size_t j = 0; j < n; j++)
    if (offsets[j + 1] < offsets[j]) {
      sv::set_error("poseidon: offsets not non-decreasing at %zu", j);
      return SV_ERR_ARG;
    }
  const uint64_t total = offsets[n] - offsets[0];
  if (total && !elements) return SV_ERR_ARG;
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  const int dev = runtime_device_id(0);
  // rebase offsets so only elements[offsets[0] .. offsets[n]) travel
  std::vector<uint64_t> off(offsets, offsets + n + 1);
  for (auto& o : off) o -= offsets[0];
  const size_t sbytes = n * (size_t)t * sizeof(sv_fe);
  Staging sg(dev);
  SV_TRY(sg.init({sbytes, total * sizeof(sv_fe), (n + 1) * sizeof(uint64_t), n * sizeof(sv_fe)}));
  SV_TRY(sg.put(0, states, sbytes));
  if (total) SV_TRY(sg.put(1, elements + offsets[0], total * sizeof(sv_fe)));
  SV_TRY(sg.put(2, off.data(), (n + 1) * sizeof(uint64_t)));
  SV_TRY(poseidon_squeeze_device(sg.at(0), sg.at(1), sg.at<const uint64_t>(2), n, t, form, sg.at(3),
                                 sg.lease.get()->stream));
  SV_TRY(sg.get(states, 0, sbytes));
  if (out) SV_TRY(sg.get(out, 3, n * sizeof(sv_fe)));
  SV_TRY(sg.sync());
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_poseidon_squeeze_device(sv_fe* d_states, const sv_fe* d_elements, const uint64_t* d_offsets, size_t n,
                                     int t, int form, sv_fe* d_out, int device, void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  SV_HIP(hipSetDevice(device));
  return poseidon_squeeze_device(d_states, d_elements, d_offsets, n, t, form, d_out, (hipStream_t)stream);
  SV_GUARD_END
}

int sv_bn254_g1_decode(const uint8_t* data, size_t n, int encoding, int form, sv_g1_affine* out,
                       int64_t* first_invalid) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (encoding != SV_ENC_HALO2_COMPRESSED && encoding != SV_ENC_EVM) {
    sv::set_error("unknown point encoding %d", encoding);
    return SV_ERR_ARG;
  }
  int64_t fi = -1;
  if (first_invalid) *first_invalid = -1;
  if (n == 0) return SV_OK;
  if (!data || !out) return SV_ERR_ARG;
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  const int dev = runtime_device_id(0);
  const size_t rec = encoding == SV_ENC_EVM ? 64 : 32;
  Staging sg(dev);
  SV_TRY(sg.init({n * rec, n * sizeof(sv_g1_affine)}));
  SV_TRY(sg.put(0, data, n * rec));
  SV_TRY(sg.sync());
  SV_TRY(g1_decode_device(sg.at(0), n, encoding, rec, 0, form, dev, nullptr, sg.at(1), &fi));
  SV_TRY(sg.get(out, 1, n * sizeof(sv_g1_affine)));
  SV_TRY(sg.sync());
  if (first_invalid) *first_invalid = fi;
  if (fi >= 0) {
    sv::set_error("Invalid elliptic curve point encoding in proof (point %lld)", (long long)fi);
    return SV_ERR_ARG;
  }
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_g1_decode_device(const uint8_t* d_data, size_t n, int encoding, int form, int device, void* stream,
                              sv_g1_affine* d_out, int64_t* first_invalid) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  SV_HIP(hipSetDevice(device));
  int64_t fi = -1;
  SV_TRY(g1_decode_device(d_data, n, encoding, encoding == SV_ENC_EVM ? 64 : 32, 0, form, device,
                          caller_stream(stream), d_out, &fi));
  if (first_invalid) *first_invalid = fi;
  if (fi >= 0) {
    sv::set_error("Invalid elliptic curve point encoding in proof (point %lld)", (long long)fi);
    return SV_ERR_ARG;
  }
  return SV_OK;
  SV_GUARD_END
}

int sv_bn254_kzg_accumulators_from_limbs(const sv_fe* limbs, size_t n, int n_limbs, int bits, int form,
                                         sv_g1_affine* lhs, sv_g1_affine* rhs, int64_t* first_invalid) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (first_invalid) *first_invalid = -1;
  if (n == 0) return SV_OK;
  if (!limbs || !lhs || !rhs || n_limbs < 1) return SV_ERR_ARG;
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  const int dev = runtime_device_id(0);
  const size_t nl = n * 4 * (size_t)n_limbs;
  Staging sg(dev);
  SV_TRY(sg.init({nl * sizeof(sv_fe), n * sizeof(sv_g1_affine), n * sizeof(sv_g1_affine)}));
  SV_TRY(sg.put(0, limbs, nl * sizeof(sv_fe)));
  SV_TRY(sg.sync());
  int64_t fi = -1;
  SV_TRY(limbs_to_accumulators_device(sg.at(0), n, n_limbs, bits, form, dev, nullptr, sg.at(1), sg.at(2), &fi));
  SV_TRY(sg.get(lhs, 1, n * sizeof(sv_g1_affine)));
  SV_TRY(sg.get(rhs, 2, n * sizeof(sv_g1_affine)));
  SV_TRY(sg.sync());
  if (first_invalid) *first_invalid = fi;
  if (fi >= 0) {
    sv::set_error("accumulator %lld: limbs do not encode a canonical on-curve point", (long long)fi);
    return SV_ERR_ARG;
  }
  return SV_OK;
  SV_GUARD_END
}

namespace {
// 32-byte big-endian word -> canonical limbs; false when >= p
bool be_word(const uint8_t* w, F& out) {
  for (int k = 0; k < 4; k++) {
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v = (v << 8) | w[(3 - k) * 8 + b];
    out.l[k] = v;
  }
  return host::f_is_reduced(out);
}
bool g2_from_eip197(const uint8_t* r, sv_g2_affine* q) {
  F w[4];
  for (int i = 0; i < 4; i++)
    if (!be_word(r + 32 * i, w[i])) return false;
  q->x.c1 = fe_out(w[0]);
  q->x.c0 = fe_out(w[1]);
  q->y.c1 = fe_out(w[2]);
  q->y.c0 = fe_out(w[3]);
  return true;
}
}  // namespace

int sv_bn254_kzg_decide_eip197(const uint8_t* input, size_t n_checks, int num_gpus, int32_t* first_fail) noexcept {
  SV_GUARD_BEGIN
  (void)num_gpus;  // one device: the records are host memory and the check count is small
  if (n_checks == 0) {
    sv::set_error("accumulators should not be empty");
    return SV_ERR_EMPTY;
  }
  if (!input || !first_fail) return SV_ERR_ARG;
  constexpr size_t kRec = 0x180;
  sv_g2_affine g2, msg2;
  if (!g2_from_eip197(input + 64, &g2) || !g2_from_eip197(input + 256, &msg2)) {
    sv::set_error("EIP-197 record 0: G2 word >= p");
    return SV_ERR_ARG;
  }
  for (size_t i = 1; i < n_checks; i++)
    if (memcmp(input + i * kRec + 64, input + 64, 128) || memcmp(input + i * kRec + 256, input + 256, 128)) {
      sv::set_error("EIP-197 record %zu: G2 points differ from record 0 (one deciding key per call)", i);
      return SV_ERR_ARG;
    }
  // s_g2 = -(-s_g2): negate y (canonical)
  sv_g2_affine sg2 = msg2;
  {
    F y0 = fe_in(msg2.y.c0), y1 = fe_in(msg2.y.c1);
    sg2.y.c0 = fe_out(host::f_sub(F{}, y0));
    sg2.y.c1 = fe_out(host::f_sub(F{}, y1));
  }
  if (resolve_gpus(1) == 0) return SV_ERR_DEVICE;
  const int dev = runtime_device_id(0);
  Staging sg(dev);
  SV_TRY(sg.init({n_checks * kRec, n_checks * sizeof(sv_g1_affine), n_checks * sizeof(sv_g1_affine)}));
  SV_TRY(sg.put(0, input, n_checks * kRec));
  SV_TRY(sg.sync());
  int64_t bl = -1, br = -1;
  SV_TRY(g1_decode_device(sg.at(0), n_checks, SV_ENC_EVM, kRec, 0, SV_CANONICAL, dev, nullptr, sg.at(1), &bl));
  SV_TRY(g1_decode_device(sg.at(0), n_checks, SV_ENC_EVM, kRec, 192, SV_CANONICAL, dev, nullptr, sg.at(2), &br));
  int32_t ff = -1;
  SV_TRY(decide_run_device(&g2, &sg2, sg.at(1), sg.at(2), n_checks, SV_CANONICAL, dev, nullptr, &ff, nullptr,
                           nullptr));
  int64_t first = -1;
  for (int64_t c : {(int64_t)ff, bl, br})
    if (c >= 0 && (first < 0 || c < first)) first = c;
  *first_fail = (int32_t)first;
  return SV_OK;
  SV_GUARD_END
}

int sv_gen_scalars_device(sv_fe* d_scalars, size_t n, uint64_t seed, uint64_t start, int form, int device,
                          void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  return gen_scalars_device(d_scalars, n, seed, start, form, device, caller_stream(stream));
  SV_GUARD_END
}

int sv_gen_bases_device(sv_g1_affine* d_bases, size_t n, uint64_t seed, uint64_t start, int form, int device,
                        void* stream) noexcept {
  SV_GUARD_BEGIN
  SV_TRY(check_form(form));
  if (resolve_gpus(0) == 0) return SV_ERR_DEVICE;
  return gen_bases_device(d_bases, n, seed, start, form, device, caller_stream(stream));
  SV_GUARD_END
}

int sv_msm_last_stats(sv_msm_stats* out) noexcept {
  SV_GUARD_BEGIN
  if (!out) return SV_ERR_ARG;
  return msm_last_stats(out);
  SV_GUARD_END
}

int sv_kzg_last_kernel_ms(float* out) noexcept {
  if (!out) return SV_ERR_ARG;
  *out = decider_last_kernel_ms();
  return SV_OK;
}

}  // extern "C"
