// Pippenger MSM entry points (see msm.hip; the plan: msm_plan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/svgpu.h"
#include "host_ec.hpp"
#include "msm_plan.hpp"  // MsmPlan, msm_plan, kSmallMsmTerms

namespace sv {

// Device-resident MSM on `device`; result (XYZZ, Montgomery) on the host.
int msm_run_device(const void* d_bases, const void* d_scalars, size_t n, int form, int device,
                   hipStream_t stream, host::Xyzz* out);

// Host-fed MSM (the host-buffer entry points): the caller's inputs reach HBM in `pieces` pieces on
// the workspace's copy stream.  stage_scalars(lo, hi, d_scalars, copy_stream, ready) and
// stage_bases(lo, hi, d_bases, copy_stream, ready) issue the transfers of points [lo, hi) into the
// given device pointers and record `ready` after them.  They are called in that order per piece,
// with the piece's sort enqueued in between: pageable transfers block the calling thread, so the
// sort then runs while the bases are still in flight.
struct MsmFeed {
  int pieces = 0;             // equal pieces (0: split, else the default schedule)
  std::vector<double> split;  // piece weights from 2^18 points when SVGPU_H2D_* are unset

  std::function<int(size_t lo, size_t hi, void* d_scalars, hipStream_t copy_stream, hipEvent_t ready)> stage_scalars;
  std::function<int(size_t lo, size_t hi, void* d_bases, hipStream_t copy_stream, hipEvent_t ready)> stage_bases;
};
int msm_run_fed(size_t n, int form, int device, const MsmFeed& feed, host::Xyzz* out);

// Resident base set: N affine points kept on one device in the form the pipeline consumes, 208 B
// per point -- the Montgomery rows (64 B, the small route's input) and the 29-bit chain's table of
// 2 N records of 72 B, P_i at record i and phi(P_i) = (beta x_i, y_i) at record N + i.
// msm_resident_prepare fills both from N rows in `form` (d_rows may equal d_rows_m) and returns
// SV_ERR_ARG for a coordinate not below p.  The runs compute sum_i scalars[i] * set[off + i] over
// rows [off, off + n) with the plan of n: no base is converted, checked or tabulated per call, the
// 29-bit chain is used whatever SVGPU_ACC_R29 says, and a fed call stages scalars only
// (feed.stage_bases is not called).
constexpr size_t kResidentRowBytes = 64, kResidentTabBytes = 144;
struct MsmResident {
  const void* rows;  // N Montgomery rows
  const void* vtab;  // 2 N table records
  size_t N;
  size_t off;        // first row of this call
};
int msm_resident_prepare(const void* d_rows, size_t n, int form, int device, hipStream_t stream, void* d_rows_m,
                         void* d_vtab);
int msm_run_resident_device(const MsmResident& set, const void* d_scalars, size_t n, int form, int device,
                            hipStream_t stream, host::Xyzz* out);
int msm_run_resident_fed(const MsmResident& set, size_t n, int form, int device, const MsmFeed& feed,
                         host::Xyzz* out);

int msm_last_stats(sv_msm_stats* out);

}  // namespace sv
