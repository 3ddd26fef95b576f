// The batched-MSM host planning (csrc/msm_batch_plan.hpp) and the batched affine conversion
// (csrc/host_ec.hpp) on their own, for tests/test_msm_batch_plan.py.
//   msm_batch_plan_check COUNT MAX_TERMS IDS BIDX [SVGPU_NAME=VALUE ...]   one msm_batch_device call
//   msm_batch_plan_check split LEN [LEN ...] [SVGPU_NAME=VALUE ...]        batch_split over MSMs of these lengths
//   msm_batch_plan_check fixed                                             msm_batch_fixed_device's layout
//   msm_batch_plan_check slot                                              the fused-launch slot, a fixed script
//   msm_batch_plan_check affine K [K ...]                                  x_to_affine_batch over the points K G
//   msm_batch_plan_check -                                                 one such case per line of stdin
// IDS, BIDX: 1 if the call passes an id map / a base-index array.  The switches are read from the
// environment as the library reads them; NAME=VALUE arguments set them for that case only.  One
// JSON line per case.  A call case prints the plan and the layout its route reserves: batch_buffers,
// or on HostHorner msm_batch_windows_host's (with the caller's offsets, and "single" for one MSM
// without).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host_ec.hpp"
#include "msm_batch_plan.hpp"

using namespace sv;

static const char* batch_route_name(BatchRoute r) {
  switch (r) {
    case BatchRoute::HostHorner: return "HostHorner";
    case BatchRoute::Fused: return "Fused";
    case BatchRoute::BucketHorner: return "BucketHorner";
    case BatchRoute::QuadWindows: return "QuadWindows";
    case BatchRoute::LaneWindows: return "LaneWindows";
  }
  return "?";
}

static void print_layout(const char* key, const MsmLayout& L) {
  printf(", \"%s\": [", key);
  for (int i = 0; i < L.count; i++)
    printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", L.bufs[i].name, L.bufs[i].off, L.bufs[i].bytes);
  printf("], \"%s_total\": %zu", key, L.total);
}

static void print_buffers(const char* prefix, const BatchBuffers& b) {
  const std::string ws = std::string(prefix) + "buffers", pin = std::string(prefix) + "pinned";
  print_layout(ws.c_str(), b.ws);
  print_layout(pin.c_str(), b.pin);
  printf(", \"%sback_bytes\": %zu", prefix, b.back_bytes);
}

static int call_case(const std::vector<std::string>& a, const BatchTuning& t) {
  if (a.size() < 4) {
    fprintf(stderr, "usage: COUNT MAX_TERMS IDS BIDX [SVGPU_NAME=VALUE ...]\n");
    return 2;
  }
  const size_t count = strtoull(a[0].c_str(), nullptr, 10), max_terms = strtoull(a[1].c_str(), nullptr, 10);
  const BatchPlan p = batch_plan(count, max_terms, atoi(a[2].c_str()) != 0, atoi(a[3].c_str()) != 0, t);
  printf("{\"route\": \"%s\", \"c\": %d, \"W\": %u, \"WG\": %u, \"horner\": \"%s\", \"bw\": %u, \"spin_max\": %u, "
         "\"nT\": %zu, \"nflag\": %zu, \"dig_bytes\": %zu, \"pts_bytes\": %zu, \"window_bits\": %d",
         batch_route_name(p.route), p.c, p.W, p.WG, p.quad_horner ? "quad" : "wave", p.bw, p.spin_max, p.nT, p.nflag,
         p.dig_bytes, p.pts_bytes, batch_window_bits(max_terms, t));
  if (p.route == BatchRoute::HostHorner) {
    printf(", \"host_ok\": %d", batch_windows_host_ok(count, max_terms) ? 1 : 0);
    print_buffers("", batch_windows_host_buffers(count, max_terms, false));
    if (count == 1) print_buffers("single_", batch_windows_host_buffers(count, max_terms, true));
  } else {
    print_buffers("", batch_buffers(p));
    if (p.route == BatchRoute::Fused) {
      const BatchPlan q = batch_without_slot(p);
      printf(", \"without_slot\": {\"route\": \"%s\", \"nT\": %zu, \"nflag\": %zu, \"total\": %zu}",
             batch_route_name(q.route), q.nT, q.nflag, batch_buffers(q).ws.total);
    }
  }
  printf("}\n");
  return 0;
}

static int split_case(const std::vector<std::string>& a, const BatchTuning& t) {
  std::vector<uint64_t> off{7};  // any start: only the differences count
  for (size_t i = 1; i < a.size(); i++)
    if (a[i].find('=') == std::string::npos) off.push_back(off.back() + strtoull(a[i].c_str(), nullptr, 10));
  std::vector<uint32_t> small_ids, big_ids;
  size_t max_small = 0;
  batch_split(off.data(), off.size() - 1, t, &small_ids, &big_ids, &max_small);
  printf("{\"small\": [");
  for (size_t i = 0; i < small_ids.size(); i++) printf("%s%u", i ? ", " : "", small_ids[i]);
  printf("], \"big\": [");
  for (size_t i = 0; i < big_ids.size(); i++) printf("%s%u", i ? ", " : "", big_ids[i]);
  printf("], \"max_small\": %zu}\n", max_small);
  return 0;
}

static int slot_case() {
  FuseSlot a, b, c, d;
  const bool first = a.acquire(3), second = b.acquire(3), other = c.acquire(4), alias = d.acquire(67);
  a.release();
  const bool after_release = b.acquire(3);
  bool scoped;
  {
    FuseSlot e;
    scoped = e.acquire(5);
  }  // the destructor releases
  FuseSlot f;
  const bool after_scope = f.acquire(5);
  printf("{\"first\": %d, \"second_same_device\": %d, \"other_device\": %d, \"device_67_while_3_held\": %d, "
         "\"after_release\": %d, \"scoped\": %d, \"after_scope\": %d}\n",
         first, second, other, alias, after_release, scoped, after_scope);
  return 0;
}

static void print_limbs(const uint64_t* v, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%s\"%016llx\"", i ? ", " : "", (unsigned long long)v[i]);
}

// the points K G in XYZZ with ZZ != 1 (double-and-add from the generator), through the batched
// conversion and through one x_to_affine each, in both forms
static int affine_case(const std::vector<std::string>& a) {
  const host::F one = host::f_one();
  const host::Xyzz G{one, host::f_dbl(one), one, one};
  std::vector<host::Xyzz> pts;
  for (size_t i = 1; i < a.size(); i++) {
    const uint64_t k = strtoull(a[i].c_str(), nullptr, 10);
    host::Xyzz r = host::x_identity();
    for (int bit = 63; bit >= 0; bit--) {
      r = host::x_dbl(r);
      if ((k >> bit) & 1) r = host::x_add(r, G);
    }
    pts.push_back(r);
  }
  const size_t n = pts.size();
  printf("{\"n\": %zu", n);
  for (int mont = 0; mont < 2; mont++) {
    std::vector<uint64_t> batch(8 * n + 1, 0xabababababababab), each(8 * n, 0);
    host::x_to_affine_batch(pts.data(), n, mont != 0, batch.data());
    for (size_t k = 0; k < n; k++) {
      host::F x, y;
      host::x_to_affine(pts[k], x, y);
      if (!mont) x = host::f_from_mont(x), y = host::f_from_mont(y);
      memcpy(&each[8 * k], x.l, 32);
      memcpy(&each[8 * k + 4], y.l, 32);
    }
    printf(", \"%s\": {\"batch\": [", mont ? "montgomery" : "canonical");
    print_limbs(batch.data(), 8 * n);
    printf("], \"each\": [");
    print_limbs(each.data(), 8 * n);
    printf("], \"guard_intact\": %d}", batch[8 * n] == 0xabababababababab ? 1 : 0);
  }
  printf("}\n");
  return 0;
}

static int run_case(const std::vector<std::string>& a) {
  if (a.empty()) return 2;
  std::vector<std::string> set;
  for (const std::string& w : a) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) continue;
    set.push_back(w.substr(0, eq));
    setenv(set.back().c_str(), w.c_str() + eq + 1, 1);
  }
  const BatchTuning t = batch_tuning();
  for (const std::string& s : set) unsetenv(s.c_str());
  if (a[0] == "split") return split_case(a, t);
  if (a[0] == "slot") return slot_case();
  if (a[0] == "affine") return affine_case(a);
  if (a[0] == "fixed") {
    printf("{\"route\": \"fixed\"");
    print_buffers("", batch_fixed_buffers());
    printf("}\n");
    return 0;
  }
  return call_case(a, t);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "-")) {
    std::string line;
    while (std::getline(std::cin, line)) {
      std::istringstream is(line);
      std::vector<std::string> a;
      for (std::string w; is >> w;) a.push_back(w);
      if (a.empty()) continue;
      if (int rc = run_case(a)) return rc;
    }
    return 0;
  }
  return run_case(std::vector<std::string>(argv + 1, argv + argc));
}
