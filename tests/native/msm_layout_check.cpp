// The single-MSM host planning (csrc/msm_plan.hpp) on its own, for tests/test_msm_layout.py.
//   msm_layout_check N MODE FORM [PIECES] [SVGPU_NAME=VALUE ...]     one case
//   msm_layout_check -                                              one such case per line of stdin
// MODE: device | split | fed | resident | resident_fed; FORM: 0 canonical, 1 Montgomery; PIECES:
// MsmFeed::pieces (0: the default schedule).  The switches are read from the environment as the
// library reads them; NAME=VALUE arguments set them for that case only.  One JSON line per case: the
// plan, the piece bounds, per-piece K / T, every buffer as [name, offset, bytes], the totals and
// the event slots the mode uses.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "msm_plan.hpp"

using namespace sv;

static void print_bufs(const MsmLayout& L) {
  for (int i = 0; i < L.count; i++)
    printf("%s[\"%s\", %zu, %zu]", i ? ", " : "", L.bufs[i].name, L.bufs[i].off, L.bufs[i].bytes);
}

static int run_case(const std::vector<std::string>& a) {
  if (a.size() < 3) {
    fprintf(stderr, "usage: N MODE FORM [PIECES] [SVGPU_NAME=VALUE ...]\n");
    return 2;
  }
  const size_t n = strtoull(a[0].c_str(), nullptr, 10);
  const std::string& mode = a[1];
  MsmMode m;
  m.canonical = atoi(a[2].c_str()) == 0;
  m.fed = mode == "fed" || mode == "resident_fed";
  m.resident = mode == "resident" || mode == "resident_fed";
  if (!m.fed && !m.resident && mode != "device" && mode != "split") {
    fprintf(stderr, "bad mode %s\n", mode.c_str());
    return 2;
  }
  std::vector<std::string> set;
  for (size_t i = 3; i < a.size(); i++) {
    const size_t eq = a[i].find('=');
    if (eq == std::string::npos) {
      m.pieces = atoi(a[i].c_str());
    } else {
      set.push_back(a[i].substr(0, eq));
      setenv(set.back().c_str(), a[i].c_str() + eq + 1, 1);
    }
  }
  if (mode == "split") {
    set.push_back("SVGPU_MSM_SPLIT");
    setenv("SVGPU_MSM_SPLIT", "1", 1);
  }
  const MsmTuning t = msm_tuning();
  for (const std::string& s : set) unsetenv(s.c_str());
  MsmPlan p = msm_plan(n, t);
  if (m.resident) p.r29 = 1;
  const MsmShape s = msm_shape(n, m, p, t);
  const MsmBuffers b = msm_buffers(n, m, p, s);

  printf("{\"plan\": {\"c\": %d, \"W\": %u, \"B\": %u, \"nbt\": %u, \"K\": %u, \"T\": %u, \"logL\": %u, \"J\": %u, "
         "\"logJ\": %u, \"NG\": %u, \"glv\": %d, \"npts\": %zu, \"phi64\": %d, \"tree\": %d, \"r29\": %d}",
         p.c, p.W, p.B, p.nbt, p.K, p.T, p.logL, p.J, p.logJ, p.NG, p.glv ? 1 : 0, p.npts, p.phi64, p.tree, p.r29);
  printf(", \"bounds\": [");
  for (size_t i = 0; i < s.pb.size(); i++) printf("%s%zu", i ? ", " : "", s.pb[i]);
  printf("], \"K\": [");
  for (int k = 0; k < s.pieces; k++) printf("%s%u", k ? ", " : "", s.K[k]);
  printf("], \"T\": [");
  for (int k = 0; k < s.pieces; k++) printf("%s%u", k ? ", " : "", s.T[k]);
  printf("], \"shape\": {\"ep\": %u, \"Tmax\": %u, \"tst_total\": %llu, \"entries\": %llu, \"piece_entries\": %llu, "
         "\"split\": %d, \"nwh\": [%u, %u], \"Th\": [%u, %u], \"nwb\": %u, \"nblk\": %u, \"conv\": %d, \"tab4\": %zu, "
         "\"nfinal\": %zu, \"gparts\": %u, \"nerr\": %zu, \"keep_halves\": %d, \"rec_bytes\": %zu, \"ntree\": %zu}",
         s.ep, s.Tmax, (unsigned long long)s.tst_total, (unsigned long long)s.entries,
         (unsigned long long)s.piece_entries, s.split ? 1 : 0, s.nwh[0], s.nwh[1], s.Th[0], s.Th[1], s.nwb, s.nblk,
         s.conv ? 1 : 0, s.tab4, s.nfinal, s.gparts, s.nerr, s.keep_halves ? 1 : 0, s.rec_bytes, s.ntree);
  printf(", \"err_offset\": %zu, \"buffers\": [", b.err);
  print_bufs(b.ws);
  printf("], \"total\": %zu, \"in_buffers\": [", b.ws.total);
  print_bufs(b.in);
  printf("], \"in_total\": %zu, \"events\": {", b.in.total);

  namespace ev = ev_slot;
  printf("\"start\": %d, \"sort_mid\": %d, \"acc_begin\": %d, \"acc_end\": %d, \"fix_end\": %d, \"end\": %d", ev::kStart,
         ev::kSortMid, ev::kAccBegin, ev::kAccEnd, ev::kFixEnd, ev::kEnd);
  if (m.fed) {
    printf(", \"fed_fork\": %d", ev::kFedFork);
    for (int k = 0; k < s.pieces; k++) {
      printf(", \"piece_scalars_%d\": %d, \"piece_sorted_%d\": %d", k, ev::piece_scalars(k), k, ev::piece_sorted(k));
      if (!m.resident) printf(", \"piece_bases_%d\": %d", k, ev::piece_bases(k));
    }
  } else if (s.split) {
    printf(", \"half_b_acc_begin\": %d, \"half_b_acc_end\": %d, \"half_b_end\": %d", ev::kHalfBAccBegin,
           ev::kHalfBAccEnd, ev::kHalfBEnd);
  } else if (!m.resident) {
    printf(", \"sort_fork\": %d, \"sort_join\": %d", ev::kSortFork, ev::kSortJoin);
  }
  printf("}, \"max_pieces\": %d, \"event_slots\": %d}\n", kMaxPieces, (int)ev::kCount);
  return 0;
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
