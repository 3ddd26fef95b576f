// The host path a caller had before sv_bn254_fr_sort_device / sv_bn254_fr_lookup_permute_device: one
// thread, std::sort over canonical 4 x 64-bit limbs (compared from the top limb down) and halo2's
// permute_expression_pair as it is written there: an ordered map from table value to count, a walk
// over the sorted input, and pop() from the back of the repeated rows.  The keys are already
// canonical, so the conversion from Montgomery form (one multiplication per element, which the device
// call includes) is NOT counted here.
//
//   c++ -O2 -std=c++17 -o tools/ubench_host_lookup_permute tools/ubench_host_lookup_permute.cpp
//   tools/ubench_host_lookup_permute 16 20 24
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

using Key = std::array<uint64_t, 4>;

struct KeyLess {
  bool operator()(const Key& a, const Key& b) const {
    for (int i = 3; i >= 0; i--)
      if (a[i] != b[i]) return a[i] < b[i];
    return false;
  }
};

static uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// full width: below 2^253 < r, every byte but the top one uniform
static std::vector<Key> full_width(size_t n, uint64_t seed) {
  std::vector<Key> v(n);
  for (auto& k : v) {
    for (auto& l : k) l = splitmix(seed);
    k[3] &= 0x1FFFFFFFFFFFFFFFull;
  }
  return v;
}

static std::vector<Key> range16(size_t n, uint64_t seed, bool random) {
  std::vector<Key> v(n);
  const uint64_t mask = std::min<uint64_t>(0xFFFF, n - 1);  // a table of fewer than 2^16 rows holds 0 .. n - 1
  for (size_t i = 0; i < n; i++) v[i] = Key{(random ? splitmix(seed) : (uint64_t)i) & mask, 0, 0, 0};
  return v;
}

// halo2's loop; returns false where a value is missing
static bool permute(const std::vector<Key>& a, const std::vector<Key>& s, std::vector<Key>& ap, std::vector<Key>& sp) {
  const size_t n = a.size();
  ap = a;
  std::sort(ap.begin(), ap.end(), KeyLess());
  std::map<Key, uint32_t, KeyLess> left;
  for (const auto& k : s) left[k]++;
  sp.assign(n, Key{});
  std::vector<uint32_t> repeated;
  for (size_t i = 0; i < n; i++) {
    if (i == 0 || ap[i] != ap[i - 1]) {
      auto it = left.find(ap[i]);
      if (it == left.end() || it->second == 0) return false;
      it->second--;
      sp[i] = ap[i];
    } else {
      repeated.push_back((uint32_t)i);
    }
  }
  for (const auto& kv : left)
    for (uint32_t c = 0; c < kv.second; c++) {
      sp[repeated.back()] = kv.first;
      repeated.pop_back();
    }
  return repeated.empty();
}

template <class F>
static void run(const char* label, int lg, int reps, F&& body) {
  double best = 1e300, worst = 0, sum = 0;
  uint64_t probe = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    probe = body();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    best = std::min(best, ms), worst = std::max(worst, ms), sum += ms;
  }
  std::printf("# %s 2^%d: probe %08x\n", label, lg, (unsigned)(probe & 0xFFFFFFFFu));
  std::printf("%s 2^%d: %.3f ms (min %.3f max %.3f, %.1f ns per row)\n", label, lg, sum / reps, best, worst,
              sum / reps * 1e6 / (double)(size_t(1) << lg));
  std::fflush(stdout);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    const int lg = std::atoi(argv[i]);
    if (lg < 1 || lg > 26) continue;
    const size_t n = size_t(1) << lg;
    const int reps = lg <= 20 ? 3 : 1;
    const auto wide = full_width(n, 11), narrow = range16(n, 12, true), table16 = range16(n, 0, false);
    std::vector<Key> inputs(n);
    uint64_t seed = 13;
    for (auto& k : inputs) k = wide[splitmix(seed) % n];
    std::vector<Key> work, ap, sp;
    run("sort, full-width keys", lg, reps, [&] {
      work = wide;
      std::sort(work.begin(), work.end(), KeyLess());
      return work[n / 2][0];
    });
    run("sort, 16-bit keys", lg, reps, [&] {
      work = narrow;
      std::sort(work.begin(), work.end(), KeyLess());
      return work[n / 2][0];
    });
    run("permutation, full-width table", lg, reps, [&] {
      if (!permute(inputs, wide, ap, sp)) std::abort();
      return sp[n / 2][0];
    });
    run("permutation, 2^16-entry range table", lg, reps, [&] {
      if (!permute(narrow, table16, ap, sp)) std::abort();
      return sp[n / 2][0];
    });
  }
  return 0;
}
