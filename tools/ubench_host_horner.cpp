// Host microbenchmark: the synthetic division q = (p - p(z)) / (X - z) a caller runs on the CPU when
// the library has no device division -- one thread, one dependent chain of n Fr products
// (csrc/host_poseidon.hpp's fr::mul / fr::add), Montgomery in and out.  Context for
// tools/kzg_open_bench.py, which runs this binary when it is there.
// Build: clang++ -O3 -std=c++17 -Isnark-verifier-axiom_amd/csrc tools/ubench_host_horner.cpp -o tools/ubench_host_horner
// Run:   tools/ubench_host_horner 16 18 20      (log2 sizes; prints "2^k: <median ms> ms" per size)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_poseidon.hpp"

int main(int argc, char** argv) {
  using namespace sv::host::fr;
  for (int a = 1; a < argc; a++) {
    const int lg = atoi(argv[a]);
    if (lg < 1 || lg > 26) return 2;
    const size_t n = size_t(1) << lg;
    std::vector<E> p(n), q(n);
    E x = to_mont(E{{0x5ca1a125ull, 2, 3, 4}});
    const E z = to_mont(E{{0x1234567ull, 5, 6, 7}});
    for (size_t i = 0; i < n; i++) p[i] = x = mul(x, z);  // reduced, Montgomery
    std::vector<double> ms;
    for (int rep = 0; rep < 7; rep++) {
      const auto t0 = std::chrono::steady_clock::now();
      E h = E{{0, 0, 0, 0}};
      for (size_t i = n; i-- > 0;) {
        q[i] = h;  // q_i = h_{i+1}; q[n-1] = h_n = 0 is not part of the quotient
        h = add(p[i], mul(z, h));
      }
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      if (rep == 0) printf("# 2^%d: p(z) limb0 %016llx\n", lg, (unsigned long long)h.l[0]);
    }
    std::sort(ms.begin(), ms.end());
    printf("2^%d: %.3f ms (min %.3f max %.3f, %.1f ns per coefficient)\n", lg, ms[ms.size() / 2], ms.front(),
           ms.back(), ms[ms.size() / 2] * 1e6 / (double)n);
  }
  return 0;
}
