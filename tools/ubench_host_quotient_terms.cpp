// Host microbenchmark: the permutation and lookup terms of the quotient numerator as a caller folds
// them on the CPU when the library has no device call for them -- one thread over csrc/field.hpp's
// host build (portable CIOS Montgomery Fr), Montgomery in and out, on extended columns of 2^K rows:
// the constraints of snark-verifier/src/system/halo2.rs:533-589 (6 columns in chunks of 3) and
// :632-651 (1 and 4 lookups), each folded onto an accumulator by acc <- acc y + c.  Rotations by one
// row of the original domain are 4 rows (log_ext = 2).  Context for tools/quotient_terms_bench.py,
// which runs this binary when it is there.
// Build: clang++ -O3 -std=c++17 -Isnark-verifier-axiom_amd/csrc tools/ubench_host_quotient_terms.cpp \
//          -o tools/ubench_host_quotient_terms
// Run:   tools/ubench_host_quotient_terms 18 22   (log2 rows; prints "<shape> 2^K: <median ms> ms")
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "field.hpp"

using sv::Fr;

static std::vector<Fr> column(size_t n, uint32_t tag) {
  std::vector<Fr> c(n);
  Fr v = Fr::one();
  for (uint32_t i = 0; i < tag + 2; i++) v = v + v + Fr::one();
  for (size_t i = 0; i < n; i++) c[i] = v = v * v + Fr::one();  // reduced, Montgomery
  return c;
}

template <class Fn>
static void timed(const char* shape, int lg, int reps, Fn fn) {
  std::vector<double> ms;
  for (int rep = 0; rep < reps; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t probe = fn();
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (rep == 0) printf("# %s 2^%d: last limb0 %08x\n", shape, lg, probe);
  }
  std::sort(ms.begin(), ms.end());
  printf("%s 2^%d: %.3f ms (min %.3f max %.3f, %.1f ns per row)\n", shape, lg, ms[ms.size() / 2], ms.front(),
         ms.back(), ms[ms.size() / 2] * 1e6 / (double)(size_t(1) << lg));
}

int main(int argc, char** argv) {
  constexpr size_t E = 4, M = 6, CHUNK = 3, NZ = 2, LAST = 6;
  for (int a = 1; a < argc; a++) {
    const int lg = atoi(argv[a]);
    if (lg < 4 || lg > 24) return 2;
    const size_t n = size_t(1) << lg, mask = n - 1;
    const int reps = lg >= 20 ? 1 : lg >= 18 ? 3 : 7;
    const Fr beta = column(1, 90)[0], gamma = column(1, 91)[0], omega = column(1, 92)[0], y = column(1, 94)[0];
    const std::vector<Fr> l0 = column(n, 40), l_last = column(n, 41), l_active = column(n, 42);
    std::vector<Fr> acc = column(n, 43);
    {
      std::vector<std::vector<Fr>> v, sg, z;
      Fr bd[M];
      for (uint32_t j = 0; j < M; j++) {
        v.push_back(column(n, j));
        sg.push_back(column(n, 10 + j));
        bd[j] = j ? bd[j - 1] * column(1, 93)[0] : beta;  // beta delta^j
      }
      for (uint32_t i = 0; i < NZ; i++) z.push_back(column(n, 20 + i));
      timed("permutation terms, 6 columns in chunks of 3", lg, reps, [&] {
        Fr x = column(1, 95)[0];  // the shift
        for (size_t j = 0; j < n; j++) {
          Fr r = acc[j] * y + l0[j] * (Fr::one() - z[0][j]);
          r = r * y + l_last[j] * (z[NZ - 1][j] * z[NZ - 1][j] - z[NZ - 1][j]);
          for (size_t i = 1; i < NZ; i++) r = r * y + l0[j] * (z[i][j] - z[i - 1][(j + n - LAST * E) & mask]);
          for (size_t i = 0; i < NZ; i++) {
            Fr left = z[i][(j + E) & mask], right = z[i][j];
            for (size_t t = i * CHUNK; t < std::min((i + 1) * CHUNK, M); t++) {
              left = left * (v[t][j] + beta * sg[t][j] + gamma);
              right = right * (v[t][j] + bd[t] * x + gamma);
            }
            r = r * y + l_active[j] * (left - right);
          }
          acc[j] = r;
          x = x * omega;
        }
        return acc[n - 1].v[0];
      });
    }
    for (size_t L : {size_t(1), size_t(4)}) {
      std::vector<std::vector<Fr>> c;
      for (uint32_t i = 0; i < 5 * L; i++) c.push_back(column(n, 50 + i));
      char shape[64];
      snprintf(shape, sizeof shape, "lookup terms, %zu lookup%s", L, L > 1 ? "s" : "");
      timed(shape, lg, reps, [&] {
        for (size_t j = 0; j < n; j++) {
          Fr r = acc[j];
          for (size_t l = 0; l < L; l++) {
            const Fr z = c[5 * l][j], zn = c[5 * l][(j + E) & mask];
            const Fr pa = c[5 * l + 1][j], pam = c[5 * l + 1][(j + n - E) & mask], ps = c[5 * l + 2][j];
            const Fr d = pa - ps;
            r = r * y + l0[j] * (Fr::one() - z);
            r = r * y + l_last[j] * (z * z - z);
            r = r * y + l_active[j] * (zn * (pa + beta) * (ps + gamma) -
                                       z * (c[5 * l + 3][j] + beta) * (c[5 * l + 4][j] + gamma));
            r = r * y + l0[j] * d;
            r = r * y + l_active[j] * d * (pa - pam);
          }
          acc[j] = r;
        }
        return acc[n - 1].v[0];
      });
    }
  }
  return 0;
}
