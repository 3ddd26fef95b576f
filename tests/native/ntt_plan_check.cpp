// Host check of csrc/ntt_plan.hpp (no HIP, no BN254): the pass widths, and the whole multi-pass
// decomposition run over the toy field F_65537 with the plan's own index and exponent functions,
// against the O(n^2) DFT.  65537 = 2^16 + 1 has 2^16-th roots of unity and 3 generates its
// multiplicative group, so 3 plays the part of the tables' root (root_log = 16).
//   usage: ntt_plan_check <default tile log>
// Built by tests/test_ntt_plan.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../snark-verifier-axiom_amd/csrc/ntt_plan.hpp"

using namespace sv;

namespace {

constexpr uint32_t Q = 65537, kRootLog = 16;
int g_fail = 0;

#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (g_fail < 20) {                    \
        fprintf(stderr, "FAIL %s: ", #cond); \
        fprintf(stderr, __VA_ARGS__);       \
        fprintf(stderr, "\n");              \
      }                                     \
      g_fail++;                             \
    }                                       \
  } while (0)

uint32_t mul(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)a * b % Q); }
uint32_t add(uint32_t a, uint32_t b) { return (a + b) % Q; }
uint32_t sub(uint32_t a, uint32_t b) { return (a + Q - b) % Q; }
uint32_t pw(uint32_t a, uint64_t e) {
  uint32_t r = 1;
  for (; e; e >>= 1, a = mul(a, a))
    if (e & 1) r = mul(r, a);
  return r;
}
uint32_t inv(uint32_t a) { return pw(a, Q - 2); }

std::vector<uint32_t> g_root[2];  // powers of 3 and of 1/3: the "tables"

// the transform's definition: out[j] = sum_i in[i] (g w^j)^i, or its inverse
std::vector<uint32_t> dft(const std::vector<uint32_t>& in, uint32_t k, bool inverse, uint32_t g) {
  const uint32_t n = 1u << k;
  std::vector<uint32_t> out(n);
  const std::vector<uint32_t>& rt = g_root[inverse ? 1 : 0];
  std::vector<uint32_t> x = in;
  if (!inverse)
    for (uint32_t i = 0; i < n; i++) x[i] = mul(x[i], pw(g, i));
  for (uint32_t j = 0; j < n; j++) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < n; i++)
      acc = add(acc, mul(x[i], rt[(((uint64_t)i * j) & (n - 1)) << (kRootLog - k)]));
    out[j] = acc;
  }
  if (inverse) {
    const uint32_t ninv = inv(n % Q), ginv = inv(g);
    for (uint32_t i = 0; i < n; i++) out[i] = mul(out[i], mul(ninv, pw(ginv, i)));
  }
  return out;
}

// the kernels' decomposition, column by column, through the plan's functions only
std::vector<uint32_t> planned(const std::vector<uint32_t>& in, const NttPlan& plan, bool inverse, uint32_t g) {
  const uint32_t k = plan.k, n = 1u << k;
  const std::vector<uint32_t>& rt = g_root[inverse ? 1 : 0];
  std::vector<uint32_t> cur = in;
  if (!inverse)
    for (uint32_t i = 0; i < n; i++) cur[i] = mul(cur[i], pw(g, i));
  for (uint32_t s = 0; s < ntt_launches(plan); s++) {
    const uint32_t w = ntt_width(plan, s);
    const uint32_t ss = ntt_src_stride_log(plan, s), ds = ntt_dst_stride_log(plan, s);
    std::vector<uint32_t> nxt(n, 0);
    std::vector<uint8_t> read(n, 0), written(n, 0);
    for (uint32_t col = 0; col < (1u << ntt_cols_log(plan, s)); col++) {
      std::vector<uint32_t> tile(1u << w);
      const uint32_t sb = ntt_src_base(plan, s, col), db = ntt_dst_base(plan, s, col);
      for (uint32_t m = 0; m < (1u << w); m++) {
        const uint32_t at = sb + (m << ss);
        CHECK(at < n && !read[at], "k %u pass %u col %u: load %u", k, s, col, at);
        if (at >= n) return nxt;
        read[at] = 1;
        tile[m] = cur[at];
      }
      for (int st = (int)w - 1; st >= 0; st--)
        for (uint32_t b = 0; b < (1u << w) / 2; b++) {
          uint32_t m, j;
          ntt_stage_pair(b, (uint32_t)st, &m, &j);
          const uint32_t p = tile[m], q = tile[m + (1u << st)];
          tile[m] = add(p, q);
          tile[m + (1u << st)] = mul(sub(p, q), rt[ntt_stage_exp(j, (uint32_t)st, kRootLog)]);
        }
      for (uint32_t f = 0; f < (1u << w); f++) {
        uint32_t v = tile[ntt_bitrev(f, w)];
        if (!ntt_is_last(plan, s)) v = mul(v, rt[ntt_root_exp(plan, ntt_twiddle_exp(plan, s, col, f), kRootLog)]);
        const uint32_t at = db + (f << ds);
        CHECK(at < n && !written[at], "k %u pass %u col %u: store %u", k, s, col, at);
        if (at >= n) return nxt;
        written[at] = 1;
        nxt[at] = v;
        // a pass before the last one writes where it read, so it may run in place
        if (!ntt_is_last(plan, s)) CHECK(at == sb + (f << ss), "k %u pass %u: not in place", k, s);
      }
    }
    cur.swap(nxt);
  }
  if (inverse) {
    const uint32_t ninv = inv(n % Q), ginv = inv(g);
    for (uint32_t i = 0; i < n; i++) cur[i] = mul(cur[i], mul(ninv, pw(ginv, i)));
  }
  return cur;
}

void check_widths(uint32_t k, uint32_t T) {
  const NttPlan p = ntt_make_plan(k, T);
  uint32_t sum = 0;
  for (uint32_t s = 0; s < p.passes; s++) {
    sum += p.width[s];
    CHECK(p.width[s] >= 1 && p.width[s] <= T, "k %u T %u: width[%u] = %u", k, T, s, p.width[s]);
    CHECK(ntt_block_cols_log(p, s) + p.width[s] <= kNttBlockLog, "k %u T %u: block too large", k, T);
  }
  CHECK(sum == k, "k %u T %u: widths sum to %u", k, T, sum);
  CHECK(p.passes == (k + T - 1) / T, "k %u T %u: %u passes", k, T, p.passes);
  CHECK(ntt_launches(p) == (p.passes ? p.passes : 1u), "k %u T %u: launches", k, T);
  for (uint32_t s = p.passes; s < kNttMaxLog; s++) CHECK(p.width[s] == 0, "k %u T %u: stray width", k, T);
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

// Part 2: the exponents and index maps alone at sizes no toy field reaches.  For an input index i
// and an output index j the passes must contribute, in total, i j mod 2^k; the element must travel
// from position i to position j through the plan's bases and strides.
void check_exponents(uint32_t k, uint32_t T, int samples) {
  const NttPlan p = ntt_make_plan(k, T);
  const uint64_t mask = (1ull << k) - 1;
  for (int it = 0; it < samples; it++) {
    const uint32_t i = (uint32_t)(rnd() & mask), j = (uint32_t)(rnd() & mask);
    uint64_t e = 0;
    uint32_t pos = i;
    for (uint32_t s = 0; s < ntt_launches(p); s++) {
      const uint32_t w = ntt_width(p, s), L = ntt_lo_bits(p, s), H = ntt_hi_bits(p, s);
      const uint32_t m = (pos >> L) & ((1u << w) - 1u), f = (j >> H) & ((1u << w) - 1u);
      CHECK(m == ((i >> L) & ((1u << w) - 1u)), "k %u pass %u: digit %u of i moved", k, s, s);
      // the column that holds the element going in, as the load side numbers it
      uint32_t col;
      if (!ntt_is_last(p, s)) col = ((pos >> (w + L)) << L) | (pos & ((1u << L) - 1u));
      else col = j & ((1u << ntt_cols_log(p, s)) - 1u);
      CHECK(ntt_src_base(p, s, col) + (m << ntt_src_stride_log(p, s)) == pos, "k %u pass %u: load of %u", k, s, pos);
      // the twiddle against (partial output index) x (remaining input index) in 64 bits
      const uint64_t want = (((uint64_t)f << H) * (uint64_t)(i & ((1u << L) - 1u))) & mask;
      CHECK(ntt_twiddle_exp(p, s, col, f) == want, "k %u pass %u col %u f %u: twiddle", k, s, col, f);
      CHECK(ntt_root_exp(p, (uint32_t)want, 26) == want << (26 - k), "k %u: root exponent", k);
      e += ((uint64_t)m * f) << (k - w);  // the tile's own DFT: omega_n^(2^(k - w) m f)
      e += want;
      pos = ntt_dst_base(p, s, col) + (f << ntt_dst_stride_log(p, s));
    }
    CHECK(pos == j, "k %u: i %u lands at %u, not %u", k, i, pos, j);
    CHECK((e & mask) == (((uint64_t)i * j) & mask), "k %u: exponents of (%u, %u)", k, i, j);
  }
  // a stage's root as a power of the tables' root: omega_{2d}^j, d = 2^st
  for (uint32_t st = 0; st < T; st++)
    for (int it = 0; it < 8; it++) {
      const uint32_t jj = (uint32_t)(rnd() & ((1u << st) - 1u));
      CHECK(ntt_stage_exp(jj, st, 26) == (uint64_t)jj << (25 - st), "stage %u", st);
    }
}

}  // namespace

int main(int argc, char** argv) {
  const uint32_t T0 = argc > 1 ? (uint32_t)atoi(argv[1]) : 10;
  if (T0 < 1 || T0 > kNttBlockLog) {
    fprintf(stderr, "bad default tile log %u\n", T0);
    return 2;
  }
  for (int d = 0; d < 2; d++) {
    g_root[d].resize(1u << kRootLog);
    const uint32_t r = d ? inv(3) : 3;
    g_root[d][0] = 1;
    for (uint32_t i = 1; i < (1u << kRootLog); i++) g_root[d][i] = mul(g_root[d][i - 1], r);
  }
  CHECK(g_root[0][1u << 15] == Q - 1, "3 is not a generator");

  int runs = 0;
  for (uint32_t k = 0; k <= 16; k++) {
    std::vector<uint32_t> tiles;
    if (k <= 12)
      for (uint32_t T = 1; T <= (k < 6 ? k : 6); T++) tiles.push_back(T);
    tiles.push_back(T0);
    for (uint32_t T : tiles) check_widths(k, T);
    if (k > 12) continue;  // the O(n^2) reference stops here
    std::vector<uint32_t> in(1u << k);
    for (auto& v : in) v = (uint32_t)(rnd() % Q);
    if (k >= 2) in[1] = 0, in[(1u << k) - 1] = Q - 1;
    for (int inverse = 0; inverse < 2; inverse++)
      for (uint32_t g : {1u, 3u}) {
        const std::vector<uint32_t> want = dft(in, k, inverse != 0, g);
        for (uint32_t T : tiles) {
          const std::vector<uint32_t> got = planned(in, ntt_make_plan(k, T), inverse != 0, g);
          CHECK(got == want, "k %u T %u inverse %d shift %u: transform differs", k, T, inverse, g);
          runs++;
        }
      }
  }
  for (uint32_t k : {20u, 21u, 26u})
    for (uint32_t T : {T0, 1u, 3u, 7u}) check_exponents(k, T, 2000);

  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("ntt_plan_check ok: %d transforms, default tile log %u\n", runs, T0);
  return 0;
}
