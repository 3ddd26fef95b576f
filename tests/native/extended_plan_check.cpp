// Host check of csrc/ext_plan.hpp (no HIP, no BN254): the coset LDE and the quotient's divide /
// inverse / truncate run over the toy field F_65537 through the NTT plan's own index functions and
// the new predicates (live input index, kept destination index, table index), the way the kernels
// of csrc/ntt.hip run them, against the O(n^2) definitions.  65537 = 2^16 + 1: 3 generates the
// multiplicative group and plays the part of the tables' root (root_log = 16); every shift used has
// order 2^16, so g^(2^K) != 1 for every K here.
//   usage: extended_plan_check
// Built by tests/test_extended_plan.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../snark-verifier-axiom_amd/csrc/ext_plan.hpp"

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
uint32_t root_of(uint32_t k) { return k ? g_root[0][1u << (kRootLog - k)] : 1u; }

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return g_rng;
}

// one pass of the plan over `cur` (2^K entries), as planned() of ntt_plan_check.cpp runs it;
// lde_ext >= 0 (pass 0 of an LDE with e = lde_ext): the butterflies of the top ext_zero_stages stages
// take their upper partner as a known zero, and skip the pairs ext_pair_dead names (and check both)
void run_pass(const NttPlan& plan, uint32_t s, bool inverse, int lde_ext, std::vector<uint32_t>& cur) {
  const uint32_t ext_log = lde_ext < 0 ? 0u : (uint32_t)lde_ext;
  const uint32_t zero_stages = lde_ext < 0 ? 0u : ext_zero_stages(plan, ext_log);
  const uint32_t K = plan.k, N = 1u << K;
  const std::vector<uint32_t>& rt = g_root[inverse ? 1 : 0];
  const uint32_t w = ntt_width(plan, s);
  std::vector<uint32_t> nxt(N, 0);
  std::vector<uint8_t> written(N, 0);
  for (uint32_t col = 0; col < (1u << ntt_cols_log(plan, s)); col++) {
    std::vector<uint32_t> tile(1u << w);
    for (uint32_t m = 0; m < (1u << w); m++) tile[m] = cur.at(ext_src_index(plan, s, col, m));
    for (int st = (int)w - 1; st >= 0; st--)
      for (uint32_t b = 0; b < (1u << w) / 2; b++) {
        uint32_t m, j;
        ntt_stage_pair(b, (uint32_t)st, &m, &j);
        const uint32_t p = tile[m], q = tile[m + (1u << st)];
        if ((uint32_t)st + zero_stages >= w) {
          CHECK(q == 0, "K %u pass %u stage %d: the upper partner is %u", K, s, st, q);
          if (ext_pair_dead(plan, ext_log, (uint32_t)st, m)) {
            CHECK(p == 0, "K %u pass %u stage %d entry %u: a dead pair holds %u", K, s, st, m, p);
            continue;
          }
          tile[m + (1u << st)] = mul(p, rt[ntt_stage_exp(j, (uint32_t)st, kRootLog)]);
          continue;
        }
        tile[m] = add(p, q);
        tile[m + (1u << st)] = mul(sub(p, q), rt[ntt_stage_exp(j, (uint32_t)st, kRootLog)]);
      }
    for (uint32_t f = 0; f < (1u << w); f++) {
      uint32_t v = tile[ntt_bitrev(f, w)];
      if (!ntt_is_last(plan, s)) v = mul(v, rt[ntt_root_exp(plan, ntt_twiddle_exp(plan, s, col, f), kRootLog)]);
      const uint32_t at = ext_dst_index(plan, s, col, f);
      CHECK(at < N && !written[at], "K %u pass %u col %u: store %u", K, s, col, at);
      if (at >= N) return;
      written[at] = 1;
      nxt[at] = v;
    }
  }
  cur.swap(nxt);
}

// ---- the LDE ----
std::vector<uint32_t> lde_definition(const std::vector<uint32_t>& a, uint32_t k, uint32_t e, uint32_t g) {
  const uint32_t n = 1u << k, N = 1u << (k + e), w = root_of(k + e);
  std::vector<uint32_t> out(N);
  for (uint32_t j = 0; j < N; j++) {
    const uint32_t x = mul(g, pw(w, j));
    uint32_t acc = 0;
    for (uint32_t i = n; i-- > 0;) acc = add(mul(acc, x), a[i]);
    out[j] = acc;
  }
  return out;
}

// `a` has exactly n entries (vector::at and ASan watch the bound): pass 0 loads live indices only
std::vector<uint32_t> lde_planned(const std::vector<uint32_t>& a, uint32_t k, uint32_t e, uint32_t T, uint32_t g) {
  const uint32_t K = k + e, N = 1u << K;
  const NttPlan plan = ntt_make_plan(K, T);
  std::vector<uint32_t> image(N, 0xdead);  // pass 0 must overwrite all of it
  std::vector<uint8_t> seen(N, 0);
  const uint32_t w = ntt_width(plan, 0);
  for (uint32_t col = 0; col < (1u << ntt_cols_log(plan, 0)); col++) {
    const bool dead = ext_col_dead(plan, col, k);
    bool live_so_far = true;
    for (uint32_t m = 0; m < (1u << w); m++) {
      const uint32_t i = ext_src_index(plan, 0, col, m);
      CHECK(i < N && !seen[i], "k %u e %u T %u: index %u", k, e, T, i);
      if (i >= N) return image;
      seen[i] = 1;
      const bool live = ext_live(i, k);
      CHECK(!(dead && live), "k %u e %u T %u: a dead column holds the live index %u", k, e, T, i);
      CHECK(live_so_far || !live, "k %u e %u T %u col %u: live entries are no prefix", k, e, T, col);
      live_so_far = live;
      image[i] = live ? mul(a.at(i), pw(g, i)) : 0;
    }
  }
  for (uint32_t i = 0; i < N; i++) CHECK(seen[i], "k %u e %u T %u: index %u never loaded", k, e, T, i);
  for (uint32_t s = 0; s < ntt_launches(plan); s++)
    run_pass(plan, s, false, s == 0 ? (int)e : -1, image);
  return image;
}

// ---- the quotient ----
// h = the inverse coset transform of N_j / t(g w^j), cut to `keep` coefficients
std::vector<uint32_t> quotient_definition(const std::vector<uint32_t>& numer, uint32_t k, uint32_t e, uint32_t g,
                                          uint32_t keep) {
  const uint32_t K = k + e, N = 1u << K, n = 1u << k, w = root_of(K);
  std::vector<uint32_t> q(N), out(keep);
  for (uint32_t j = 0; j < N; j++) q[j] = mul(numer[j], inv(sub(pw(mul(g, pw(w, j)), n), 1)));
  const uint32_t winv = inv(w), ginv = inv(g), ninv = inv(N % Q);
  for (uint32_t i = 0; i < keep; i++) {
    uint32_t acc = 0;
    for (uint32_t j = 0; j < N; j++) acc = add(acc, mul(q[j], pw(winv, (uint64_t)i * j)));
    out[i] = mul(acc, mul(ninv, pw(ginv, i)));
  }
  return out;
}

// `out` has exactly `keep` entries
std::vector<uint32_t> quotient_planned(const std::vector<uint32_t>& numer, uint32_t k, uint32_t e, uint32_t T,
                                       uint32_t g, uint32_t keep) {
  const uint32_t K = k + e, N = 1u << K, n = 1u << k;
  const NttPlan plan = ntt_make_plan(K, T);
  std::vector<uint32_t> table(1u << e);
  for (uint32_t i = 0; i < (1u << e); i++) table[i] = inv(sub(mul(pw(g, n), pw(root_of(e), i)), 1));
  std::vector<uint32_t> image(N);
  const uint32_t w = ntt_width(plan, 0);
  for (uint32_t col = 0; col < (1u << ntt_cols_log(plan, 0)); col++)
    for (uint32_t m = 0; m < (1u << w); m++) {
      const uint32_t i = ext_src_index(plan, 0, col, m);
      const uint32_t ti = ext_table_index(plan, col, m, e);
      CHECK(ti == (i & ((1u << e) - 1u)), "k %u e %u T %u: table index of %u", k, e, T, i);
      if (ext_table_shared(plan, e)) CHECK(ti == ext_table_index(plan, col, 0, e), "k %u e %u T %u: not shared", k, e, T);
      image.at(i) = mul(numer.at(i), table.at(ti));
    }
  const uint32_t launches = ntt_launches(plan);
  for (uint32_t s = 0; s + 1 < launches; s++) run_pass(plan, s, true, -1, image);
  // the last pass, with the cut on its store
  std::vector<uint32_t> full = image;
  run_pass(plan, launches - 1, true, -1, full);
  std::vector<uint32_t> out(keep, 0xdead);
  const uint32_t s = launches - 1, wl = ntt_width(plan, s);
  uint32_t stored = 0;
  for (uint32_t col = 0; col < (1u << ntt_cols_log(plan, s)); col++)
    for (uint32_t f = 0; f < (1u << wl); f++) {
      const uint32_t at = ext_dst_index(plan, s, col, f);
      if (!ext_kept(at, keep)) continue;
      out.at(at) = mul(full.at(at), mul(inv(N % Q), pw(inv(g), at)));
      stored++;
    }
  CHECK(stored == keep, "k %u e %u T %u: %u of %u stored", k, e, T, stored, keep);
  return out;
}

// ---- the predicates alone at K = 26 ----
void check_predicates(uint32_t k, uint32_t e, uint32_t T, int samples) {
  const uint32_t K = k + e;
  const NttPlan plan = ntt_make_plan(K, T);
  const uint64_t mask = (1ull << K) - 1, n = 1ull << k;
  const uint32_t w = ntt_width(plan, 0), L = ntt_lo_bits(plan, 0);
  const bool one_pass = ntt_launches(plan) == 1;
  CHECK(ext_zero_stages(plan, e) == (e < w ? e : w), "K %u e %u T %u: zero stages", K, e, T);
  CHECK(ext_table_shared(plan, e) == ((one_pass ? 0 : L) >= e), "K %u e %u T %u: shared", K, e, T);
  for (int it = 0; it < samples; it++) {
    uint32_t i = (uint32_t)(rnd() & mask);
    if (it % 4 == 1) i = (uint32_t)((n - 1 + (it % 8 == 1)) & mask);  // the last live and the first dead index
    const uint32_t m = one_pass ? i : i >> L, col = one_pass ? 0 : i & ((1u << L) - 1u);
    CHECK(ext_src_index(plan, 0, col, m) == i, "K %u T %u: load of %u", K, T, i);
    CHECK(ext_live(i, k) == ((uint64_t)i < n), "k %u e %u: live(%u)", k, e, i);
    CHECK(ext_table_index(plan, col, m, e) == (uint32_t)((uint64_t)i % (1ull << e)), "k %u e %u: table(%u)", k, e, i);
    if (ext_table_shared(plan, e)) CHECK(ext_table_index(plan, col, m, e) == (col & ((1u << e) - 1u)), "shared %u", i);
    if (!one_pass) CHECK(ext_col_dead(plan, col, k) == ((uint64_t)col >= n), "k %u e %u T %u: dead(%u)", k, e, T, col);
    else CHECK(!ext_col_dead(plan, col, k), "k %u e %u: the only column is dead", k, e);
    // a tile entry with one of the top zero_stages bits set is padding
    for (uint32_t z = 0; z < ext_zero_stages(plan, e); z++)
      if ((m >> (w - 1 - z)) & 1u) CHECK(!ext_live(i, k), "k %u e %u T %u: entry %u of stage %u is live", k, e, T, m, z);
    // the store side of the last pass
    const uint32_t j = (uint32_t)(rnd() & mask), s = ntt_launches(plan) - 1, cl = ntt_cols_log(plan, s);
    const uint32_t dcol = j & ((1u << cl) - 1u), f = j >> cl;
    CHECK(ext_dst_index(plan, s, dcol, f) == j, "K %u T %u: store of %u", K, T, j);
    for (uint64_t pieces : {1ull, 1ull << e, (rnd() % (1ull << e)) + 1})
      CHECK(ext_kept(j, pieces << k) == ((uint64_t)j < pieces * n), "k %u e %u: kept(%u, %llu)", k, e, j,
            (unsigned long long)pieces);
  }
}

}  // namespace

int main() {
  for (int d = 0; d < 2; d++) {
    g_root[d].resize(1u << kRootLog);
    const uint32_t r = d ? inv(3) : 3;
    g_root[d][0] = 1;
    for (uint32_t i = 1; i < (1u << kRootLog); i++) g_root[d][i] = mul(g_root[d][i - 1], r);
  }
  CHECK(g_root[0][1u << 15] == Q - 1, "3 is not a generator");

  int ldes = 0, quotients = 0;
  for (uint32_t k = 0; k <= 6; k++)
    for (uint32_t e = 0; e <= 4; e++) {
      const uint32_t n = 1u << k, N = 1u << (k + e);
      std::vector<uint32_t> a(n), numer(N);
      for (auto& v : a) v = (uint32_t)(rnd() % Q);
      for (auto& v : numer) v = (uint32_t)(rnd() % Q);
      a[n - 1] = Q - 1;
      for (uint32_t g : {1u, 3u, 243u}) {
        const std::vector<uint32_t> want = lde_definition(a, k, e, g);
        for (uint32_t T = 1; T <= 4; T++) {
          CHECK(lde_planned(a, k, e, T, g) == want, "k %u e %u T %u shift %u: LDE differs", k, e, T, g);
          ldes++;
        }
      }
      for (uint32_t g : {3u, 243u}) {
        CHECK(pw(g, N) != 1, "shift %u meets the domain", g);
        const std::vector<uint32_t> want = quotient_definition(numer, k, e, g, N);
        for (uint32_t pieces = 1; pieces <= (1u << e); pieces++) {
          const std::vector<uint32_t> cut(want.begin(), want.begin() + pieces * n);
          for (uint32_t T = 1; T <= 4; T++) {
            CHECK(quotient_planned(numer, k, e, T, g, pieces * n) == cut, "k %u e %u T %u pieces %u shift %u: quotient differs",
                  k, e, T, pieces, g);
            quotients++;
          }
        }
      }
    }
  for (uint32_t e : {0u, 1u, 2u, 5u, 8u})
    for (uint32_t T : {10u, 1u, 3u, 7u}) check_predicates(26 - e, e, T, 2000);
  check_predicates(4, 8, 10, 2000);   // two passes, the whole top digit padding
  check_predicates(2, 8, 10, 2000);   // one pass

  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("extended_plan_check ok: %d extensions, %d quotients\n", ldes, quotients);
  return 0;
}
