// Test harness (not part of libsvgpu): the redundant-limb differences of csrc/field29.hpp (sub_lazy)
// and the bucket chain's steps that multiply them (csrc/curve29.hpp's madd_live / dbl_start), on the
// host for tests/test_field29_lazy.py.  Values travel as hex integers below 2^261; a result is
// printed as its 9 raw limbs, most significant first, 8 hex digits each (a redundant limb may use
// more than 29 bits).
//   sublazy      stdin "K a b" (K = 2 or 8)        -> limbs of sub_lazy<K>(a, b)
//   msum         stdin "a0 q x3 a1 ppp"            -> mul_sum2(a0, sub_lazy<8>(q, x3), a1, sub_lazy<2>(0, ppp))
//                                                     and the same product over sub<8> / sub<2>
//   prod         stdin "a b"                       -> mul(a, b), sqr(a), mul_sub<8>(a, b, 0)
//   step         stdin "X Y ZZ ZZZ x2 y2 neg"      -> the loop's step: start for an identity state,
//                                                     else madd_live (doubling -> dbl_start, a
//                                                     cancellation zeroes ZZ), then the special code
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "curve29.hpp"

using namespace sv::r29;

static F parse(const std::string& h) {  // hex integer (below 2^261) -> normalized limbs
  F r = zero();
  int bit = 0;
  for (int k = (int)h.size() - 1; k >= 0 && h[k] != 'x'; k--, bit += 4) {
    const char c = h[k];
    const uint32_t d = c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10;
    r.v[bit / 29] |= (d << (bit % 29)) & MASK;
    if (bit % 29 > 25 && bit / 29 + 1 < L) r.v[bit / 29 + 1] |= d >> (29 - bit % 29);
  }
  return r;
}
static void pr(const F& a, const char* end) {
  for (int i = L - 1; i >= 0; i--) printf("%08x", a.v[i]);
  printf("%s", end);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  char b[7][80];
  if (mode == "sublazy") {
    int k;
    while (scanf("%d %79s %79s", &k, b[0], b[1]) == 3) {
      const F x = parse(b[0]), y = parse(b[1]);
      pr(k == 2 ? sub_lazy<2>(x, y) : sub_lazy<8>(x, y), "\n");
    }
  } else if (mode == "msum") {
    while (scanf("%79s %79s %79s %79s %79s", b[0], b[1], b[2], b[3], b[4]) == 5) {
      const F a0 = parse(b[0]), q = parse(b[1]), x3 = parse(b[2]), a1 = parse(b[3]), ppp = parse(b[4]);
      pr(mul_sum2(a0, sub_lazy<8>(q, x3), a1, sub_lazy<2>(zero(), ppp)), " ");
      pr(mul_sum2(a0, sub<8>(q, x3), a1, sub<2>(zero(), ppp)), "\n");
    }
  } else if (mode == "prod") {
    while (scanf("%79s %79s", b[0], b[1]) == 2) {
      const F x = parse(b[0]), y = parse(b[1]);
      pr(mul(x, y), " "), pr(sqr(x), " "), pr(mul_sub<8>(x, y, zero()), "\n");
    }
  } else if (mode == "step") {
    int neg;
    while (scanf("%79s %79s %79s %79s %79s %79s %d", b[0], b[1], b[2], b[3], b[4], b[5], &neg) == 7) {
      const Xyzz st{parse(b[0]), parse(b[1]), parse(b[2]), parse(b[3])};
      const F x2 = parse(b[4]), y2 = parse(b[5]);
      Xyzz r;
      int special = 0;
      if (is_identity(st)) {
        r = start(x2, y2, neg != 0);
      } else {
        r = madd_live(st, x2, y2, neg != 0, special);
        if (special == 2) r = dbl_start(x2, y2, neg != 0);
        else if (special == 1) r.ZZ = zero();
      }
      pr(r.X, " "), pr(r.Y, " "), pr(r.ZZ, " "), pr(r.ZZZ, " ");
      printf("%d\n", special);
    }
  } else {
    fprintf(stderr, "usage: field29lazy sublazy|msum|step < cases\n");
    return 2;
  }
  return 0;
}
