// CPU check of the fused family evaluators' domain and routes (csrc/small_layout.h: small_family_fused_supported).
// Walks n 1..40, d 1..3, K 1..4 and the three kernel families (0 Gaussian, 1 Matern, 2 Matern + spline):
//   - small_family_fused_supported is true exactly for family 1 or 2, d = 1, 1 <= n <= 32, and K = 2 where the family is 2
//     (every carve of these shapes fits: the largest, the search instance at n = 32, K = 4, is summed by hand below);
//   - the four route functions that take the option -- small_route(Op::Loglik), small_route_sets, small_route_chain,
//     small_route_nm --, called as capi.hip calls them with the option on, `gauss || supported`, say Reg there;
//   - called with the plain `gauss` flag, as with the option off, they say what they said before the option existed: Reg for
//     the Gaussian family at every shape of the walk, and Blocked / Blocked / Unsupported / Unsupported for the other two;
//   - with the option on and the shape outside the domain (n = 33 included) a 1-D family keeps exactly those four answers.
// Built and run by tests/test_family_fused_layout.py (also once with -fsanitize=address,undefined).  Prints the counts, then "ok".
#include <cstdio>
#include <cstdlib>

#include "small_layout.h"

using namespace ccgp;

#define CHECK(cond)                                                                                         \
  do {                                                                                                      \
    if (!(cond)) {                                                                                          \
      std::printf("FAILED %s (line %d): family %d n %d d %d K %d\n", #cond, __LINE__, g_fam, g_n, g_d, g_K); \
      std::exit(1);                                                                                         \
    }                                                                                                       \
  } while (0)
static int g_fam, g_n, g_d, g_K;

int main() {
  long supported = 0, cells = 0, gauss_reg = 0, family_kept = 0;
  for (int fam = 0; fam < 3; ++fam)
    for (int n = 1; n <= 40; ++n)
      for (int d = 1; d <= 3; ++d)
        for (int K = 1; K <= 4; ++K) {
          g_fam = fam; g_n = n; g_d = d; g_K = K;
          ++cells;
          const bool want = (fam == 1 || (fam == 2 && K == 2)) && d == 1 && n >= 1 && n <= 32;
          const bool got = small_family_fused_supported(fam, n, d, K);
          CHECK(got == want);
          const bool gauss = fam == 0;
          // option off: the plain flag
          const Route l0 = small_route(Op::Loglik, gauss, n, d, K), s0 = small_route_sets(gauss, n, d, K),
                      c0 = small_route_chain(gauss, n, d, K), m0 = small_route_nm(gauss, n, d, K);
          if (gauss) {
            CHECK(l0 == Route::Reg && s0 == Route::Reg && c0 == Route::Reg && m0 == Route::Reg);
            ++gauss_reg;
          } else {
            CHECK(l0 == Route::Blocked && s0 == Route::Blocked && c0 == Route::Unsupported && m0 == Route::Unsupported);
          }
          // option on: what capi.hip passes
          const bool flag = gauss || got;
          const Route l1 = small_route(Op::Loglik, flag, n, d, K), s1 = small_route_sets(flag, n, d, K),
                      c1 = small_route_chain(flag, n, d, K), m1 = small_route_nm(flag, n, d, K);
          if (got) {
            CHECK(l1 == Route::Reg && s1 == Route::Reg && c1 == Route::Reg && m1 == Route::Reg);
            ++supported;
          } else {
            CHECK(l1 == l0 && s1 == s0 && c1 == c0 && m1 == m0);
            if (!gauss) ++family_kept;
          }
          // every other decision takes the family's own flag, whatever the option says: none of them is Reg for a 1-D family
          if (!gauss) {
            CHECK(small_route(Op::Predict, gauss, n, d, K) == Route::Blocked);
            CHECK(small_route(Op::Inverse, gauss, n, d, K) == Route::Blocked);
            CHECK(small_route_loo(gauss, n, d, K) == Route::Blocked);
            CHECK(small_route_profile_grad_sets(gauss, n, d, K) == Route::Blocked);
            CHECK(small_route_fit(gauss, n, d, K) == Route::Unsupported);
          }
        }
  // the domain ends at kFamilyFusedMaxN for every K the evaluator takes
  g_fam = 1; g_d = 1;
  for (int K = 1; K <= kMaxK; ++K) {
    g_K = K; g_n = kFamilyFusedMaxN;
    CHECK(small_family_fused_supported(1, kFamilyFusedMaxN, 1, K) && !small_family_fused_supported(1, kFamilyFusedMaxN + 1, 1, K));
  }
  CHECK(!small_family_fused_supported(1, 8, 1, 0) && !small_family_fused_supported(1, 8, 1, kMaxK + 1) &&
        !small_family_fused_supported(1, 0, 1, 2) && !small_family_fused_supported(3, 8, 1, 2) &&
        !small_family_fused_supported(-1, 8, 1, 2));
  // the largest carve of the walk by hand, in doubles: the search instance at n = 32 (NB = 2, NP = 32), d = 1, K = 4:
  // exp table | xs[n] | us[K][NP] th[K] w2[K] colbuf[2][NP + 16] dvec[NP] zb[2][NP] slack[8] | chain words | search state
  const size_t by_hand = (size_t)(CCGP_SMALL_EXP_TABLE ? 256 : 0) + 32 + 4 * 32 + 4 + 4 + 2 * (32 + 16) + 32 + 2 * 32 + 8 +
                         (2 * 256 + 4 + 4 + 4 + 2) + (4 * 4 + 5 * 4 + 18);
  g_n = 32; g_K = 4;
  CHECK(reg_nm_lds_doubles(2, 32, 1, 4) == by_hand && 8 * by_hand <= (size_t)160 * 1024 - 64);
  std::printf("cells %ld supported %ld gauss %ld kept %ld lds %zu\n", cells, supported, gauss_reg, family_kept, 8 * by_hand);
  std::printf("ok\n");
  return 0;
}
