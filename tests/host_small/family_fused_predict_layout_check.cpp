// CPU check of the domain and routes of the 1-D families' prediction and leave-one-out on the register-resident evaluator
// (csrc/small_layout.h: small_family_fused_predict_supported, small_family_fused_loo_supported; CCGP_OPT_FAMILY_FUSED_PREDICT).
// Walks n 1..40, d 1..3, K 1..4 and the three kernel families (0 Gaussian, 1 Matern, 2 Matern + spline):
//   - small_family_fused_predict_supported is true exactly for family 1 at K <= 3 or family 2 at K = 2, d = 1, 1 <= n <= 32;
//   - small_family_fused_loo_supported is true exactly for family 1 (any K of the walk) or family 2 at K = 2, d = 1, 2 <= n <= 32;
//   - with the flags capi.hip passes, `gauss || supported`, small_route(Op::Predict) and small_route_loo say Reg there;
//   - with the plain `gauss` flag they say what they say without the option: Blocked for a 1-D family at every shape, and for
//     the Gaussian family what the expressions behind them give;
//   - outside the domains (n = 33, d > 1, K = 4 for prediction, family 2 with K != 2) the flags change nothing;
//   - the carves of the instances the routes launch fit: the factor-keeping likelihood instance on both grids (8 x 8 with four
//     matrices per workgroup, 16 x 16 wide form), the leave-one-out instance (16 x 16, n identity rows), and SiteSolveCarve with
//     two workgroups per CU; the largest of each is summed by hand below.
// Built and run by tests/test_family_fused_predict_layout.py (also once with -fsanitize=address,undefined).  Prints the counts,
// then "ok".
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
  long cells = 0, predict = 0, loo = 0, predict_kept = 0, loo_kept = 0;
  for (int fam = 0; fam < 3; ++fam)
    for (int n = 1; n <= 40; ++n)
      for (int d = 1; d <= 3; ++d)
        for (int K = 1; K <= 4; ++K) {
          g_fam = fam; g_n = n; g_d = d; g_K = K;
          ++cells;
          const bool dom = (fam == 1 || (fam == 2 && K == 2)) && d == 1 && n >= 1 && n <= 32;
          const bool want_p = dom && K <= 3, want_l = dom && n >= 2;
          const bool got_p = small_family_fused_predict_supported(fam, n, d, K);
          const bool got_l = small_family_fused_loo_supported(fam, n, d, K);
          CHECK(got_p == want_p);
          CHECK(got_l == want_l);
          CHECK(!got_p || small_family_fused_supported(fam, n, d, K));
          CHECK(!got_l || small_family_fused_supported(fam, n, d, K));
          const bool gauss = fam == 0;
          // option off: the plain flag
          const Route p0 = small_route(Op::Predict, gauss, n, d, K), l0 = small_route_loo(gauss, n, d, K);
          if (gauss) {
            const bool reg_p = small_lds_tier(n, d) && small_reg_supported(n, d, K, false, true);
            CHECK(p0 == (reg_p ? Route::Reg : Route::Blocked));
            CHECK(l0 == (small_reg_inverse_supported(n, d, K) ? Route::Reg : Route::Blocked));
          } else {
            CHECK(p0 == Route::Blocked && l0 == Route::Blocked);
          }
          // option on: what capi.hip passes (prediction: with CCGP_OPT_PREDICT_FACTOR at its default)
          const Route p1 = small_route(Op::Predict, gauss || got_p, n, d, K), l1 = small_route_loo(gauss || got_l, n, d, K);
          if (got_p) {
            CHECK(p1 == Route::Reg);
            ++predict;
            // what predict_run launches: the kept-factor scheme and nothing else
            CHECK(small_reg_sites_supported(n, d, K));
            const int nb8 = (n + 7) / 8, nb16 = (n + 15) / 16;
            CHECK(nb8 >= 1 && nb8 <= 4 && nb16 >= 1 && nb16 <= 2);                          // the FAM + FAC instances compiled
            CHECK(lds_fits(reg_lds_doubles(8, nb8, 1, false, false, n, d, K)));             // 8 x 8: four matrices per workgroup
            CHECK(lds_fits(reg_lds_doubles(16, nb16, 1, false, false, n, d, K)));           // 16 x 16: the wide form
            CHECK(lds_fits(SiteSolveCarve(n).total, 2));
            CHECK(small_reg_sites_scratch(n, d, K, 1) == sizeof(double) * ((size_t)FacLayout(n).total + (size_t)fac_npf(n) * 64));
            CHECK(fac_npf(n) >= n && fac_npf(n) % 8 == 0 && fac_npf(n) <= 32);
          } else {
            CHECK(p1 == p0);
            if (!gauss) ++predict_kept;
          }
          if (got_l) {
            CHECK(l1 == Route::Reg);
            ++loo;
            const int nb16 = (n + 15) / 16;
            CHECK(nb16 >= 1 && nb16 <= 2);                                                   // the FAM + INV = 4 instances compiled
            CHECK(lds_fits(reg_lds_doubles(16, nb16, nb16 + 1, true, false, n, d, K)));
          } else {
            CHECK(l1 == l0);
            if (!gauss) ++loo_kept;
          }
          // the routes option 11 takes are not these: a 1-D family's likelihood under the plain flag stays where it was
          if (!gauss) CHECK(small_route(Op::Loglik, gauss, n, d, K) == Route::Blocked);
        }
  // the edges by name
  g_fam = 1; g_d = 1; g_K = 2; g_n = 33;
  CHECK(!small_family_fused_predict_supported(1, 33, 1, 2) && !small_family_fused_loo_supported(1, 33, 1, 2));
  CHECK(small_family_fused_predict_supported(1, 32, 1, 3) && !small_family_fused_predict_supported(1, 32, 1, 4));
  CHECK(small_family_fused_loo_supported(1, 32, 1, 4) && small_family_fused_loo_supported(1, 32, 1, kMaxK));
  CHECK(!small_family_fused_predict_supported(1, 8, 2, 2) && !small_family_fused_loo_supported(1, 8, 2, 2));
  CHECK(!small_family_fused_predict_supported(2, 8, 1, 1) && !small_family_fused_predict_supported(2, 8, 1, 3));
  CHECK(!small_family_fused_loo_supported(2, 8, 1, 1) && !small_family_fused_loo_supported(2, 8, 1, 3));
  CHECK(small_family_fused_predict_supported(1, 1, 1, 1) && !small_family_fused_loo_supported(1, 1, 1, 1));
  CHECK(!small_family_fused_predict_supported(0, 8, 1, 2) && !small_family_fused_loo_supported(0, 8, 1, 2));
  // the largest carves by hand, in doubles, at n = 32, d = 1, K = 3 (prediction) and K = 4 (leave-one-out); `tab` is the exp
  // table.  One matrix: us[K][NP] th[K] w2[K] colbuf[2][NP + G NE] dvec[NP] zb[2][NP] slack[8] (+ the inverse's tail)
  const size_t tab = CCGP_SMALL_EXP_TABLE ? 256 : 0;
  g_n = 32; g_K = 3;
  const size_t mat8 = 3 * 32 + 3 + 3 + 2 * (32 + 8) + 32 + 2 * 32 + 8;                 // G = 8, NB = 4
  const size_t fac8 = tab + 32 + 4 * mat8;
  CHECK(reg_lds_doubles(8, 4, 1, false, false, 32, 1, 3) == fac8);
  const size_t fac16 = tab + 32 + (3 * 32 + 3 + 3 + 2 * (32 + 16) + 32 + 2 * 32 + 8);   // G = 16, NB = 2
  CHECK(reg_lds_doubles(16, 2, 1, false, false, 32, 1, 3) == fac16);
  // the factor block: hdr[8] rd[32] zy[32] z1[32] L'[32 31 / 2]; the solve's carve: head | L' in row blocks | slack[8]
  CHECK(FacLayout(32).head == 8 + 3 * 32 && FacLayout(32).total == 8 + 3 * 32 + 496);
  const size_t solve = (8 + 3 * 32) + 32 * 4 * 4 + 8;
  CHECK(SiteSolveCarve(32).total == solve);
  g_K = 4;
  const size_t head = 4 * 32 + 4 + 4 + 2 * (32 + 48) + 32 + 2 * 32 + 8;                // G = 16, NB = 2, NE = 3
  const size_t bump = (tab + 32 + head) & 1;
  const size_t loo16 = tab + 32 + head + 32 * 34 + 1 + 4 * kGradSlots;
  CHECK(bump <= 1 && reg_lds_doubles(16, 2, 3, true, false, 32, 1, 4) == loo16);
  CHECK(8 * loo16 <= (size_t)160 * 1024 - 64 && 8 * fac8 <= (size_t)160 * 1024 - 64 && 8 * solve <= (size_t)80 * 1024 - 64);
  std::printf("cells %ld predict %ld loo %ld predict_kept %ld loo_kept %ld fac8 %zu fac16 %zu solve %zu loo16 %zu\n", cells, predict,
              loo, predict_kept, loo_kept, 8 * fac8, 8 * fac16, 8 * solve, 8 * loo16);
  std::printf("ok\n");
  return 0;
}
