// CPU check of the domain and routes of the 1-D families' profiled mode and analytic gradient on the register-resident
// evaluator (csrc/small_layout.h: small_family_fused_profile_supported, small_family_fused_grad_supported;
// CCGP_OPT_FAMILY_FUSED_GRAD).  Walks n 1..40, d 1..3, K 1..4 and the three kernel families (0 Gaussian, 1 Matern,
// 2 Matern + spline):
//   - both predicates are true exactly for family 1 or family 2 at K = 2, d = 1, 1 <= n <= 32, and never outside
//     small_family_fused_supported;
//   - with the flags capi.hip passes, `gauss || supported`, small_route(Op::Loglik) (the value-only profiled call),
//     small_route(Op::Grad) (ccgp_loglik_grad_batch, ccgp_profile_batch with a gradient) and small_route_profile_grad_sets say Reg
//     there, and the carves of the instances they launch fit: the profiled likelihood instance on both grids (NB <= 4 on the
//     8 x 8, NB <= 2 on the 16 x 16) and the gradient instance (16 x 16, n identity rows);
//   - with the plain `gauss` flag nothing moves: Op::Loglik and small_route_profile_grad_sets say Blocked for a 1-D family at
//     every shape (Op::Grad does not look at the flag: capi.hip refuses the gradient before it asks), and for the Gaussian
//     family every route is what the expressions behind it give;
//   - outside the domain (n = 33, d > 1, family 2 with K != 2) the flags change nothing.
// Built and run by tests/test_family_fused_grad_layout.py (also once with -fsanitize=address,undefined).  Prints the counts,
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
  long cells = 0, profile = 0, grad = 0, kept = 0;
  for (int fam = 0; fam < 3; ++fam)
    for (int n = 1; n <= 40; ++n)
      for (int d = 1; d <= 3; ++d)
        for (int K = 1; K <= 4; ++K) {
          g_fam = fam; g_n = n; g_d = d; g_K = K;
          ++cells;
          const bool dom = (fam == 1 || (fam == 2 && K == 2)) && d == 1 && n >= 1 && n <= 32;
          const bool got_p = small_family_fused_profile_supported(fam, n, d, K);
          const bool got_g = small_family_fused_grad_supported(fam, n, d, K);
          CHECK(got_p == dom);
          CHECK(got_g == dom);
          CHECK(got_p == small_family_fused_supported(fam, n, d, K));
          CHECK(!got_g || (small_family_fused_supported(fam, n, d, K) && small_reg_inverse_supported(n, 1, K)));
          const bool gauss = fam == 0;
          // option off: the plain flag
          const Route v0 = small_route(Op::Loglik, gauss, n, d, K), g0 = small_route(Op::Grad, gauss, n, d, K);
          const Route s0 = small_route_profile_grad_sets(gauss, n, d, K);
          const Route grad_expr = !small_lds_tier(n, d) ? Route::Blocked : small_reg_inverse_supported(n, d, K) ? Route::Reg : Route::Lds;
          CHECK(g0 == grad_expr);   // (whatever the flag)
          if (gauss) {
            CHECK(v0 == (small_reg_supported(n, d, K) ? Route::Reg : Route::Blocked));
            CHECK(s0 == (grad_expr == Route::Reg ? Route::Reg : Route::Blocked));
          } else {
            CHECK(v0 == Route::Blocked && s0 == Route::Blocked);
          }
          // option on: what capi.hip passes
          const Route v1 = small_route(Op::Loglik, gauss || got_p, n, d, K), g1 = small_route(Op::Grad, gauss || got_g, n, d, K);
          const Route s1 = small_route_profile_grad_sets(gauss || got_g, n, d, K);
          CHECK(g1 == g0);
          if (got_p) {
            CHECK(v1 == Route::Reg);
            ++profile;
            const int nb8 = (n + 7) / 8, nb16 = (n + 15) / 16;
            CHECK(nb8 >= 1 && nb8 <= 4 && nb16 >= 1 && nb16 <= 2);                          // the FAM + PROF instances compiled
            CHECK(lds_fits(reg_lds_doubles(8, nb8, 1, false, false, n, d, K)));
            CHECK(lds_fits(reg_lds_doubles(16, nb16, 1, false, false, n, d, K)));
          } else {
            CHECK(v1 == v0);
          }
          if (got_g) {
            CHECK(g1 == Route::Reg && s1 == Route::Reg);
            ++grad;
            const int nb16 = (n + 15) / 16;
            CHECK(nb16 >= 1 && nb16 <= 2);                                                   // the FAM + INV = 2 instances compiled
            CHECK(lds_fits(reg_lds_doubles(16, nb16, nb16 + 1, true, false, n, d, K)));
          } else {
            CHECK(s1 == s0);
            if (!gauss) ++kept;
          }
          // what options 11 and 12 move is not this: the predicates do not depend on them, and a family's other routes under the
          // plain flag stay where they were
          if (!gauss) CHECK(small_route_sets(gauss, n, d, K) == Route::Blocked && small_route_loo(gauss, n, d, K) == Route::Blocked);
        }
  // the edges by name
  g_fam = 1; g_d = 1; g_K = 2; g_n = 33;
  CHECK(!small_family_fused_grad_supported(1, 33, 1, 2) && !small_family_fused_profile_supported(1, 33, 1, 2));
  CHECK(small_family_fused_grad_supported(1, 32, 1, 2) && small_family_fused_grad_supported(1, 32, 1, kMaxK));
  CHECK(small_family_fused_grad_supported(1, 1, 1, 1) && small_family_fused_profile_supported(1, 1, 1, 1));
  CHECK(!small_family_fused_grad_supported(1, 8, 2, 2) && !small_family_fused_profile_supported(1, 8, 2, 2));
  CHECK(!small_family_fused_grad_supported(2, 8, 1, 1) && !small_family_fused_grad_supported(2, 8, 1, 3));
  CHECK(small_family_fused_grad_supported(2, 8, 1, 2) && small_family_fused_profile_supported(2, 32, 1, 2));
  CHECK(!small_family_fused_grad_supported(0, 8, 1, 2) && !small_family_fused_profile_supported(0, 8, 1, 2));
  // the largest gradient carve by hand, in doubles, at n = 32, d = 1, K = 4: G = 16, NB = 2, NE = 3 -- the carve of the
  // leave-one-out instance (tests/host_small/family_fused_predict_layout_check.cpp)
  const size_t tab = CCGP_SMALL_EXP_TABLE ? 256 : 0;
  g_n = 32; g_K = 4;
  const size_t head = 4 * 32 + 4 + 4 + 2 * (32 + 48) + 32 + 2 * 32 + 8;
  const size_t grad16 = tab + 32 + head + 32 * 34 + 1 + 4 * kGradSlots;
  CHECK(reg_lds_doubles(16, 2, 3, true, false, 32, 1, 4) == grad16);
  CHECK(8 * grad16 <= (size_t)160 * 1024 - 64);
  std::printf("cells %ld profile %ld grad %ld kept %ld grad16 %zu\n", cells, profile, grad, kept, 8 * grad16);
  std::printf("ok\n");
  return 0;
}
