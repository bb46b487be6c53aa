// CPU check of the design search's route and carve (csrc/small_layout.h: small_route_design_fit, reg_design_fit_lds_doubles).
// Walks n 1..129, every d, K, kernel family and n_fixed from -1 to n: the route is Reg exactly where the family is Gaussian,
// n <= 128, n_fixed lies in [0, n), the start has 1 .. 64 variables nv = (n - n_fixed) d, and the words fit -- the INV = 3
// per-design carve and the start's words behind it, both summed here by hand -- and Unsupported everywhere else; wherever it is
// Reg the design gradient itself has its route.  The dynamic LDS the launcher asks for is that hand sum.  Built and run by
// tests/test_design_fit_layout.py (also once with -fsanitize=address,undefined).  Prints the counts and the pinned totals,
// then "ok".
#include <cstdio>
#include <cstdlib>

#include "small_layout.h"

using namespace ccgp;

#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      std::printf("FAILED %s (line %d): n %d d %d K %d n_fixed %d\n", #cond, __LINE__, g_n, g_d, g_K, g_nf); \
      std::exit(1);                                                                                          \
    }                                                                                                        \
  } while (0)
static int g_n, g_d, g_K, g_nf;

static bool fits(size_t doubles) { return 8 * doubles <= (size_t)160 * 1024 - 64; }
// the design-gradient instance's LDS in doubles, summed by hand: exp table | the shared design slot | ONE matrix of
// us[K][NP] th[K][d] w2[K] colbuf[2][NP + 16 (NB + 1)] dvec[NP] zb[2][NP] slack[8] | bump | zmat[NP][NP + 2] | part[4][28] |
// the design's own copy
static size_t design_grad_by_hand(int n, int d, int K) {
  const int NB = (n + 15) / 16, NP = 16 * NB, XR = 16 * (NB + 1);
  return (size_t)(CCGP_SMALL_EXP_TABLE ? 256 : 0) + (size_t)d * n + (size_t)K * NP + (size_t)K * d + K + 2 * (size_t)(NP + XR) + NP +
         2 * (size_t)NP + 8 + 1 + (size_t)NP * (NP + 2) + 4 * 28 + (size_t)d * n;
}
// the start's words behind it: go | ld | grad[nv] | state[16 + 16 nv]
static size_t design_fit_by_hand(int n, int d, int K, int nv) { return design_grad_by_hand(n, d, K) + 2 + nv + 16 + 16 * (size_t)nv; }

int main() {
  long reg = 0, unsupported = 0, refused_for_words = 0;
  for (int n = 1; n <= 129; ++n)
    for (int d = 1; d <= kMaxD; ++d)
      for (int K = 1; K <= kMaxK; ++K)
        for (int fam = 0; fam < 3; ++fam)
          for (int nf = -1; nf <= n; ++nf) {
            g_n = n; g_d = d; g_K = K; g_nf = nf;
            const long long nv = (long long)(n - nf) * d;
            const bool grad_route = n <= 128 && fits(design_grad_by_hand(n, d, K));
            CHECK((small_route(Op::DesignGrad, true, n, d, K) == Route::Reg) == grad_route);
            const bool want = fam == 0 && nf >= 0 && nf < n && grad_route && nv >= 1 && nv <= 64 &&
                              fits(design_fit_by_hand(n, d, K, (int)nv));
            const Route got = small_route_design_fit(fam == 0, n, d, K, nf);
            CHECK(got == (want ? Route::Reg : Route::Unsupported));
            if (want) {
              CHECK(reg_design_fit_lds_doubles((n + 15) / 16, n, d, K, (int)nv) == design_fit_by_hand(n, d, K, (int)nv));
              ++reg;
            } else {
              ++unsupported;
              // shapes the evaluator serves and the stepper takes, refused for the start's words alone
              if (fam == 0 && nf >= 0 && nf < n && grad_route && nv >= 1 && nv <= 64) ++refused_for_words;
            }
          }
  std::printf("reg %ld unsupported %ld words %ld\n", reg, unsupported, refused_for_words);
  // the eight instances at the shapes of tests/test_gpu_device_design.py (n, d, n_fixed, NB), K = 2: dynamic LDS in bytes
  const int shapes[9][4] = {{14, 2, 0, 1}, {21, 2, 14, 2}, {17, 9, 10, 2}, {33, 3, 16, 3}, {50, 9, 43, 4}, {65, 1, 1, 5}, {81, 2, 60, 6},
                            {97, 5, 90, 7}, {128, 4, 112, 8}};
  std::printf("lds");
  for (int s = 0; s < 9; ++s) {
    const int n = shapes[s][0], d = shapes[s][1], nf = shapes[s][2], NB = (n + 15) / 16;
    g_n = n; g_d = d; g_K = 2; g_nf = nf;
    CHECK(NB == shapes[s][3] && small_route_design_fit(true, n, d, 2, nf) == Route::Reg);
    std::printf(" %zu", 8 * reg_design_fit_lds_doubles(NB, n, d, 2, (n - nf) * d));
  }
  std::printf("\nok\n");
  return 0;
}
