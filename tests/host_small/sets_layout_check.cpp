// CPU check of the sets form's route and staging (csrc/small_layout.h: small_route_sets, small_reg_sets_grid; csrc/call_stage.h:
// sets_stage).  Walks n 1..129, every d, K and kernel family: the route is Reg exactly where the family is Gaussian and the
// sets instance's carves -- summed here by hand -- fit; the grid the chooser picks for a call of B rows has an instance (block
// count) and a carve that fits, and the per-matrix design copies of the 8 x 8 grid lie behind everything else, disjoint,
// and end at `total`.  Then sets_stage: its pieces lie inside the buffer, 256-byte aligned, in order and without overlap,
// the planning pass measures what the real pass uses, and inputs() / results() name each piece with its size.
// Built and run by tests/test_sets_layout.py (also once with -fsanitize=address,undefined).  Prints the counts, then "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "call_stage.h"
#include "small_layout.h"

using namespace ccgp;

#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      std::printf("FAILED %s (line %d): n %d d %d K %d\n", #cond, __LINE__, g_n, g_d, g_K); \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)
static int g_n, g_d, g_K;

// the plain likelihood instance's LDS in doubles, summed by hand: exp table | shared design | MPW matrices of
// us[K][NP] th[K][d] w2[K] colbuf[2][NP + G] dvec[NP] zb[2][NP] slack[8] | one design per matrix (8 x 8 grid of the sets form)
static size_t by_hand(int G, int n, int d, int K, bool own_design) {
  const int NB = (n + G - 1) / G, NP = G * NB, MPW = 256 / (G * G);
  const size_t per_mat = (size_t)K * NP + (size_t)K * d + K + 2 * (size_t)(NP + G) + NP + 2 * (size_t)NP + 8;
  return (size_t)(CCGP_SMALL_EXP_TABLE ? 256 : 0) + (size_t)d * n + MPW * per_mat + (own_design ? (size_t)MPW * d * n : 0);
}
static bool fits(size_t doubles) { return 8 * doubles <= (size_t)160 * 1024 - 64; }

static void check_stage(int n, int d, int K, int C, int B) {
  g_n = n; g_d = d; g_K = K;
  const int P = K + K * d;
  const size_t bytes = layout_bytes([&](Layout& c) { sets_stage(c, n, d, P, C, B); });
  Layout plan;
  const SetsStage p = sets_stage(plan, n, d, P, C, B);
  CHECK(!p.Xs && !p.ys && !p.sigma2 && !p.params && !p.set && !p.loglik && !p.beta && !p.status && plan.off == bytes);
  char* base = static_cast<char*>(std::aligned_alloc(256, bytes + 256));
  Layout real(base);
  const SetsStage s = sets_stage(real, n, d, P, C, B);
  CHECK(real.off == bytes);
  struct R { char* p; size_t b; };
  const std::vector<R> r = {{(char*)s.Xs, 8 * (size_t)C * n * d}, {(char*)s.ys, 8 * (size_t)C * n}, {(char*)s.sigma2, 8 * (size_t)C},
                            {(char*)s.params, 8 * (size_t)B * P}, {(char*)s.set, 4 * (size_t)B}, {(char*)s.loglik, 8 * (size_t)B},
                            {(char*)s.beta, 8 * (size_t)B}, {(char*)s.status, 4 * (size_t)B}};
  char* end = base;
  for (const R& x : r) {
    CHECK(x.p >= end && (x.p - base) % 256 == 0 && x.p + x.b <= base + bytes);   // declared in address order: no overlap
    end = x.p + x.b;
  }
  CHECK(end + 255 >= base + bytes);                                              // nothing but alignment behind the last piece
  for (const R& x : r) std::fill(x.p, x.p + x.b, (char)0x5a);                   // every byte of every piece is writable
  std::vector<double> hX(1), hy(1), hs(1), hp(1), hl(1), hb(1);
  std::vector<int> hset(1);
  const std::vector<Piece> in = s.inputs(hX.data(), hy.data(), hs.data(), hp.data(), hset.data());
  CHECK(in.size() == 5);
  for (int i = 0; i < 5; ++i) CHECK(in[i].dev == r[i].p && in[i].bytes == r[i].b);
  const std::vector<Piece> out = s.results(hl.data(), hb.data());
  CHECK(out.size() == 2 && out[0].dev == r[5].p && out[0].bytes == r[5].b && out[1].dev == r[6].p && out[1].bytes == r[6].b);
  // pull_status reads the status words behind beta
  CHECK((char*)s.status >= (char*)s.beta + 8 * (size_t)B);
  const Span up = span_of(in);
  CHECK(up.lo == (char*)s.Xs && up.lo + up.bytes == (char*)s.set + 4 * (size_t)B);
  std::free(base);
}

int main() {
  long reg = 0, blocked = 0, grid8 = 0, grid16 = 0;
  for (int n = 1; n <= 129; ++n)
    for (int d = 1; d <= kMaxD; ++d)
      for (int K = 1; K <= kMaxK; ++K) {
        g_n = n; g_d = d; g_K = K;
        const bool want = n <= 128 && fits(by_hand(16, n, d, K, false)) && (n > 64 || fits(by_hand(8, n, d, K, true)));
        for (int family = 0; family < 3; ++family) {
          const Route r = small_route_sets(family == 0, n, d, K);
          CHECK(r == (family == 0 && want ? Route::Reg : Route::Blocked));
          (r == Route::Reg ? reg : blocked)++;
        }
        if (n <= 128) {
          // the header's totals are the hand sums
          CHECK(reg_lds_doubles(16, (n + 15) / 16, 1, false, false, n, d, K) == by_hand(16, n, d, K, false));
          if (n <= 104) CHECK(reg_lds_doubles(8, (n + 7) / 8, 1, false, true, n, d, K) == by_hand(8, n, d, K, true));
        }
        if (!want) continue;
        for (int B : {1, 63, 64, 65, 4096}) {
          const int G = small_reg_sets_grid(n, d, K, B);
          CHECK(G == 8 || G == 16);
          CHECK(B > 64 || G == 16);                                  // the latency case: four waves per matrix
          CHECK(B <= 64 || n > 64 || G == 8);                        // a large call at n <= 64: one wave per matrix
          const int NB = (n + G - 1) / G;
          CHECK(G == 8 ? NB <= 13 : NB <= 8);                        // dispatch_sets has the instance
          const RegCarve cv(G, NB, 1, false, G == 8, n, d, K);
          CHECK(fits(cv.total) && cv.total == by_hand(G, n, d, K, G == 8));
          if (G == 8) {
            // four designs behind the four matrices' blocks, the last one ending at total
            CHECK(cv.xs_own == cv.mat0 + 4 * cv.per_mat && (size_t)cv.xs_own + 4 * (size_t)d * n == cv.total);
          } else {
            // one matrix per workgroup: the set's design lies in the shared slot, right in front of the matrix's block
            CHECK(cv.xs + d * n == cv.mat0 && (size_t)cv.mat0 + cv.per_mat == cv.total);
          }
          (G == 8 ? grid8 : grid16)++;
        }
      }
  for (int n : {1, 5, 50, 64, 128})
    for (int d : {1, 9, kMaxD})
      for (int K : {1, 2, kMaxK})
        for (int C : {1, 9, 100})
          for (int B : {1, 7, 63, 4097}) check_stage(n, d, K, C, B);
  std::printf("reg %ld blocked %ld grid8 %ld grid16 %ld\n", reg, blocked, grid8, grid16);
  std::printf("ok\n");
  return 0;
}
