// CPU check of csrc/small_layout.h over every shape the entry points accept (n 1..128, d 1..kMaxD, K 1..kMaxK) and every
// (G, NB, NE, inv, per-design) instance the dispatchers of small_reg.hip can form.  The `old` namespace holds the hand-summed
// formulas the header replaced, written out as they stood before it, so that sizes and routes are pinned to those values.
// small_route is held, over n 1..129, both families and all six ops, to the route expressions the entry points of capi.hip
// carried before it (old::route).  Prints counts and, with "table" as argument, one line per (n, d) -- the gradient's route
// letters from small_route itself -- for tests/test_small_layout.py to compare the Python mirrors of
// tests/test_gpu_gradient_exact.py against; with "witness", one shape per reachable (op, route) cell (tests/route_witnesses.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "small_layout.h"

using namespace ccgp;

namespace old {
constexpr int kTab = CCGP_SMALL_EXP_TABLE ? 256 : 0;
constexpr size_t kLds = 160 * 1024;
int kPerMat(int NP, int G, int NE, int K, int d, bool inv = false) {
  return K * NP + K * d + K + 2 * (NP + G * NE) + NP + 2 * NP + 8 +
         (inv ? NP * (NP + 2) + 1 + 4 * 28 : (NE > 1 ? K * G * NE + 3 * G * G * NE : 0));
}
size_t reg_lds_bytes(int G, int NB, int NE, int n, int d, int K, bool per_design) {
  const int MPW = 256 / (G * G);
  return sizeof(double) * (kTab + (size_t)d * n + (size_t)MPW * kPerMat(G * NB, G, NE, K, d) +
                           (per_design ? (size_t)MPW * d * n : 0) + (NE > 1 ? (size_t)d * G * NE : 0));
}
bool small_reg_supported(int n, int d, int K, bool per_design = false, bool predict = false) {
  if (n > 128) return false;
  const int G = n <= 64 ? 8 : 16;
  const int NB = (n + G - 1) / G;
  const int MPW = 256 / (G * G);
  const int NE = predict ? 4 : 1;
  return sizeof(double) * (kTab + (size_t)d * n + (size_t)MPW * kPerMat(G * NB, G, NE, K, d) +
                           (per_design ? (size_t)MPW * d * n : 0) + (predict ? (size_t)d * G * NE : 0)) <= kLds - 64;
}
bool fits8(int n, int d, int K, bool per_design) {
  const int nb8 = (n + 7) / 8;
  return sizeof(double) * (kTab + (size_t)d * n + (size_t)4 * kPerMat(8 * nb8, 8, 1, K, d) +
                           (per_design ? (size_t)4 * d * n : 0)) <= kLds - 64;
}
int npf_of(int n) { return (n + 7) / 8 * 8; }
size_t site_corr_lds_bytes(int n, int d, int K, int waves) {
  const int npf = npf_of(n);
  return sizeof(double) * ((size_t)(K * d + 7) / 8 * 8 + 8 + (size_t)K * npf + (size_t)K * d * npf + (size_t)waves * d * 64);
}
size_t site_solve_lds_doubles(int n) {
  const int npf = npf_of(n);
  return (size_t)(8 + 3 * npf) + 32 * (npf / 8) * (npf / 8) + 8;
}
bool small_reg_sites_supported(int n, int d, int K) {
  if (n > 104 || K > 3) return false;
  const int nb8 = (n + 7) / 8;
  return sizeof(double) * (kTab + (size_t)d * n + (size_t)4 * kPerMat(8 * nb8, 8, 1, K, d)) <= kLds - 64 &&
         sizeof(double) * site_solve_lds_doubles(n) <= kLds / 2 - 64 && site_corr_lds_bytes(n, d, K, 4) <= kLds / 2 - 64;
}
size_t inv_lds_bytes(int NB, int n, int d, int K, bool per_design) {
  return sizeof(double) * (kTab + (size_t)d * n + (size_t)kPerMat(16 * NB, 16, NB + 1, K, d, true)) +
         (per_design ? sizeof(double) * (size_t)d * n : 0);
}
bool small_reg_inverse_supported(int n, int d, int K) {
  if (n > 128) return false;
  const int NB = (n + 15) / 16;
  return sizeof(double) * (kTab + (size_t)d * n + (size_t)kPerMat(16 * NB, 16, NB + 1, K, d, true)) <= kLds - 64;
}
bool small_reg_design_grad_supported(int n, int d, int K) {
  if (n > 128) return false;
  const int NB = (n + 15) / 16;
  return sizeof(double) * (kTab + (size_t)2 * d * n + (size_t)kPerMat(16 * NB, 16, NB + 1, K, d, true)) <= kLds - 64;
}
size_t small_lds_bytes(int n, int d, int mtile) {
  size_t dbl = (size_t)(n + 2 + mtile) * n + (size_t)d * n + (size_t)8 * n + (size_t)d * mtile + (size_t)8 * mtile +
               (size_t)8 * d + 8 + 16 + 256;
  return dbl * sizeof(double);
}
int small_pick_mtile(int n, int d, int m) {
  const size_t budget = 150 * 1024;
  int mt = m < 1 ? 1 : m;
  if (mt > 256) mt = 256;
  while (mt > 1 && small_lds_bytes(n, d, mt) > budget) --mt;
  return mt;
}
// The route decisions as the entry points of capi.hip wrote them out, each in its own words, before small_route: over the
// header's predicates (which the loop in main holds to the formulas above).
using ccgp::kLdsBytes;
using ccgp::kSmallMaxN;
bool loglik_reg(bool gauss, int n, int d, int K) { return gauss && ccgp::small_reg_supported(n, d, K); }   // loglik_run
bool reserve_sweep(bool gauss, int n) { return n > kSmallMaxN || !gauss; }                                  // ccgp_reserve
bool grad_blocked(int n, int d) { return n > kSmallMaxN || ccgp::small_lds_bytes(n, d, 1) > (size_t)kLdsBytes - 64; }
bool grad_reg(int n, int d, int K) { return ccgp::small_reg_inverse_supported(n, d, K); }                   // ccgp_loglik_grad_batch
bool logpost_reg_val(bool gauss, int n, int d, int K) { return gauss && ccgp::small_reg_supported(n, d, K); }
bool logpost_reg_inv(bool gauss, int n, int d, int K) { return gauss && ccgp::small_reg_inverse_supported(n, d, K); }
bool logpost_blocked(bool gauss, int n, int d) {
  return !gauss || n > kSmallMaxN || ccgp::small_lds_bytes(n, d, 1) > (size_t)kLdsBytes - 64;
}
bool designs_blocked(int n, int d, int K) { return !ccgp::small_reg_supported(n, d, K, true); }          // ccgp_mixed_logdet_designs
bool design_grad_ok(int n, int d, int K) { return ccgp::small_reg_design_grad_supported(n, d, K); }
bool predict_blocked(bool gauss, int n, int d, int K) {                                                   // predict_run
  return !gauss || n > kSmallMaxN || ccgp::small_lds_bytes(n, d, 1) > (size_t)kLdsBytes - 64 ||
         !ccgp::small_reg_supported(n, d, K, false, true);
}
bool fused(bool gauss, int n, int d) {                                                                    // ccgp_factor_batch
  return gauss && n <= kSmallMaxN && ccgp::small_lds_bytes(n, d, 1) <= (size_t)kLdsBytes - 64;
}
Route route(Op op, bool gauss, int n, int d, int K) {
  switch (op) {
    case Op::Loglik: return loglik_reg(gauss, n, d, K) ? Route::Reg : Route::Blocked;
    case Op::Predict: return predict_blocked(gauss, n, d, K) ? Route::Blocked : Route::Reg;
    case Op::Inverse: return logpost_reg_inv(gauss, n, d, K) ? Route::Reg : logpost_blocked(gauss, n, d) ? Route::Blocked : Route::Lds;
    case Op::Grad: return grad_blocked(n, d) ? Route::Blocked : grad_reg(n, d, K) ? Route::Reg : Route::Lds;
    case Op::LogdetDesigns: return designs_blocked(n, d, K) ? Route::Blocked : Route::Reg;
    case Op::DesignGrad: return design_grad_ok(n, d, K) ? Route::Reg : Route::Unsupported;
  }
  return Route::Unsupported;
}
}  // namespace old

static long failures = 0;
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (failures++ < 20) { std::fprintf(stderr, "FAIL %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fputc('\n', stderr); } \
    }                                                       \
  } while (0)

// regions {start, size} in the order of the carve: each starts at or after the previous one's end; the last ends inside total
struct Region { long start, size; };
static void check_order(const Region* r, int count, long total, const char* what, int n, int d, int K) {
  long end = 0;
  for (int i = 0; i < count; ++i) {
    CHECK(r[i].start >= end, "%s region %d at n=%d d=%d K=%d", what, i, n, d, K);
    end = r[i].start + r[i].size;
  }
  CHECK(end <= total, "%s ends at %ld > total %ld, n=%d d=%d K=%d", what, end, total, n, d, K);
}

static void check_reg(int G, int NB, int NE, bool inv, bool per_design, int n, int d, int K) {
  const int NP = G * NB, XR = G * NE, MPW = 256 / (G * G);
  const size_t want = inv ? old::inv_lds_bytes(NB, n, d, K, per_design) : old::reg_lds_bytes(G, NB, NE, n, d, K, per_design);
  const size_t total = reg_lds_doubles(G, NB, NE, inv, per_design, n, d, K);
  CHECK(sizeof(double) * total == want, "RegCarve total G=%d NB=%d NE=%d inv=%d pd=%d n=%d d=%d K=%d", G, NB, NE, inv, per_design, n, d, K);
  CHECK(!inv || MPW == 1, "the inverse instances run one matrix per workgroup");
  // the shared pieces in order, every matrix's block among them, and each matrix's own design
  Region r[5 + 4 * 9];
  int count = 0;
  long blocks_end = 0;
  const RegCarve c(G, NB, NE, inv, per_design, n, d, K);
  CHECK(c.total == total && c.per_mat == old::kPerMat(NP, G, NE, K, d, inv), "per_mat n=%d d=%d K=%d", n, d, K);
  r[count++] = {c.etab, (long)kSmallExpTable};
  r[count++] = {c.xs, (long)d * n};
  for (int sub = 0; sub < MPW; ++sub) {
    const long block = c.mat0 + (long)sub * c.per_mat;
    r[count++] = {block + c.us, (long)K * NP};
    r[count++] = {block + c.th, (long)K * d};
    r[count++] = {block + c.w2, (long)K};
    r[count++] = {block + c.colbuf, (long)2 * (NP + XR)};
    r[count++] = {block + c.dvec, (long)NP};
    r[count++] = {block + c.zb, (long)2 * NP};
    r[count++] = {block + c.slack, 8};
    if (inv) {
      r[count++] = {block + c.zmat, (long)NP * (NP + 2)};
      r[count++] = {block + c.part, (long)4 * kGradSlots};
      CHECK((block + c.zmat) % 2 == 0, "zmat 16-byte aligned n=%d d=%d K=%d", n, d, K);
    } else if (NE > 1) {
      r[count++] = {block + c.ut, (long)K * XR};
      r[count++] = {block + c.psum, (long)3 * XR * G};
    }
    blocks_end = block + c.per_mat;
    CHECK(r[count - 1].start + r[count - 1].size <= blocks_end, "matrix %d leaves its block n=%d d=%d K=%d", sub, n, d, K);
  }
  CHECK(c.xt == blocks_end, "xt follows the last matrix n=%d d=%d K=%d", n, d, K);
  if (NE > 1 && !inv) r[count++] = {c.xt, (long)d * XR};
  if (per_design)
    for (int sub = 0; sub < MPW; ++sub) r[count++] = {c.xs_own + (long)sub * d * n, (long)d * n};
  check_order(r, count, (long)total, "RegCarve", n, d, K);
}

// small_route over n 1..129, every d and K, both families and all six ops against the expressions it replaced.  Prints
// the counts of its last line; with `witness`, instead, the first shape (smallest n, then d, then K) of every reachable
// (op, route) cell of the Gaussian family, and of the shapes where ccgp_reserve now reserves the sweep's workspace.
static const char* const kOpNames[] = {"loglik", "predict", "inverse", "grad", "logdet_designs", "design_grad"};
static const char kRouteLetters[] = "rlbu";
static void check_routes(bool witness) {
  long reserve_m0 = 0, reserve_m = 0, predict_outside_lds = 0;
  bool seen[6][4] = {};
  bool seen_reserve = false;
  for (int n = 1; n <= kSmallMaxN + 1; ++n)
    for (int d = 1; d <= kMaxD; ++d)
      for (int K = 1; K <= kMaxK; ++K)
        for (int gauss = 1; gauss >= 0; --gauss) {
          for (int o = 0; o < 6; ++o) {
            const Op op = (Op)o;
            const Route r = small_route(op, gauss, n, d, K);
            CHECK(r == old::route(op, gauss, n, d, K), "small_route %s gauss=%d n=%d d=%d K=%d", kOpNames[o], gauss, n, d, K);
            if (witness && gauss && !seen[o][(int)r] && (op != Op::Inverse || K == 2)) {   // ccgp_logpost has two components
              seen[o][(int)r] = true;
              std::printf("%s %c %d %d %d\n", kOpNames[o], kRouteLetters[(int)r], n, d, K);
            }
          }
          const Route ll = small_route(Op::Loglik, gauss, n, d, K), pr = small_route(Op::Predict, gauss, n, d, K);
          CHECK((pr == Route::Reg) == old::fused(gauss, n, d), "predict route and ccgp_factor_batch's fused n=%d d=%d K=%d", n, d, K);
          CHECK(small_route_inverse_staged(gauss, n, d) == (old::logpost_blocked(gauss, n, d) ? Route::Blocked : Route::Lds),
                "staged inverse gauss=%d n=%d d=%d", gauss, n, d);
          CHECK(pr != Route::Reg || ll == Route::Reg, "prediction on the register evaluator without the likelihood n=%d d=%d K=%d", n, d, K);
          // ccgp_reserve: the sweep's workspace without test sites (m = 0) and with them
          const bool was = old::reserve_sweep(gauss, n), now_m0 = ll == Route::Blocked, now_m = now_m0 || pr == Route::Blocked;
          CHECK(!was || now_m0, "ccgp_reserve stopped reserving at gauss=%d n=%d d=%d K=%d", gauss, n, d, K);
          reserve_m0 += now_m0 != was;
          reserve_m += now_m != was;
          if (witness && now_m != was && !seen_reserve) {
            seen_reserve = true;
            std::printf("reserve b %d %d %d\n", n, d, K);
          }
          // is Predict's small.hip clause redundant?  shapes whose prediction instance fits outside small.hip's domain
          predict_outside_lds += gauss && n <= kSmallMaxN && small_reg_supported(n, d, K, false, true) && pr != Route::Reg;
        }
  if (!witness) std::printf("reserve %ld %ld predict_outside_lds %ld\n", reserve_m0, reserve_m, predict_outside_lds);
}

int main(int argc, char** argv) {
  const bool table = argc > 1 && !std::strcmp(argv[1], "table");
  if (argc > 1 && !std::strcmp(argv[1], "witness")) {
    check_routes(true);
    return failures != 0;
  }
  long dead_loglik = 0, dead_predict = 0, lds_grad = 0, lds_inverse_k2 = 0, old_lds_grad = 0, old_lds_inverse_k2 = 0;
  for (int n = 1; n <= kSmallMaxN; ++n) {
    const FacLayout fl(n);
    CHECK(fl.npf % 8 == 0 && fl.rd % 8 == 0 && fl.zy % 8 == 0 && fl.z1 % 8 == 0 && fl.L % 8 == 0 && fl.total % 8 == 0 &&
              fl.head == 8 + 3 * fl.npf && fl.total >= fl.L + n * (n - 1) / 2,
          "FacLayout n=%d", n);
    const SiteSolveCarve ss(n);
    CHECK(ss.total == old::site_solve_lds_doubles(n), "SiteSolveCarve total n=%d", n);
    const Region sr[] = {{ss.F, (long)fl.head}, {ss.L, (long)32 * (fl.npf / 8) * (fl.npf / 8)}};
    check_order(sr, 2, (long)ss.total, "SiteSolveCarve", n, 0, 0);
    // L' image: every row block's rectangle ends where its triangle starts, the triangle before the next block
    for (int I = 0; I < fl.npf / 8; ++I)
      CHECK(lrect(I, 8 * I, 0) == ltri(I, 1, 0) && ltri(I, 7, 6) < lrect(I + 1, 0, 0) && lrect(I + 1, 0, 0) <= 32 * (I + 1) * (I + 1),
            "L' image n=%d I=%d", n, I);
    for (int d = 1; d <= kMaxD; ++d) {
      for (int mt = 0; mt <= 256; mt += (mt < 2 ? 1 : 127)) {   // 0, 1, 2, 129, 256
        CHECK(small_lds_bytes(n, d, mt) == old::small_lds_bytes(n, d, mt), "small_lds_bytes n=%d d=%d mtile=%d", n, d, mt);
      }
      const int mtile = small_pick_mtile(n, d, n);
      CHECK(mtile == old::small_pick_mtile(n, d, n) && small_pick_mtile(n, d, 300) == old::small_pick_mtile(n, d, 300) &&
                small_pick_mtile(n, d, 0) == 1,
            "small_pick_mtile n=%d d=%d", n, d);
      const bool small1 = small_lds_bytes(n, d, 1) <= (size_t)kLdsBytes - 64, small0 = small_lds_bytes(n, d, 0) <= (size_t)kLdsBytes - 64;
      char inv_bits[kMaxK + 1] = {0}, routes[kMaxK + 1] = {0};
      for (int K = 1; K <= kMaxK; ++K) {
        // small_kernel carves with its own K inside what the host sized for kMaxK
        const SmallCarve sc(n, d, K, mtile);
        const Region kr[] = {{sc.A, (long)(n + 2 + mtile) * n}, {sc.xs, (long)d * n}, {sc.us, (long)K * n}, {sc.reserved, (long)(d + K) * mtile},
                             {sc.th, (long)K * d}, {sc.w2, (long)K}, {sc.red, 16}, {sc.etab, (long)kExpTableDoubles}};
        check_order(kr, 8, (long)(small_lds_bytes(n, d, mtile) / sizeof(double)), "SmallCarve", n, d, K);
        for (int waves = 1; waves <= 4; ++waves) {
          const SiteCorrCarve c(fl.npf, d, K, waves);
          CHECK(sizeof(double) * c.total == old::site_corr_lds_bytes(n, d, K, waves), "SiteCorrCarve total n=%d d=%d K=%d", n, d, K);
          const Region cr[] = {{c.th, (long)K * d}, {c.w2, 8}, {c.us, (long)K * fl.npf}, {c.xs, (long)K * d * fl.npf}, {c.xw, (long)waves * d * 64}};
          check_order(cr, 5, (long)c.total, "SiteCorrCarve", n, d, K);
          CHECK(c.xs % 2 == 0, "site_corr xs is read two doubles at a time");
        }
        // every instance the dispatchers can form
        const int nb8 = (n + 7) / 8, nb16 = (n + 15) / 16;
        for (int pd = 0; pd < 2; ++pd) {
          if (n <= 104) check_reg(8, nb8, 1, false, pd, n, d, K);   // NB 1..8, and 9..13 above 64
          check_reg(16, nb16, 1, false, pd, n, d, K);
          check_reg(16, nb16, nb16 + 1, true, pd, n, d, K);         // inverse / gradient; design gradient (per-design)
        }
        if (n <= 64) check_reg(8, nb8, kPredictNE, false, false, n, d, K);
        else check_reg(16, nb16, kPredictNE, false, false, n, d, K);
        // predicates
        for (int pd = 0; pd < 2; ++pd) {
          CHECK(small_reg_supported(n, d, K, pd, false) == old::small_reg_supported(n, d, K, pd, false), "small_reg_supported n=%d d=%d K=%d", n, d, K);
          CHECK(small_reg_fits8(n, d, K, pd) == old::fits8(n, d, K, pd), "fits8 n=%d d=%d K=%d", n, d, K);
        }
        CHECK(small_reg_supported(n, d, K, false, true) == old::small_reg_supported(n, d, K, false, true), "small_reg_supported(predict) n=%d d=%d K=%d", n, d, K);
        CHECK(small_reg_sites_supported(n, d, K) == old::small_reg_sites_supported(n, d, K), "small_reg_sites_supported n=%d d=%d K=%d", n, d, K);
        CHECK(small_reg_inverse_supported(n, d, K) == old::small_reg_inverse_supported(n, d, K), "small_reg_inverse_supported n=%d d=%d K=%d", n, d, K);
        CHECK(small_reg_design_grad_supported(n, d, K) == old::small_reg_design_grad_supported(n, d, K), "small_reg_design_grad_supported n=%d d=%d K=%d", n, d, K);
        // routes: the in-LDS value and prediction routes are gone; the gradient and solve(R) still reach small.hip
        dead_loglik += small0 && !small_reg_supported(n, d, K);
        dead_predict += small1 && !small_reg_supported(n, d, K, false, true);
        const bool lds_old = old::small_lds_bytes(n, d, 1) <= old::kLds - 64 && !old::small_reg_inverse_supported(n, d, K);
        lds_grad += small_route(Op::Grad, true, n, d, K) == Route::Lds;
        old_lds_grad += lds_old;
        if (K == 2) { lds_inverse_k2 += small_route(Op::Inverse, true, n, d, K) == Route::Lds; old_lds_inverse_k2 += lds_old; }
        inv_bits[K - 1] = small_reg_inverse_supported(n, d, K) ? '1' : '0';
        routes[K - 1] = kRouteLetters[(int)small_route(Op::Grad, true, n, d, K)];
      }
      if (table) std::printf("%d %d %zu %s %s\n", n, d, small_lds_bytes(n, d, 1), inv_bits, routes);
    }
  }
  CHECK(small_lds_bytes(129, 1, 1) == old::small_lds_bytes(129, 1, 1) && !small_reg_supported(129, 1, 1) && !small_reg_inverse_supported(129, 1, 1) &&
            !small_reg_design_grad_supported(129, 1, 1) && !small_reg_sites_supported(105, 1, 1) && !small_reg_sites_supported(8, 1, 4),
        "limits");
  CHECK(dead_loglik == 0 && dead_predict == 0, "shapes that needed the removed routes: %ld likelihood, %ld prediction", dead_loglik, dead_predict);
  CHECK(lds_grad == old_lds_grad && lds_inverse_k2 == old_lds_inverse_k2 && lds_grad > 0 && lds_inverse_k2 > 0, "in-LDS routes");
  check_routes(false);
  std::printf("dead %ld %ld lds_grad %ld lds_inverse_k2 %ld\n", dead_loglik, dead_predict, lds_grad, lds_inverse_k2);
  if (failures) { std::fprintf(stderr, "%ld checks failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
