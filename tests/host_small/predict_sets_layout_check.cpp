// CPU check of the staging of ccgp_predict_batch_sets, ccgp_krige_predict_batch_sets and ccgp_predict_summary_sets
// (csrc/call_stage.h: predict_sets_stage).  For several shapes, row counts per set (a set without rows among them) and each
// of the three calls with and without its optional inputs: every piece lies inside the buffer, 256-byte aligned, in address
// order without overlap; the three passes follow one another -- all inputs, then all tables, then all results -- so that the
// pieces that go up are one span that ends before the first table, and the pieces that come down are one span: behind the
// tables for a summary (which leaves them on the device), from the first table on otherwise; a set no row refers to takes
// nothing; `off` counts the grouped rows; the planning pass measures what the real pass uses.  That is the grouped route.  For
// the one-launch route: small_route_predict_sets walked over n 1..129, every d, K and family -- Reg exactly where the family is
// Gaussian, n <= 104, K <= 3, the single-set kept-factor carves fit and the sets instance's carve fits (summed here by hand:
// on the 8 x 8 grid four matrices and a design copy each) --, the dynamic LDS of the FAC + SETS instances at pinned shapes on
// both grids, every one <= 160 KiB - 64, and the tiling of predict_sets_one_stage: inputs one span in front, results one span
// behind the tables.  Built and run by tests/test_predict_sets_layout.py (both exp settings; once with
// -fsanitize=address,undefined).  Prints the route counts, the pinned LDS totals, the number of staging cases, then "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "call_stage.h"
#include "small_layout.h"

using namespace ccgp;

#define CHECK(cond)                                                                                      \
  do {                                                                                                   \
    if (!(cond)) {                                                                                       \
      std::printf("FAILED %s (line %d): n %d d %d P %d m %d op %d opt %d\n", #cond, __LINE__, g[0], g[1], g[2], g[3], g[4], g[5]); \
      std::exit(1);                                                                                      \
    }                                                                                                    \
  } while (0)
static int g[6];

struct R { char* p; size_t b; };

static void check(const std::vector<int>& nb_of, int n, int d, int P, int m, int op, bool opt, int n_probs) {
  g[0] = n; g[1] = d; g[2] = P; g[3] = m; g[4] = op; g[5] = opt;
  const bool krige = op == 1, summary = op == 2;
  const bool s2row = krige && opt, y_at = summary && opt;
  const size_t nout = summary ? (size_t)m * (4 + n_probs) : 0;
  auto lay = [&](Layout& w) { return predict_sets_stage(w, nb_of, n, d, P, m, krige, s2row, summary, y_at, nout); };
  const size_t bytes = layout_bytes(lay);
  Layout plan;
  for (const SetPieces& s : lay(plan)) CHECK(!s.X && !s.mean && !s.beta && !s.status);
  CHECK(plan.off == bytes);
  char* base = static_cast<char*>(std::aligned_alloc(256, bytes + 256));
  Layout real(base);
  const std::vector<SetPieces> sp = lay(real);
  CHECK(real.off == bytes && sp.size() == nb_of.size());
  std::vector<R> in, tab, res;
  int off = 0;
  for (size_t c = 0; c < sp.size(); ++c) {
    const SetPieces& s = sp[c];
    CHECK(s.nb == nb_of[c] && s.off == off);
    off += s.nb;
    if (!s.nb) {   // nothing staged
      CHECK(!s.X && !s.y && !s.params && !s.Xt && !s.s2row && !s.y_at && !s.mean && !s.var && !s.idx && !s.count && !s.out &&
            !s.beta && !s.q && !s.status);
      continue;
    }
    const size_t nb = (size_t)s.nb;
    in.push_back({(char*)s.X, 8 * (size_t)n * d});
    in.push_back({(char*)s.y, 8 * (size_t)n});
    in.push_back({(char*)s.params, 8 * nb * P});
    in.push_back({(char*)s.Xt, 8 * (size_t)m * d});
    CHECK((s.s2row != nullptr) == s2row && (s.y_at != nullptr) == y_at);
    if (s.s2row) in.push_back({(char*)s.s2row, 8 * nb});
    if (s.y_at) in.push_back({(char*)s.y_at, 8 * (size_t)m});
    tab.push_back({(char*)s.mean, 8 * nb * m});
    tab.push_back({(char*)s.var, 8 * nb * m});
    CHECK((s.idx != nullptr) == summary && (s.count != nullptr) == summary && (s.out != nullptr) == summary);
    if (summary) { tab.push_back({(char*)s.idx, 4 * nb}); tab.push_back({(char*)s.count, 4}); }
    if (summary) res.push_back({(char*)s.out, 8 * nout});
    res.push_back({(char*)s.beta, 8 * nb});
    CHECK((s.q != nullptr) == krige);
    if (krige) res.push_back({(char*)s.q, 8 * nb});
    res.push_back({(char*)s.status, 4 * nb});
  }
  // the three passes in address order, nothing overlapping, everything aligned and inside, every byte writable
  std::vector<R> all = in;
  all.insert(all.end(), tab.begin(), tab.end());
  all.insert(all.end(), res.begin(), res.end());
  char* end = base;
  for (const R& x : all) {
    CHECK(x.p >= end && (x.p - base) % 256 == 0 && x.p + x.b <= base + bytes);
    end = x.p + x.b;
  }
  CHECK(all.empty() ? bytes == 0 : end + 255 >= base + bytes);
  for (const R& x : all) std::fill(x.p, x.p + x.b, (char)0x5a);
  if (!all.empty()) {
    double host = 0.0;
    std::vector<Piece> up, down;
    for (const R& x : in) up.push_back(Piece{x.p, &host, x.b});
    if (!summary) for (const R& x : tab) down.push_back(Piece{x.p, &host, x.b});
    for (const R& x : res) down.push_back(Piece{x.p, &host, x.b});
    const Span u = span_of(up), dn = span_of(down);
    CHECK(u.lo == in.front().p && u.lo + u.bytes == in.back().p + in.back().b && u.lo + u.bytes <= tab.front().p);
    CHECK(dn.lo == (summary ? res.front().p : tab.front().p) && dn.lo + dn.bytes == res.back().p + res.back().b);
    CHECK(!summary || dn.lo >= tab.back().p + tab.back().b);   // a summary's tables stay on the device: not inside the span
  }
  std::free(base);
}

// the FAC + SETS instance's LDS in doubles, by hand.  Per matrix: us[K][NP] th[K][d] w2[K] colbuf[2][NP + G] dvec[NP] zb[2][NP]
// slack[8]; in front the exp table and the shared design slot; 8 x 8 grid: four matrices, and a design copy per matrix behind
static size_t sets_fac_by_hand(int G, int n, int d, int K) {
  const int NB = (n + G - 1) / G, NP = G * NB, MPW = 256 / (G * G);
  const size_t per = (size_t)K * NP + (size_t)K * d + K + 2 * (size_t)(NP + G) + NP + 2 * (size_t)NP + 8;
  return (size_t)(CCGP_SMALL_EXP_TABLE ? 256 : 0) + (size_t)d * n + MPW * per + (MPW > 1 ? (size_t)MPW * d * n : 0);
}
static bool fits(size_t doubles) { return 8 * doubles <= (size_t)160 * 1024 - 64; }

static void check_one_stage(int n, int d, int P, int C, int B, int m, int op, bool opt, int n_probs) {
  g[0] = n; g[1] = d; g[2] = P; g[3] = m; g[4] = op; g[5] = opt;
  const bool krige = op == 1, summary = op == 2;
  const bool s2row = !krige || opt, y_at = summary && opt;
  const size_t nout = summary ? (size_t)m * (4 + n_probs) : 0;
  auto lay = [&](Layout& w) { return predict_sets_one_stage(w, n, d, P, C, B, m, krige, s2row, summary, y_at, nout); };
  const size_t bytes = layout_bytes(lay);
  char* base = static_cast<char*>(std::aligned_alloc(256, bytes + 256));
  Layout real(base);
  const PredictSetsOneStage s = lay(real);
  CHECK(real.off == bytes);
  CHECK((s.s2row != nullptr) == s2row && (s.y_at != nullptr) == y_at && (s.idx != nullptr) == summary &&
        (s.count != nullptr) == summary && (s.out != nullptr) == summary && (s.q != nullptr) == krige);
  std::vector<R> r = {{(char*)s.Xs, 8 * (size_t)C * n * d}, {(char*)s.ys, 8 * (size_t)C * n}, {(char*)s.sigma2_set, 8 * (size_t)C},
                      {(char*)s.Xtests, 8 * (size_t)C * m * d}, {(char*)s.set, 4 * (size_t)B}, {(char*)s.off, 4 * (size_t)C},
                      {(char*)s.nb, 4 * (size_t)C}, {(char*)s.params, 8 * (size_t)B * P}};
  if (s2row) r.push_back({(char*)s.s2row, 8 * (size_t)B});
  if (y_at) r.push_back({(char*)s.y_at, 8 * (size_t)C * m});
  const size_t n_in = r.size();
  r.push_back({(char*)s.mean, 8 * (size_t)B * m});
  r.push_back({(char*)s.var, 8 * (size_t)B * m});
  if (summary) { r.push_back({(char*)s.idx, 4 * (size_t)B}); r.push_back({(char*)s.count, 4 * (size_t)C}); }
  const size_t n_tab = r.size();
  if (summary) r.push_back({(char*)s.out, 8 * (size_t)C * nout});
  r.push_back({(char*)s.beta, 8 * (size_t)B});
  if (krige) r.push_back({(char*)s.q, 8 * (size_t)B});
  r.push_back({(char*)s.status, 4 * (size_t)B});
  char* end = base;
  for (const R& x : r) {
    CHECK(x.p >= end && (x.p - base) % 256 == 0 && x.p + x.b <= base + bytes);
    end = x.p + x.b;
  }
  CHECK(end + 255 >= base + bytes);
  for (const R& x : r) std::fill(x.p, x.p + x.b, (char)0x5a);
  double hd = 0.0;
  int hi = 0;
  const std::vector<Piece> up = s.inputs(&hd, &hd, &hd, &hd, &hi, &hi, &hi, &hd, s2row ? &hd : nullptr, y_at ? &hd : nullptr);
  const Span u = span_of(up);
  CHECK(u.lo == r[0].p && u.lo + u.bytes == r[n_in - 1].p + r[n_in - 1].b && u.lo + u.bytes <= r[n_in].p);
  const std::vector<Piece> down = s.results(summary ? nullptr : &hd, summary ? nullptr : &hd, summary ? &hd : nullptr, &hd,
                                            krige ? &hd : nullptr, &hi);
  const Span dn = span_of(down);
  CHECK(dn.lo == (summary ? r[n_tab].p : r[n_in].p) && dn.lo + dn.bytes == r.back().p + r.back().b);
  std::free(base);
}

int main() {
  // ---- the route, and the carve of the instances it launches
  long reg = 0, grouped = 0;
  for (int n = 1; n <= 129; ++n)
    for (int d = 1; d <= kMaxD; ++d)
      for (int K = 1; K <= kMaxK; ++K)
        for (int fam = 0; fam < 3; ++fam) {
          g[0] = n; g[1] = d; g[2] = K; g[3] = fam; g[4] = g[5] = 0;
          const bool gauss = fam == 0;
          const bool single = n <= 104 && K <= 3 && fits(sets_fac_by_hand(8, n, d, K) - (size_t)4 * d * n) &&   // no design copies
                              lds_fits(SiteSolveCarve(n).total, 2) && lds_fits(SiteCorrCarve(fac_npf(n), d, K, 4).total, 2);
          const bool sets = n <= 128 && fits(sets_fac_by_hand(16, n, d, K)) && (n > 64 || fits(sets_fac_by_hand(8, n, d, K)));
          const bool want = gauss && single && sets;
          CHECK((small_route_predict_sets(gauss, n, d, K) == Route::Reg) == want);
          CHECK(!want || small_route(Op::Predict, true, n, d, K) == Route::Reg);   // where the single-set call keeps its factor
          if (want) {
            // what launch_one asks for on either grid is the hand sum, and the grid a call takes has a carve that fits
            CHECK(reg_lds_doubles(16, (n + 15) / 16, 1, false, false, n, d, K) == sets_fac_by_hand(16, n, d, K));
            CHECK(reg_lds_doubles(8, (n + 7) / 8, 1, false, true, n, d, K) == sets_fac_by_hand(8, n, d, K));
            for (int B : {1, 64, 65, 100000}) {
              const int G = small_reg_sets_grid(n, d, K, B);
              CHECK(fits(sets_fac_by_hand(G, n, d, K)));
            }
          }
          (want ? reg : grouped)++;
        }
  std::printf("reg %ld grouped %ld\n", reg, grouped);
  const int pins[][3] = {{5, 1, 1}, {14, 2, 2}, {17, 2, 1}, {40, 3, 2}, {50, 9, 2}, {64, 4, 2}, {65, 3, 3}, {104, 2, 2}};
  std::printf("lds16");
  for (const auto& q : pins) std::printf(" %zu", 8 * sets_fac_by_hand(16, q[0], q[1], q[2]));
  std::printf("\nlds8");
  for (const auto& q : pins) std::printf(" %zu", 8 * sets_fac_by_hand(8, q[0], q[1], q[2]));
  std::printf("\n");
  for (const auto& q : pins) CHECK(fits(sets_fac_by_hand(16, q[0], q[1], q[2])) && fits(sets_fac_by_hand(8, q[0], q[1], q[2])));
  int cases = 0;
  const std::vector<std::vector<int>> counts = {{3},        {2, 1}, {4, 0, 3}, {0, 0, 5}, {1, 1, 1, 1, 1, 1, 1, 1, 37},
                                                {1000, 0, 64, 65}, {0, 0}};   // rows per set
  const int shapes[][4] = {{5, 1, 1, 1},    {14, 2, 2, 7},   {17, 2, 1, 64},
                           {50, 9, 2, 150}, {65, 3, 3, 257}, {129, 2, 2, 3}};   // n d K m
  for (const auto& nb_of : counts)
    for (const auto& sh : shapes)
      for (int op = 0; op < 3; ++op)
        for (int opt = 0; opt < 2; ++opt)
          for (int n_probs : {0, 2, 8}) {
            if (op != 2 && n_probs != 0) continue;
            check(nb_of, sh[0], sh[1], sh[2] + sh[2] * sh[1], sh[3], op, opt != 0, n_probs);
            ++cases;
          }
  for (const auto& sh : shapes)
    for (int C : {1, 3, 17})
      for (int op = 0; op < 3; ++op)
        for (int opt = 0; opt < 2; ++opt) {
          check_one_stage(sh[0], sh[1], sh[2] + sh[2] * sh[1], C, 5 * C + 2, sh[3], op, opt != 0, op == 2 ? 2 : 0);
          ++cases;
        }
  std::printf("cases %d\nok\n", cases);
  return 0;
}
