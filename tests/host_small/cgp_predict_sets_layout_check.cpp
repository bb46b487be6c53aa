// CPU check of the staging of ccgp_cgp_predict_sets (csrc/call_stage.h: cgp_predict_sets_stage).  For chunks of nb rows over
// several shapes -- m = 0 included -- the pieces lie inside the buffer, 256-byte aligned, in order and without overlap: the
// sets, their responses and their test sites in front, then a chunk's set indices and rows (one span up), its m x 6 blocks,
// gathered states and status words (one span down), and behind them what never leaves the device (val | beta | tau2 and the
// kept blocks, CgpKeep(n).total doubles a row).  The planning pass measures what the real pass uses; a row's share is what
// the planner is told; inputs() names the sets and the test sites on the first chunk only; results() leaves the states out
// where the caller does not want them.  Built and run by tests/test_cgp_predict_sets_layout.py (also once with
// -fsanitize=address,undefined).  Prints the number of cases, then "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "call_stage.h"

using namespace ccgp;

#define CHECK(cond)                                                                                    \
  do {                                                                                                 \
    if (!(cond)) {                                                                                     \
      std::printf("FAILED %s (line %d): n %d d %d C %d m %d nb %d\n", #cond, __LINE__, g_n, g_d, g_C, g_m, g_nb); \
      std::exit(1);                                                                                    \
    }                                                                                                  \
  } while (0)
static int g_n, g_d, g_C, g_m, g_nb;

// CgpKeep(n).total of csrc/ccgp_internal.h by hand: the factor | Q^-1 1 | s | e^2 | temp | eight scalars
static size_t keep_by_hand(int n) { return (size_t)n * n + 4 * (size_t)n + 8; }

struct R { char* p; size_t b; };
static void check_tiling(char* base, size_t bytes, const std::vector<R>& r) {
  char* end = base;
  for (const R& x : r) {
    CHECK(x.p >= end && (x.p - base) % 256 == 0 && x.p + x.b <= base + bytes);   // declared in address order: no overlap
    end = x.p + x.b;
  }
  CHECK(end + 255 >= base + bytes);                                              // nothing but alignment behind the last piece
  for (const R& x : r) std::fill(x.p, x.p + x.b, (char)0x5a);                   // every byte of every piece is writable
}

static void check_stage(int n, int d, int C, int m, int nb) {
  g_n = n; g_d = d; g_C = C; g_m = m; g_nb = nb;
  const size_t keep = keep_by_hand(n), P = 2 * (size_t)d + 2, ns = 3 * (size_t)n + 3;
  std::vector<double> hX(1), hy(1), hXt(1), hp(1), o(1);
  std::vector<int> hset(1);
  const size_t bytes = layout_bytes([&](Layout& c) { cgp_predict_sets_stage(c, n, d, C, m, keep, nb); });
  Layout plan;
  const CgpPredictSetsStage p = cgp_predict_sets_stage(plan, n, d, C, m, keep, nb);
  CHECK(!p.Xs && !p.ys && !p.Xtests && !p.set && !p.params && !p.out && !p.state && !p.status && !p.res && !p.keep);
  CHECK(plan.off == bytes);
  // what the planner is told per row, against what 256 more rows take: ten pieces, each rounded up once
  CHECK(cgp_predict_sets_row_bytes(n, d, m, keep) == 8 * (P + 6 * (size_t)m + ns + 3 + keep) + 8);
  const size_t more = layout_bytes([&](Layout& c) { cgp_predict_sets_stage(c, n, d, C, m, keep, nb + 256); });
  CHECK(more - bytes <= 256 * cgp_predict_sets_row_bytes(n, d, m, keep) + 10 * 256);
  CHECK(more - bytes + 10 * 256 >= 256 * cgp_predict_sets_row_bytes(n, d, m, keep));
  char* base = static_cast<char*>(std::aligned_alloc(256, bytes + 256));
  Layout real(base);
  const CgpPredictSetsStage s = cgp_predict_sets_stage(real, n, d, C, m, keep, nb);
  CHECK(real.off == bytes && s.P == P && s.nout == 6 * (size_t)m && s.nstate == ns);
  const std::vector<R> r = {{(char*)s.Xs, 8 * (size_t)C * n * d},     {(char*)s.ys, 8 * (size_t)C * n},
                            {(char*)s.Xtests, 8 * (size_t)C * m * d}, {(char*)s.set, 4 * (size_t)nb},
                            {(char*)s.params, 8 * (size_t)nb * P},    {(char*)s.out, 8 * (size_t)nb * 6 * m},
                            {(char*)s.state, 8 * (size_t)nb * ns},    {(char*)s.status, 4 * (size_t)nb},
                            {(char*)s.res, 8 * 3 * (size_t)nb},       {(char*)s.keep, 8 * (size_t)nb * keep}};
  check_tiling(base, bytes, r);
  // row r's kept block ends where row r + 1's begins, and the last one inside the buffer
  CHECK((char*)(s.keep + (size_t)nb * keep) <= base + bytes);
  for (int first = 1; first >= 0; --first) {
    const std::vector<Piece> in = s.inputs(first, hX.data(), hy.data(), hXt.data(), hset.data(), hp.data(), nb);
    CHECK(in.size() == 5);
    for (int i = 0; i < 5; ++i) CHECK(in[i].dev == r[i].p && in[i].bytes == r[i].b);
    for (int i = 0; i < 3; ++i) CHECK((in[i].host != nullptr) == (first == 1));
    CHECK(in[3].host && in[4].host);
    const Span up = span_of(in);   // a later chunk moves its set indices and rows only
    CHECK(up.lo == (first ? (char*)s.Xs : (char*)s.set) && up.lo + up.bytes == (char*)s.params + 8 * (size_t)nb * P);
  }
  for (int want_state = 1; want_state >= 0; --want_state) {
    const std::vector<Piece> out = s.results(m ? o.data() : nullptr, want_state ? o.data() : nullptr, nb);
    CHECK(out.size() == 2 && out[0].dev == r[5].p && out[0].bytes == r[5].b);
    CHECK(out[1].dev == r[6].p && out[1].bytes == r[6].b);
    // with the status words behind them (pull_status) the results are one span that ends before what stays on the device
    std::vector<Piece> all = out;
    all.push_back(piece(s.status, hset.data(), (size_t)nb));
    const Span down = span_of(all);
    const char* lo = m ? (char*)s.out : (want_state ? (char*)s.state : (char*)s.status);
    CHECK(down.lo == lo && down.lo + down.bytes == (char*)s.status + 4 * (size_t)nb && down.lo + down.bytes <= (char*)s.res);
  }
  std::free(base);
}

int main() {
  int cases = 0;
  const int shapes[][4] = {{1, 1, 1, 0},  {1, 1, 1, 1}, {6, 2, 2, 3},   {50, 4, 3, 150},   {50, 9, 17, 150},
                           {64, 3, 2, 0}, {65, 1, 4, 7}, {128, 2, 2, 5}, {128, 21, 2, 257}};   // n, d, C, m
  for (const auto& sh : shapes)
    for (int nb : {1, 2, 31, 32, 33, 64, 1000}) {
      check_stage(sh[0], sh[1], sh[2], sh[3], nb);
      ++cases;
    }
  std::printf("cases %d\nok\n", cases);
  return 0;
}
