// csrc/stage_layout.h and csrc/call_stage.h on the CPU.
// Layout: for each list of pieces, the planning pass (no base) and the carving pass (over a base) run the SAME
// declaration and must end at the same offset; every pointer is 256-byte aligned, and the pieces lie inside
// [base, base + off) without overlapping.  The base is an address that is never dereferenced, so sizes above 4 GiB need
// no memory.
// call_stage.h: the declarations the library itself stages its calls with, at three shapes, with and without every
// optional piece: both passes end at the same offset, what a call pushes and what it pulls are each one run of
// 256-byte-aligned pieces lying back to back, and the staging ccgp_reserve provides holds every layout it reserves for.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../convex-combination-of-gaussian-processes_amd/csrc/call_stage.h"

using namespace ccgp;

struct PieceSpec {
  int elem;        // 1: char, 4: int, 8: double
  size_t count;
};

static void declare(Layout& c, const std::vector<PieceSpec>& ps, std::vector<char*>* out) {
  for (const PieceSpec& p : ps) {
    char* q = p.elem == 8   ? reinterpret_cast<char*>(c.take<double>(p.count))
              : p.elem == 4 ? reinterpret_cast<char*>(c.take<int>(p.count))
                            : c.take<char>(p.count);
    if (out) out->push_back(q);
  }
}

static int check(const char* name, const std::vector<PieceSpec>& ps) {
  std::vector<char*> planned, got;
  Layout plan;
  declare(plan, ps, &planned);
  const size_t bytes = ccgp::layout_bytes([&](Layout& c) { declare(c, ps, nullptr); });
  char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);
  Layout real(base);
  declare(real, ps, &got);
  int bad = 0;
  if (plan.off != real.off || bytes != real.off) {
    std::printf("%s: planning ends at %zu / %zu, carving at %zu\n", name, plan.off, bytes, real.off);
    ++bad;
  }
  size_t end_prev = 0;
  for (size_t i = 0; i < ps.size(); ++i) {
    const size_t len = ps[i].count * (size_t)ps[i].elem;
    if (planned[i] != nullptr) { std::printf("%s: piece %zu: the planning pass handed out a pointer\n", name, i); ++bad; }
    const size_t off = (size_t)(got[i] - base);
    if (reinterpret_cast<uintptr_t>(got[i]) % 256) { std::printf("%s: piece %zu not 256-byte aligned\n", name, i); ++bad; }
    if (off < end_prev) { std::printf("%s: piece %zu overlaps its predecessor\n", name, i); ++bad; }
    if (off + len > real.off) { std::printf("%s: piece %zu ends at %zu, beyond %zu\n", name, i, off + len, real.off); ++bad; }
    end_prev = off + len;
  }
  return bad;
}

// ---- the library's own declarations -----------------------------------------------------------------------------------
static char* const kBase = reinterpret_cast<char*>(uintptr_t(1) << 40);
static double host_d[1];   // stands for every host array: set, never dereferenced
static int host_i[1];
static char tag[160];

static size_t off_of(const void* p) { return (size_t)(static_cast<const char*>(p) - kBase); }

// `lay` over no base and over kBase: the same end; returns it
template <class F>
static size_t both_passes(int* bad, F&& lay) {
  const size_t planned = layout_bytes(lay);
  Layout real(kBase);
  lay(real);   // last: the caller reads the pointers
  if (planned != real.off) { std::printf("%s: planning ends at %zu, carving at %zu\n", tag, planned, real.off); ++*bad; }
  return real.off;
}

// the pieces that move (host set, bytes > 0), taken in address order, are 256-byte aligned, lie inside [kBase, kBase + end),
// and each starts where its predecessor's 256-byte line ends -- but for `gap` bytes in all (0 everywhere except
// the per-row tail of the prediction layout, which lies behind the other side's pieces); span_of covers exactly that run
static int one_run(const char* side, std::vector<Piece> ps, size_t end, size_t gap = 0) {
  std::sort(ps.begin(), ps.end(), [](const Piece& a, const Piece& b) { return a.dev < b.dev; });
  int bad = 0, moving = 0;
  size_t first = 0, next = 0, last_end = 0, gaps = 0;
  for (const Piece& p : ps) {
    if (!p.host || !p.bytes) continue;
    const size_t o = off_of(p.dev);
    if (o % 256) { std::printf("%s %s: piece at %zu not 256-byte aligned\n", tag, side, o); ++bad; }
    if (moving == 0) first = o;
    else if (o < next) { std::printf("%s %s: piece at %zu overlaps its predecessor\n", tag, side, o); ++bad; }
    else gaps += o - next;
    last_end = o + p.bytes;
    next = Layout::al(last_end);
    ++moving;
  }
  if (gaps != gap) { std::printf("%s %s: %zu bytes between the pieces, expected %zu\n", tag, side, gaps, gap); ++bad; }
  if (last_end > end) { std::printf("%s %s: ends at %zu, beyond %zu\n", tag, side, last_end, end); ++bad; }
  const Span sp = span_of(ps);
  if (moving == 0 ? sp.lo != nullptr : (off_of(sp.lo) != first || sp.bytes != last_end - first)) {
    std::printf("%s %s: span_of disagrees with the pieces\n", tag, side);
    ++bad;
  }
  return bad;
}

static std::vector<Piece> with_status(std::vector<Piece> ps, int* status, size_t count) {
  ps.push_back(piece(status, host_i, count));
  return ps;
}

static int check_shape(int n, int d, int K, int B, int m) {
  const int P = K + K * d;
  const size_t reserved = reserve_stage_bytes(n, d, P, B, m);
  int bad = 0;
  auto holds = [&](size_t bytes) {
    if (bytes > reserved) { std::printf("%s: %zu B, ccgp_reserve provides %zu\n", tag, bytes, reserved); ++bad; }
  };
  {
    std::snprintf(tag, sizeof tag, "loglik n=%d d=%d K=%d B=%d", n, d, K, B);
    LoglikStage s;
    const size_t end = both_passes(&bad, [&](Layout& c) { s = loglik_stage(c, n, d, P, B); });
    holds(end);
    const size_t in_b = 8 * ((size_t)n * d + n + (size_t)B * P), out_b = 8 * (2 * (size_t)B + ((size_t)B + 1) / 2);
    // X | y | params are ONE piece, and so are loglik | beta | status with the word that makes the status whole doubles
    const Span up = span_of({piece(s.X, host_d, (size_t)n * d), piece(s.y, host_d, n), piece(s.params, host_d, (size_t)B * P)});
    const Span down = span_of({piece(s.loglik, host_d, B), piece(s.beta, host_d, B), piece(s.status, host_i, (size_t)B + (B & 1))});
    if (off_of(up.lo) != 0 || up.bytes != in_b || off_of(down.lo) != Layout::al(in_b) || down.bytes != out_b ||
        off_of(s.y) != 8 * (size_t)n * d || s.beta != s.loglik + B || s.payload != in_b + out_b || end != Layout::al(in_b) + Layout::al(out_b)) {
      std::printf("%s: the two pieces are not %zu + %zu bytes\n", tag, in_b, out_b);
      ++bad;
    }
  }
  for (int opt = 0; opt < 8; ++opt) {
    const bool grad = opt & 1, s2hat = opt & 2;
    const size_t gpart = opt & 4 ? (size_t)B * 3 * P : 0;
    if (!grad && !s2hat) continue;   // value only is legal in the profiled mode alone
    std::snprintf(tag, sizeof tag, "grad n=%d d=%d K=%d B=%d grad=%d s2hat=%d gpart=%zu", n, d, K, B, grad, s2hat, gpart);
    GradStage s;
    const size_t end = both_passes(&bad, [&](Layout& c) { s = grad_stage(c, n, d, P, B, grad, s2hat, gpart); });
    if (!s.o.grad != !grad || !s.o.s2hat != !s2hat || !s.o.gpart != !gpart) { std::printf("%s: optional pieces\n", tag); ++bad; }
    bad += one_run("push", s.inputs(host_d, host_d, host_d), end);
    bad += one_run("pull", with_status(s.results(host_d, host_d, host_d, host_d), s.o.status, B), end);
  }
  for (int tail = 0; tail < 2; ++tail) {
    std::snprintf(tag, sizeof tag, "predict n=%d d=%d K=%d S=%d m=%d tail=%d", n, d, K, B, m, tail);
    PredictStage s;
    const size_t end = both_passes(&bad, [&](Layout& c) { s = predict_stage(c, n, d, P, B, m, tail); });
    if (!tail && m > 0) holds(end);
    // the tail lies behind the status words: sigma2 goes up from behind the results, Q comes back from behind sigma2
    const size_t tables = 2 * Layout::al(8 * (size_t)B * m), words = Layout::al(8 * (size_t)B);
    bad += one_run("push", s.inputs(host_d, host_d, host_d, host_d, host_d), end, tail ? tables + words + Layout::al(4 * (size_t)B) : 0);
    bad += one_run("pull", with_status(s.results(host_d, host_d, host_d, host_d), s.status, B), end, tail ? words : 0);
    if (tail && (off_of(s.q) + words != end || off_of(s.sigma2) + 2 * words != end)) { std::printf("%s: the tail\n", tag); ++bad; }
  }
  for (int opt = 0; opt < 4; ++opt) {
    const int n_probs = opt & 1 ? 8 : 0;
    const bool y_at = opt & 2;
    std::snprintf(tag, sizeof tag, "summary n=%d d=%d K=%d S=%d m=%d n_probs=%d y_at=%d", n, d, K, B, m, n_probs, y_at);
    SummaryStage s;
    const size_t end = both_passes(&bad, [&](Layout& c) { s = summary_stage(c, n, d, P, B, m, n_probs); });
    bad += one_run("push", s.inputs(host_d, host_d, host_d, host_d, y_at ? host_d : nullptr), end);
    bad += one_run("pull", with_status(s.results(host_d, host_d), s.status, B), end);
    if (off_of(s.t.mean) < off_of(s.y_at) + 8 * (size_t)m || off_of(s.t.count) + 4 > off_of(s.out)) {
      std::printf("%s: the tables do not lie between the inputs and the results\n", tag);
      ++bad;
    }
  }
  for (int own = 0; own < 2; ++own) {
    std::snprintf(tag, sizeof tag, "summary_dev S=%d m=%d own_status=%d", B, m, own);
    SummaryDevStage s;
    const size_t end = both_passes(&bad, [&](Layout& c) { s = summary_dev_stage(c, B, m, own); });
    if (m > 0) holds(end);
    if (!s.status != !own) { std::printf("%s: status\n", tag); ++bad; }
  }
  for (int opt = 0; opt < 4; ++opt) {
    std::snprintf(tag, sizeof tag, "predict_tail S=%d beta=%d status=%d", B, opt & 1, opt >> 1);
    SweepOut p;
    const size_t end = both_passes(&bad, [&](Layout& t) { p = predict_tail(t, B, opt & 1 ? host_d : nullptr, opt & 2 ? host_i : nullptr); });
    const size_t want = Layout::al(8 * (size_t)B) * (opt & 1 ? 1 : 2) + (opt & 2 ? 0 : Layout::al(4 * (size_t)B));
    if (end != want || (opt & 1 && p.beta != host_d) || (opt & 2 && p.status != host_i)) { std::printf("%s: %zu B\n", tag, end); ++bad; }
  }
  return bad;
}

// (n, d, K, B) = (5, 2, 2, 3): every piece is under 256 bytes, so the offsets can be written down by hand
static int check_pinned_offsets() {
  int bad = 0;
  auto at = [&](const char* what, const void* p, size_t want) {
    if (off_of(p) != want) { std::printf("pinned offsets: %s at %zu, expected %zu\n", what, off_of(p), want); ++bad; }
  };
  Layout c(kBase);
  const GradStage g = grad_stage(c, 5, 2, 6, 3, true, false, 0);
  at("X", g.X, 0); at("y", g.y, 256); at("params", g.params, 512); at("grad", g.o.grad, 768);
  at("loglik", g.o.loglik, 1024); at("beta", g.o.beta, 1280); at("status", g.o.status, 1536);
  if (c.off != 1792 || g.o.s2hat || g.o.gpart) { std::printf("pinned offsets: the gradient layout ends at %zu\n", c.off); ++bad; }
  Layout c2(kBase);
  const GradStage p = grad_stage(c2, 5, 2, 6, 3, true, true, 0);
  at("profiled loglik", p.o.loglik, 1024); at("s2hat", p.o.s2hat, 1280); at("profiled beta", p.o.beta, 1536);
  at("profiled status", p.o.status, 1792);
  if (c2.off != 2048) { std::printf("pinned offsets: the profiled layout ends at %zu, expected 2048\n", c2.off); ++bad; }
  return bad;
}

int main() {
  const size_t big = (size_t(5) << 30) / 8 + 3;   // doubles: more than 4 GiB, not a multiple of 256 bytes
  int bad = 0;
  bad += check("empty", {});
  bad += check("one double", {{8, 1}});
  bad += check("odd int counts", {{8, 33}, {4, 1}, {4, 7}, {8, 5}, {4, 65}, {4, 63}, {8, 1}});
  bad += check("zero-length pieces", {{8, 0}, {8, 12}, {4, 0}, {4, 0}, {8, 32}, {1, 0}});
  bad += check("exact multiples of 256 bytes", {{8, 32}, {4, 64}, {1, 256}, {8, 64}});
  bad += check("bytes then tail", {{1, 1000003}, {8, 17}, {8, 128}});
  bad += check("above 4 GiB", {{8, big}, {4, 3}, {8, big}, {1, (size_t(4) << 30) + 1}, {4, 5}});
  bad += check_shape(5, 2, 2, 3, 0);
  bad += check_shape(64, 4, 2, 7, 5);
  bad += check_shape(128, 5, 3, 1000, 150);
  bad += check_pinned_offsets();
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
