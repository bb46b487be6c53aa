// CPU check of the sets forms of the comparator fits (csrc/small_layout.h: small_route_profile_grad_sets; csrc/call_stage.h:
// profile_sets_stage, cgp_sets_stage).  Walks n 1..129, every d, K and kernel family: the profiled gradient over sets is ONE
// launch exactly where the family is Gaussian and ccgp_profile_batch's gradient takes the register-resident instance -- the
// in-LDS tier's boundary and the INV = 2 carve, both summed here by hand -- and the dynamic LDS the launcher asks for (the carve
// of the single-set instance: one matrix per workgroup, the set's design in the shared xs slot, no design copy) is that hand
// sum.  Then the two chunked stages: for a chunk of nb rows their pieces lie inside the buffer, 256-byte aligned, in order and
// without overlap, the sets in front; the planning pass measures what the real pass uses; a row's share is what the planner is
// told; inputs() names the sets on the first chunk only.  Built and run by tests/test_comparator_sets_layout.py (also once with
// -fsanitize=address,undefined).  Prints the counts and the pinned totals, then "ok".
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

static bool fits(size_t doubles) { return 8 * doubles <= (size_t)160 * 1024 - 64; }
// the gradient instance's LDS in doubles, summed by hand: exp table | the set's design | ONE matrix of
// us[K][NP] th[K][d] w2[K] colbuf[2][NP + 16 (NB + 1)] dvec[NP] zb[2][NP] slack[8] | bump | zmat[NP][NP + 2] | part[4][28]
static size_t grad_by_hand(int n, int d, int K) {
  const int NB = (n + 15) / 16, NP = 16 * NB, XR = 16 * (NB + 1);
  return (size_t)(CCGP_SMALL_EXP_TABLE ? 256 : 0) + (size_t)d * n + (size_t)K * NP + (size_t)K * d + K + 2 * (size_t)(NP + XR) + NP +
         2 * (size_t)NP + 8 + 1 + (size_t)NP * (NP + 2) + 4 * 28;
}
// small.hip's carve with one unit row, sized for kMaxK: the boundary of the tier whose shapes have a register gradient
static size_t lds_tier_by_hand(int n, int d) {
  return (size_t)(n + 3) * n + (size_t)d * n + (size_t)kMaxK * n + d + kMaxK + (size_t)kMaxK * d + kMaxK + 16 + 256;
}

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

static void check_stages(int n, int d, int K, int C, int nb) {
  g_n = n; g_d = d; g_K = K;
  const int P = K + K * d;
  std::vector<double> hX(1), hy(1), hp(1), o(4);
  std::vector<int> hset(1), hskip(1);
  {
    const size_t bytes = layout_bytes([&](Layout& c) { profile_sets_stage(c, n, d, P, C, nb); });
    Layout plan;
    const ProfileSetsStage p = profile_sets_stage(plan, n, d, P, C, nb);
    CHECK(!p.Xs && !p.ys && !p.set && !p.params && !p.grad && !p.loglik && !p.s2hat && !p.beta && !p.status && plan.off == bytes);
    // one more row costs no more than the planner is told, up to the alignment of the seven row pieces
    const size_t more = layout_bytes([&](Layout& c) { profile_sets_stage(c, n, d, P, C, nb + 256); });
    CHECK(more - bytes <= 256 * profile_sets_row_bytes(P) + 7 * 256);
    char* base = static_cast<char*>(std::aligned_alloc(256, bytes + 256));
    Layout real(base);
    const ProfileSetsStage s = profile_sets_stage(real, n, d, P, C, nb);
    CHECK(real.off == bytes);
    const std::vector<R> r = {{(char*)s.Xs, 8 * (size_t)C * n * d}, {(char*)s.ys, 8 * (size_t)C * n}, {(char*)s.set, 4 * (size_t)nb},
                              {(char*)s.params, 8 * (size_t)nb * P}, {(char*)s.grad, 8 * (size_t)nb * P},
                              {(char*)s.loglik, 8 * (size_t)nb}, {(char*)s.s2hat, 8 * (size_t)nb}, {(char*)s.beta, 8 * (size_t)nb},
                              {(char*)s.status, 4 * (size_t)nb}};
    check_tiling(base, bytes, r);
    for (int first = 1; first >= 0; --first) {
      const std::vector<Piece> in = s.inputs(first, hX.data(), hy.data(), hset.data(), hp.data(), nb);
      CHECK(in.size() == 4);
      for (int i = 0; i < 4; ++i) CHECK(in[i].dev == r[i].p && in[i].bytes == r[i].b);
      CHECK((in[0].host != nullptr) == (first == 1) && (in[1].host != nullptr) == (first == 1) && in[2].host && in[3].host);
      const Span up = span_of(in);   // a later chunk moves its rows only
      CHECK(up.lo == (first ? (char*)s.Xs : (char*)s.set) && up.lo + up.bytes == (char*)s.params + 8 * (size_t)nb * P);
    }
    const std::vector<Piece> out = s.results(o.data(), o.data(), o.data(), o.data(), nb);
    CHECK(out.size() == 4);
    for (int i = 0; i < 4; ++i) CHECK(out[i].dev == r[4 + i].p && out[i].bytes == r[4 + i].b);
    CHECK((char*)s.status >= (char*)s.beta + 8 * (size_t)nb);   // pull_status reads the status words behind beta
    std::free(base);
  }
  {
    const size_t PC = 2 * (size_t)d + 2;
    const size_t bytes = layout_bytes([&](Layout& c) { cgp_sets_stage(c, n, d, C, nb); });
    Layout plan;
    const CgpSetsStage p = cgp_sets_stage(plan, n, d, C, nb);
    CHECK(!p.Xs && !p.ys && !p.set && !p.skip && !p.params && !p.val && !p.beta && !p.tau2 && !p.loo && !p.status && plan.off == bytes);
    const size_t more = layout_bytes([&](Layout& c) { cgp_sets_stage(c, n, d, C, nb + 256); });
    CHECK(more - bytes <= 256 * cgp_sets_row_bytes(d) + 8 * 256);
    char* base = static_cast<char*>(std::aligned_alloc(256, bytes + 256));
    Layout real(base);
    const CgpSetsStage s = cgp_sets_stage(real, n, d, C, nb);
    CHECK(real.off == bytes && s.P == PC);
    const std::vector<R> r = {{(char*)s.Xs, 8 * (size_t)C * n * d}, {(char*)s.ys, 8 * (size_t)C * n}, {(char*)s.set, 4 * (size_t)nb},
                              {(char*)s.skip, 4 * (size_t)nb}, {(char*)s.params, 8 * (size_t)nb * PC}, {(char*)s.val, 8 * (size_t)nb},
                              {(char*)s.beta, 8 * (size_t)nb}, {(char*)s.tau2, 8 * (size_t)nb}, {(char*)s.loo, 8 * (size_t)nb},
                              {(char*)s.status, 4 * (size_t)nb}};
    check_tiling(base, bytes, r);
    for (int first = 1; first >= 0; --first) {
      const std::vector<Piece> in = s.inputs(first, hX.data(), hy.data(), hset.data(), hskip.data(), hp.data(), nb);
      CHECK(in.size() == 5);
      for (int i = 0; i < 5; ++i) CHECK(in[i].dev == r[i].p && in[i].bytes == r[i].b);
      CHECK((in[0].host != nullptr) == (first == 1) && (in[1].host != nullptr) == (first == 1));
    }
    const std::vector<Piece> noskip = s.inputs(true, hX.data(), hy.data(), hset.data(), nullptr, hp.data(), nb);
    CHECK(noskip[3].host == nullptr);                            // push skips it
    const std::vector<Piece> out = s.results(o.data(), o.data(), o.data(), o.data(), nb);
    CHECK(out.size() == 4);
    for (int i = 0; i < 4; ++i) CHECK(out[i].dev == r[5 + i].p && out[i].bytes == r[5 + i].b);
    CHECK((char*)s.status >= (char*)s.loo + 8 * (size_t)nb);
    std::free(base);
  }
}

int main() {
  long reg = 0, grouped = 0, lds_fallback = 0;
  for (int n = 1; n <= 129; ++n)
    for (int d = 1; d <= kMaxD; ++d)
      for (int K = 1; K <= kMaxK; ++K) {
        g_n = n; g_d = d; g_K = K;
        const bool tier = n <= 128 && fits(lds_tier_by_hand(n, d));
        const bool want = tier && fits(grad_by_hand(n, d, K));
        if (tier && !want) ++lds_fallback;   // the in-LDS gradient serves these: they go set by set
        CHECK(small_reg_profile_grad_sets_supported(n, d, K) == want);
        for (int family = 0; family < 3; ++family) {
          const Route r = small_route_profile_grad_sets(family == 0, n, d, K);
          CHECK(r == (family == 0 && want ? Route::Reg : Route::Blocked));
          (r == Route::Reg ? reg : grouped)++;
        }
        if (!want) continue;
        // the one-launch route exists exactly where the single-set gradient takes the same instance
        CHECK(small_route(Op::Grad, true, n, d, K) == Route::Reg);
        const int NB = (n + 15) / 16;
        CHECK(NB >= 1 && NB <= 8);                                   // dispatch_inv has the instance
        // what launch_inv asks for: no design copy (x_stride == 0), one matrix per workgroup
        const RegCarve cv(16, NB, NB + 1, true, false, n, d, K);
        CHECK(cv.total == grad_by_hand(n, d, K) && reg_lds_doubles(16, NB, NB + 1, true, false, n, d, K) == cv.total);
        CHECK(cv.xs + d * n == cv.mat0 && (size_t)cv.mat0 + cv.per_mat == cv.total && (size_t)cv.xs_own == cv.total);
        CHECK((cv.mat0 + cv.zmat) % 2 == 0);                         // ds_read_b128 on zmat
      }
  for (int n : {1, 5, 50, 128})
    for (int d : {1, 9, 21})
      for (int K : {1, 2, kMaxK})
        for (int C : {1, 9, 100})
          for (int nb : {1, 7, 75, 4097}) check_stages(n, d, K, C, nb);
  std::printf("reg %ld grouped %ld lds_fallback %ld\n", reg, grouped, lds_fallback);
  // the dynamic LDS total in bytes of the eight new instances at their witness shapes (n, d, K): NB = 1 .. 8
  const int pins[8][3] = {{5, 1, 1}, {17, 2, 1}, {48, 4, 2}, {50, 9, 1}, {80, 3, 2}, {96, 2, 3}, {105, 2, 2}, {128, 3, 3}};
  std::printf("lds");
  for (const auto& p : pins) std::printf(" %zu", 8 * reg_lds_doubles(16, (p[0] + 15) / 16, (p[0] + 15) / 16 + 1, true, false, p[0], p[1], p[2]));
  std::printf("\nok\n");
  return 0;
}
