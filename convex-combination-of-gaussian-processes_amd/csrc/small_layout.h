// LDS carves of the small-n evaluators (small_reg.hip, small.hip), each declared ONCE: the kernel takes its pointers from the
// carve's offsets, the launcher its dynamic LDS size from the carve's `total`, and the routing predicates of capi.hip ask
// whether `total` fits.  Plain C++ (no HIP include) so that a CPU test (tests/host_small/) runs the same declarations over
// every shape the entry points accept.  All offsets (from the start of LDS) and totals are in doubles.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define CCGP_HD __host__ __device__
#else
#define CCGP_HD
#endif

// which exp the small-n evaluators use: 0 = polynomial, 1 = table in LDS (A/B: -DCCGP_SMALL_EXP_TABLE=1)
#ifndef CCGP_SMALL_EXP_TABLE
#define CCGP_SMALL_EXP_TABLE 0
#endif

namespace ccgp {

constexpr int kSmallMaxN = 128;  // the small-n evaluators take no more rows; which call they serve below it: small_route (foot of this file)
constexpr int kMaxD = 64;        // input dimensions supported by the covariance kernels
constexpr int kMaxK = 8;         // component GPs per draw
constexpr int kLdsBytes = 160 * 1024;
constexpr int kExpTableDoubles = 256;
constexpr int kSmallExpTable = CCGP_SMALL_EXP_TABLE ? kExpTableDoubles : 0;

// does a carve fit the dynamic-LDS ceiling (raise_lds_limit) of per_cu workgroups on a CU?
CCGP_HD constexpr bool lds_fits(size_t total, int per_cu = 1) { return sizeof(double) * total <= (size_t)kLdsBytes / per_cu - 64; }

// ---- the factor a prediction keeps, in HBM (small_reg.hip) -------------------------------------------------------------
//   hdr[8]: beta, s11, bad, sw, Q | rd[NPF] | zy[NPF] | z1[NPF] | L'
// L' in HBM: column-major packed (column k = rows k + 1 .. n - 1, contiguous: the elimination writes a column per step,
// coalesced); site_solve_kernel re-lays it in LDS by row blocks of eight (lrect / ltri below).
CCGP_HD constexpr int fac_npf(int n) { return (n + 7) / 8 * 8; }
CCGP_HD constexpr int fac_col(int n, int k) { return k * (n - 1) - k * (k - 1) / 2; }   // first entry (row k + 1) of column k
struct FacLayout {
  int npf, rd, zy, z1, L, head, total;
  CCGP_HD FacLayout(int n) {
    npf = fac_npf(n);
    rd = 8; zy = rd + npf; z1 = zy + npf; L = z1 + npf; head = L; total = (L + n * (n - 1) / 2 + 7) / 8 * 8;
  }
};
// LDS image of L' for the blocked forward substitution: row block I (rows 8 I .. 8 I + 7) holds first its rectangle -- columns
// k < 8 I, each column as the block's 8 row entries side by side (one FMA per row and column, eight independent chains, the
// operands of a column in four ds_read_b128) -- then its 8 x 8 triangle row by row (row j: its j entries).
// (block I starts at sum_{J<I} (64 J + 32) = 32 I^2 words)
CCGP_HD constexpr int lrect(int I, int k, int j) { return 32 * I * I + k * 8 + j; }
CCGP_HD constexpr int ltri(int I, int j, int c) { return 32 * I * I + 64 * I + j * (j - 1) / 2 + c; }

// ---- small_reg_kernel<G, NB, NE, ., INV> -----------------------------------------------------------------------------
//   etab | xs[d][n] | 256 / G^2 matrices of per_mat words | xt[d][G NE] (NE > 1) | one xs[d][n] per matrix (per-design, and
//   the sets form on the 8 x 8 grid; on the 16 x 16 grid the sets form's one matrix reads its set's design from the shared xs)
// (the inverse / gradient instances run one matrix per workgroup, so zmat's bump depends on nothing but the shape)
// one matrix:  us[K][NP] | th[K][d] | w2[K] | colbuf[2][NP + G NE] | dvec[NP] | zb[2][NP] | slack[8] | tail
//   tail, prediction (NE > 1): ut[K][G NE] | psum[3][G NE][G]
//   tail, inverse / gradients: zmat[NP][NP + 2] behind a one-word bump to 16 bytes | part[4][kGradSlots]
// Sized from the ACTUAL number of components and dimensions (round 3: sized for kMaxK / kMaxD before -- 4 KB of th[] per
// matrix for a 2 x 4 table -- which left the prediction instances one workgroup per CU short).
constexpr int kGradSlots = 28;   // accumulators of one pass of the gradient contraction: QG (1 + KG) <= 27
struct RegCarve {
  int etab, xs, mat0, per_mat, xt, xs_own;                          // from the start of LDS; mat0, xs_own: matrix 0's
  int us, th, w2, colbuf, dvec, zb, slack, ut, psum, zmat, part;   // from the start of a matrix's block, mat0 + sub per_mat
  size_t total;
  CCGP_HD RegCarve(int G, int NB, int NE, bool inv, bool per_design, int n, int d, int K) {
    const int NP = G * NB, XR = G * NE, MPW = 256 / (G * G);
    etab = 0;                          // 2^(j/256) for exp_cov, shared by the workgroup
    xs = kSmallExpTable;               // d x n, shared by the matrices of this workgroup
    mat0 = xs + d * n;
    us = 0;
    th = us + K * NP;
    w2 = th + K * d;
    colbuf = w2 + K;                   // [2][NP + XR]
    dvec = colbuf + 2 * (NP + XR);
    zb = dvec + NP;                    // [2][NP]
    slack = zb + 2 * NP;               // [8]: beta, 1'R^-1 1 for the epilogues, cs_hat (PROF), Q (prediction)
    const int tail = slack + 8;
    ut = tail;                         // [K][XR]    (prediction)
    psum = ut + K * XR;                // [3][XR][G] (prediction)
    // [NP][NP + 2] (inv): row t = L'^-1 e_t, columns scaled by d_c^-1/2; read two doubles at a time (ds_read_b128), and one
    // matrix per workgroup there, so the block starts at mat0
    zmat = tail + ((mat0 + tail) & 1);
    part = zmat + NP * (NP + 2);       // [4][kGradSlots] wave partial sums of the gradient
    per_mat = tail + (inv ? NP * (NP + 2) + 1 + 4 * kGradSlots : (NE > 1 ? K * XR + 3 * XR * G : 0));
    xt = mat0 + MPW * per_mat;         // [d][XR], shared by the workgroup (prediction)
    xs_own = xt + (NE > 1 && !inv ? d * XR : 0);   // per-design: matrix sub keeps its own copy at xs_own + sub d n
    total = (size_t)xs_own + (per_design ? (size_t)MPW * d * n : 0);
  }
};
inline size_t reg_lds_doubles(int G, int NB, int NE, bool inv, bool per_design, int n, int d, int K) {
  return RegCarve(G, NB, NE, inv, per_design, n, d, K).total;
}
constexpr int kPredictNE = 4;   // extra row-blocks of the prediction instances: 30 (G = 8) / 62 (G = 16) sites per chunk
// the 8 x 8 grid with up to 13 x 13 blocks per thread, four matrices per workgroup (64 < n <= 104, the likelihood)
inline bool small_reg_fits8(int n, int d, int K, bool per_design) {
  return lds_fits(reg_lds_doubles(8, (n + 7) / 8, 1, false, per_design, n, d, K));
}

// ---- site_corr_kernel<K>, `waves` batches of 64 test sites:  th[K][d] up to 8 | w2[8] | us[K][npf] | xs[K][d][npf] | xw[waves][d][64]
struct SiteCorrCarve {
  int th, w2, us, xs, xw;
  size_t total;
  CCGP_HD SiteCorrCarve(int npf /* fac_npf(n) */, int d, int K, int waves) {
    th = 0;
    w2 = th + (K * d + 7) / 8 * 8;
    us = w2 + 8;
    xs = us + K * npf;
    xw = xs + K * d * npf;                     // wave w's test sites: xw + w d 64, [k][lane]
    total = (size_t)xw + (size_t)waves * d * 64;
  }
};
// ---- site_solve_kernel<fac_npf(n)>:  F: the factor block's head as it is in HBM | L' in row blocks of 8 (lrect / ltri) | slack[8]
struct SiteSolveCarve {
  int F, L;
  size_t total;
  CCGP_HD SiteSolveCarve(int n) {
    const int nbl = fac_npf(n) / 8;
    F = 0;
    L = FacLayout(n).head;
    total = (size_t)L + 32 * nbl * nbl + 8;
  }
};

// ---- small_kernel, mtile unit rows per workgroup:
//   A[n + 2 + mtile][n] | xs[d][n] | us[K][n] | reserved[(d + K) mtile] | th[K][d] | w2[K] | red[16] | etab[256]
// The reserved words held the test sites of the in-LDS prediction, which the register scheme replaced; they stay in the
// size because mtile is picked from it and the chunking of the gradient (hence its bits) and the routes follow from mtile.
// The host sizes for K = kMaxK; the kernel carves with its own K, which ends no later.
struct SmallCarve {
  int A, xs, us, reserved, th, w2, red, etab;
  size_t total;
  CCGP_HD SmallCarve(int n, int d, int K, int mtile) {
    A = 0;
    xs = A + (n + 2 + mtile) * n;
    us = xs + d * n;
    reserved = us + K * n;
    th = reserved + d * mtile + K * mtile;
    w2 = th + K * d;
    red = w2 + K;
    etab = red + 16;                           // 2^(j/256) for exp_cov
    total = (size_t)etab + kExpTableDoubles;
  }
};
inline size_t small_lds_bytes(int n, int d, int mtile) { return sizeof(double) * SmallCarve(n, d, kMaxK, mtile).total; }
inline int small_pick_mtile(int n, int d, int m) {
  const size_t budget = 150 * 1024;
  int mt = m < 1 ? 1 : m;
  if (mt > 256) mt = 256;
  while (mt > 1 && small_lds_bytes(n, d, mt) > budget) --mt;
  return mt;
}

// ---- does an instance fit: the building blocks of small_route below ---------------------------------------------------
// the register-resident evaluator: likelihood, log det of per-design matrices, prediction by the extra-row scheme
inline bool small_reg_supported(int n, int d, int K, bool per_design = false, bool predict = false) {
  if (n > 128) return false;
  const int G = n <= 64 ? 8 : 16;
  return lds_fits(reg_lds_doubles(G, (n + G - 1) / G, predict ? kPredictNE : 1, false, per_design, n, d, K));
}
// kept-factor prediction (round 5; else the extra-row scheme of rounds 2 - 4): the factorising instance on the 8 x 8 grid
// and two workgroups per CU of each site kernel
inline bool small_reg_sites_supported(int n, int d, int K) {
  if (n > 104 || K > 3) return false;
  return small_reg_fits8(n, d, K, false) && lds_fits(SiteSolveCarve(n).total, 2) &&
         lds_fits(SiteCorrCarve(fac_npf(n), d, K, 4).total, 2);
}
// scratch per draw (bytes): the factor block + the correlation vectors of its ceil(m / 64) site batches
inline size_t small_reg_sites_scratch(int n, int d, int K, int m) {
  (void)d; (void)K;
  return sizeof(double) * ((size_t)FacLayout(n).total + (size_t)((m + 63) / 64) * fac_npf(n) * 64);
}
// solve(R) of one draw and the analytic gradient (INV = 1, 2); the design gradient (INV = 3) keeps its design behind the matrix
inline bool small_reg_inverse_supported(int n, int d, int K, bool per_design = false) {
  if (n > 128) return false;
  const int NB = (n + 15) / 16;
  return lds_fits(reg_lds_doubles(16, NB, NB + 1, true, per_design, n, d, K));
}
inline bool small_reg_design_grad_supported(int n, int d, int K) { return small_reg_inverse_supported(n, d, K, true); }

// ---- which tier serves which call: decided HERE, once per call (capi.hip branches on the result) ------------------------
//   Reg      the register-resident evaluator (small_reg.hip)
//   Lds      the in-LDS evaluator (small.hip): the gradient and solve(R) of shapes whose INV instance does not fit
//   Blocked  the blocked sweep over materialised matrices (cov.hip + blocked.hip): any n, any kernel family
// `gauss`: the Gaussian family; the others exist on the blocked sweep only (but see small_family_fused_supported at the foot of
// this file: under CCGP_OPT_FAMILY_FUSED the caller sets the flag for a 1-D family too).  Grad, LogdetDesigns and DesignGrad refuse them
// before they ask (Grad: but for a 1-D family under CCGP_OPT_FAMILY_FUSED_GRAD, small_family_fused_grad_supported at the foot of
// this file, whose domain lies inside Grad's Reg cell), so their routes do not look at it.  For Grad the caller turns Blocked into a refusal when the
// contraction kernel cannot take (d, K) (blocked_grad_supported, blocked.hip).
// What is decided after the route, from more than the shape, stays with its owner: kept-factor or extra-row prediction
// (capi.hip: option, small_reg_sites_supported, scratch), the grid of an instance (small_reg.hip: dispatch), the sweep's
// schedule (blocked.hip).  tests/host_small/small_layout_check.cpp holds this function, shape by shape, to the expressions
// it replaced and prints the table; tests/test_gpu_routes.py runs one shape of every cell.
enum class Op { Loglik, Predict, Inverse, Grad, LogdetDesigns, DesignGrad };
enum class Route { Reg, Lds, Blocked, Unsupported };
// where small.hip's one-row carve fits: the Lds tier's domain
inline bool small_lds_tier(int n, int d) { return n <= kSmallMaxN && lds_fits(SmallCarve(n, d, kMaxK, 1).total); }
// Op::Inverse without its Reg route: what ccgp_logpost falls back to when that route's pinned host buffer cannot be had
inline Route small_route_inverse_staged(bool gauss, int n, int d) {
  return gauss && small_lds_tier(n, d) ? Route::Lds : Route::Blocked;
}
inline Route small_route(Op op, bool gauss, int n, int d, int K) {
  const bool lds_tier = small_lds_tier(n, d);
  switch (op) {
    case Op::Loglik:
      return gauss && small_reg_supported(n, d, K) ? Route::Reg : Route::Blocked;
    case Op::Predict:
      // lds_tier is a frozen legacy boundary (the in-LDS prediction that used to sit between the two is gone): every shape
      // inside it has its register instance (the check program's `dead` line), and so have the 4216 shapes of n <= 128
      // outside it (its `predict_outside_lds`), which the blocked sweep keeps serving until the boundary is moved
      return gauss && lds_tier && small_reg_supported(n, d, K, false, true) ? Route::Reg : Route::Blocked;
    case Op::Inverse:
      return gauss && small_reg_inverse_supported(n, d, K) ? Route::Reg : small_route_inverse_staged(gauss, n, d);
    case Op::Grad:
      if (!lds_tier) return Route::Blocked;
      return small_reg_inverse_supported(n, d, K) ? Route::Reg : Route::Lds;
    case Op::LogdetDesigns:
      return small_reg_supported(n, d, K, true) ? Route::Reg : Route::Blocked;
    case Op::DesignGrad:
      return small_reg_design_grad_supported(n, d, K) ? Route::Reg : Route::Unsupported;
  }
  return Route::Unsupported;
}
// leave-one-out tables (ccgp_loo_batch, ccgp_loo_summary): the fourth inverse instance (INV = 4) on the carve of the other
// three where it fits, else identity rows on the blocked sweep -- which is every family but the Gaussian.  A function of its
// own, not an Op: the check program switches over Op and holds each of its cells to the expression it replaced.
inline Route small_route_loo(bool gauss, int n, int d, int K) {
  return gauss && small_reg_inverse_supported(n, d, K) ? Route::Reg : Route::Blocked;
}
// the sets form of the likelihood (ccgp_loglik_batch_sets, ccgp_logpost_sets): C training sets of one shape, row b on set
// set[b].  Which grid a call of B rows takes: at most 64 rows are a latency problem and run four waves per matrix on the
// 16 x 16 grid (one matrix per workgroup: the set's design lies in the shared xs slot); a larger call runs one wave per
// matrix on the 8 x 8 grid with a design copy per matrix (RegCarve::xs_own) up to 13 x 13 blocks where that carve fits, and
// stays on the 16 x 16 grid beyond.  The two grids give the same bits, so the choice is one of speed only.
inline int small_reg_sets_grid(int n, int d, int K, int B) {
  if (B <= 64 || n > 104) return 16;
  return small_reg_fits8(n, d, K, true) ? 8 : 16;
}
// both carves a call may need: the 16 x 16 grid's for any B, and at n <= 64 the 8 x 8 grid's with four designs (above 64
// a large call falls back to the 16 x 16 grid where the 8 x 8 carve does not fit)
inline bool small_reg_sets_supported(int n, int d, int K) {
  if (n > kSmallMaxN) return false;
  if (!lds_fits(reg_lds_doubles(16, (n + 15) / 16, 1, false, false, n, d, K))) return false;
  return n > 64 || small_reg_fits8(n, d, K, true);
}
// Reg: one launch of the sets instances.  Blocked: the host groups the rows by set and runs each group through the
// single-set call (whatever route that call takes), which covers n > 128 and the Matern and spline families.
inline Route small_route_sets(bool gauss, int n, int d, int K) {
  return gauss && small_reg_sets_supported(n, d, K) ? Route::Reg : Route::Blocked;
}
// The predictions over sets (ccgp_predict_batch_sets, ccgp_krige_predict_batch_sets, ccgp_predict_summary_sets).  Reg: ONE set
// of launches per chunk of rows for all sets -- the factor-keeping sets instance (FAC + SETS), site_corr_kernel<K, true> with a
// set per row, site_solve_kernel, and for the summary the (site, set) grids of summary.hip -- exactly where the single-set
// call takes the kept-factor scheme on the Gaussian family (small_reg_sites_supported: n <= 104, K <= 3) and the sets
// instance's carve fits (on the 8 x 8 grid it keeps a design per matrix).  capi.hip adds what only the handle knows:
// CCGP_OPT_PREDICT_FACTOR and whether the scratch could be had.  Blocked: the rows are grouped by set and every group goes
// through the single-set launches, whatever route they take (105 <= n <= 128, K > 3, n > 128, the Matern and spline families
// with or without option 12).  The kept-factor and extra-row schemes have the same bits, so the contract does not depend on it.
inline Route small_route_predict_sets(bool gauss, int n, int d, int K) {
  return gauss && small_reg_sites_supported(n, d, K) && small_reg_sets_supported(n, d, K) ? Route::Reg : Route::Blocked;
}
// Metropolis chains on the device (ccgp_metro_segments_sets): the CHAIN instances are the sets likelihood instances of the
// 16 x 16 grid, one workgroup per chain, with the chain's own words behind the instance's carve: the two 256-entry tables
// of the portable exp (chain_terms.h), state, candidate, l / ljac / lprior / beta, and the two words of the decision (go on, accepted)
// that the whole workgroup reads after its barrier
constexpr int kChainLdsDoubles = 2 * 256 + 4 + 4 + 4 + 2;
inline size_t reg_chain_lds_doubles(int NB, int n, int d, int K) {
  return reg_lds_doubles(16, NB, 1, false, false, n, d, K) + kChainLdsDoubles;
}
// Reg exactly where the sets likelihood has its one-launch route and the chain's words fit beside the carve; Unsupported
// otherwise (n > 128, Matern and spline, a carve that does not fit): the caller keeps the chain on the host there
inline Route small_route_chain(bool gauss, int n, int d, int K) {
  if (small_route_sets(gauss, n, d, K) != Route::Reg) return Route::Unsupported;
  return lds_fits(reg_chain_lds_doubles((n + 15) / 16, n, d, K)) ? Route::Reg : Route::Unsupported;
}
// the sets form of the profiled gradient (ccgp_profile_batch_sets with out_grad): the INV = 2 instances on the 16 x 16 grid,
// one matrix per workgroup with its set's design in the shared xs slot -- the carve of the single-set instance, so the sets
// form exists exactly where ccgp_profile_batch's gradient takes the Reg route (the in-LDS and blocked routes have no sets
// form: their rows go set by set)
inline bool small_reg_profile_grad_sets_supported(int n, int d, int K) {
  return small_route(Op::Grad, true, n, d, K) == Route::Reg;
}
inline Route small_route_profile_grad_sets(bool gauss, int n, int d, int K) {
  return gauss && small_reg_profile_grad_sets_supported(n, d, K) ? Route::Reg : Route::Blocked;
}
// the ordinary-kriging fits on the device (ccgp_profile_fit_sets): the FIT instances are the profiled-gradient sets instances,
// one workgroup per start, K = 1, with the start's own words behind the instance's carve: the two 256-entry tables of the
// portable exp (chain_terms.h), the word the whole workgroup reads after its barrier (go on / leave), the likelihood, the
// gradient row (kMaxD words) and the start's state (fit_logic.h: 16 + 16 d doubles)
constexpr int kFitLdsHead = 2 * 256 + 2 + kMaxD;
CCGP_HD constexpr int fit_state_words(int d) { return 16 + 16 * d; }
inline size_t reg_fit_lds_doubles(int NB, int n, int d) {
  return reg_lds_doubles(16, NB, NB + 1, true, false, n, d, 1) + kFitLdsHead + fit_state_words(d);
}
// Reg exactly where the sets form of the profiled gradient has its one-launch route and the start's words fit beside the
// carve; Unsupported otherwise (n > 128, Matern and spline, K != 1, a carve that does not fit): the caller keeps the fit on
// the host twin there
inline Route small_route_fit(bool gauss, int n, int d, int K) {
  if (K != 1 || small_route_profile_grad_sets(gauss, n, d, K) != Route::Reg) return Route::Unsupported;
  return lds_fits(reg_fit_lds_doubles((n + 15) / 16, n, d)) ? Route::Reg : Route::Unsupported;
}
// the Laplace search on the device (ccgp_laplace_search_sets): the NM instances are the CHAIN instances with a Nelder-Mead
// search in place of the Metropolis walk, one workgroup per search.  The search's state (nm_logic.h: q^2 + 5 q + 18 doubles,
// q = 3 or 4 for the priors a chain has) lies behind the chain's words, of which the search uses the tables, ljac / lprior
// and the decision word
constexpr int kNmLdsQ = 4;
CCGP_HD constexpr int nm_state_words(int q) { return q * q + 5 * q + 18; }
inline size_t reg_nm_lds_doubles(int NB, int n, int d, int K) {
  return reg_chain_lds_doubles(NB, n, d, K) + nm_state_words(kNmLdsQ);
}
// Reg exactly where small_route_chain says Reg and the search's words fit behind the chain's; Unsupported otherwise: the
// caller keeps the search on the host twin there
inline Route small_route_nm(bool gauss, int n, int d, int K) {
  if (small_route_chain(gauss, n, d, K) != Route::Reg) return Route::Unsupported;
  return lds_fits(reg_nm_lds_doubles((n + 15) / 16, n, d, K)) ? Route::Reg : Route::Unsupported;
}
// the 1-D families on the register-resident evaluator (CCGP_OPT_FAMILY_FUSED, ccgp.h): the FAM instances of small_reg.hip
// generate a Matern (family 1) or Matern + spline (family 2: K = 2, as ccgp_set_kernel's callers enforce) matrix from the one
// coordinate in xs, for the plain likelihood with or without SETS / CHAIN / NM.  They are compiled for the reference's own
// shapes, d = 1 and n <= 32 (its designs have 8 points): two blocks of the 16 x 16 grid, four of the 8 x 8.  The four route
// functions above keep their `gauss` flag; where the option is on, capi.hip passes `gauss || small_family_fused_supported(..)`
// for Op::Loglik, small_route_sets, small_route_chain and small_route_nm, and nothing else.  The carves asked for are those
// of all four, so a shape inside this domain is Reg on each (tests/host_small/family_fused_layout_check.cpp).
constexpr int kFamilyFusedMaxN = 32;
inline bool small_family_fused_supported(int family, int n, int d, int K) {
  if ((family != 1 && family != 2) || d != 1 || n < 1 || n > kFamilyFusedMaxN) return false;
  if (K < 1 || K > kMaxK || (family == 2 && K != 2)) return false;
  return small_reg_supported(n, d, K) && small_reg_sets_supported(n, d, K) && lds_fits(reg_nm_lds_doubles((n + 15) / 16, n, d, K));
}
// prediction and leave-one-out of the 1-D families on the same evaluator (CCGP_OPT_FAMILY_FUSED_PREDICT, an option of its
// own: option 11 keeps moving exactly what it moved).  Prediction has the kept-factor scheme only -- the FAM instances that
// keep their factor (FAC), site_corr_family_kernel for the test sites' correlation vectors and site_solve_kernel as it is --
// so its domain is the likelihood's cut by small_reg_sites_supported (K <= 3); no FAM instance carries extra rows.
// Leave-one-out is the fourth inverse instance (INV = 4) compiled with FAM, on the carve of the other inverse instances; a
// fold needs another point.  capi.hip passes `gauss || (option && these)` to small_route(Op::Predict) -- together with
// CCGP_OPT_PREDICT_FACTOR, without which a family stays on the sweep -- and to small_route_loo, and nothing else: both are Reg
// there (tests/host_small/family_fused_predict_layout_check.cpp).
inline bool small_family_fused_predict_supported(int family, int n, int d, int K) {
  return small_family_fused_supported(family, n, d, K) && small_reg_sites_supported(n, d, K);
}
inline bool small_family_fused_loo_supported(int family, int n, int d, int K) {
  return small_family_fused_supported(family, n, d, K) && small_reg_inverse_supported(n, d, K) && n >= 2;
}
// the profiled mode and the analytic gradient of the 1-D families on the same evaluator (CCGP_OPT_FAMILY_FUSED_GRAD, an option
// of its own: options 11 and 12 keep moving exactly what they moved).  The value-only profiled call is the likelihood
// instance compiled with FAM + PROF, so its domain is the likelihood's; the gradient -- plain, profiled, profiled over sets --
// is the INV = 2 instance compiled with FAM on the carve of the other inverse instances.  capi.hip passes
// `gauss || (option && these)` where grad_call and grad_run decide Op::Grad / Op::Loglik for ccgp_loglik_grad_batch and
// ccgp_profile_batch and to small_route_profile_grad_sets, and nothing else: all three are Reg there
// (tests/host_small/family_fused_grad_layout_check.cpp).
inline bool small_family_fused_profile_supported(int family, int n, int d, int K) {
  return small_family_fused_supported(family, n, d, K);
}
inline bool small_family_fused_grad_supported(int family, int n, int d, int K) {
  return small_family_fused_supported(family, n, d, K) && small_reg_inverse_supported(n, 1, K);
}

// the maximum-entropy design search on the device (ccgp_design_fit): the DFIT instances are the design-gradient instances
// (INV = 3, per-design carve), one workgroup per start.  A start's variables are the free rows of its design in the order
// numpy ravels [n - n_fixed, d]: nv = (n - n_fixed) d, variable v = i d + k is free row i, dimension k.  Nothing is
// transformed between the iterate and the design, so there are no exp tables: the start's words behind the carve are
//   go | ld | grad[nv] | state[fit_state_words(nv)]
// (go: the word the whole workgroup reads after its barrier), sized from the actual nv
inline size_t reg_design_fit_lds_doubles(int NB, int n, int d, int K, int nv) {
  return reg_lds_doubles(16, NB, NB + 1, true, true, n, d, K) + 2 + nv + fit_state_words(nv);
}
// Reg exactly where the design gradient has its route, the start is one the stepper takes (1 <= nv <= kMaxD: its state and
// fit_sum's stated order end there) and the words fit; Unsupported otherwise: the caller keeps the search on the host twin
inline Route small_route_design_fit(bool gauss, int n, int d, int K, int n_fixed) {
  if (!gauss || n_fixed < 0 || n_fixed >= n || small_route(Op::DesignGrad, gauss, n, d, K) != Route::Reg) return Route::Unsupported;
  const long long nv = (long long)(n - n_fixed) * d;
  if (nv < 1 || nv > kMaxD) return Route::Unsupported;
  return lds_fits(reg_design_fit_lds_doubles((n + 15) / 16, n, d, K, (int)nv)) ? Route::Reg : Route::Unsupported;
}

}  // namespace ccgp
