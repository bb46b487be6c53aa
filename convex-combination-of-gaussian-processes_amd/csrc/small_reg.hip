// Register-resident fused evaluator for the plain likelihood at n <= 128 (BASELINE configs 2
// and 3: the hyperprior grids, HX:549-595 / ADV:552-599; and the likelihood term of logpost).
//
// A G x G grid of threads owns ONE matrix 2-D cyclically in registers: thread (ty, tx) holds
// entries (ty + G a, tx + G b), a >= b, plus one block row of right-hand sides (row ty = 0 is
// y', row ty = 1 is 1').  The covariance is generated straight into those registers (never in
// HBM, never in LDS), then eliminated as L' D L'^T: per column, the owning threads publish the
// column through a 2 x (n + G)-word LDS buffer and every thread applies its rank-1 update on
// registers.  The right-hand-side row is updated like any other row, so the forward
// substitutions come for free (same scheme as small.hip, which keeps the matrix in LDS and
// also serves prediction / inverse / gradient).
//   G = 8 : one WAVE per matrix, no s_barrier at all (LDS traffic of one wave is ordered), four
//           matrices per workgroup -- n <= 64 (Heat-Exchanger grid, n = 64)
//   G = 16: one workgroup per matrix, one barrier per column -- 64 < n <= 128
// NB = ceil(n / G) is a template parameter so that every register index is static.
// INV (round 3, G = 16, NE = NB + 1): the extra rows are the IDENTITY -- solve(R) of logpost (HX:454), one matrix per
// call: Metro's sequential caller.  After the sweep row t holds z_t = L'^-1 e_t; Z goes to LDS and
// R^-1 = Z' D^-1 Z is formed by all 256 threads (the in-LDS kernel of small.hip back-substituted one row per
// thread: 208 us per call at n = 64 against ~50 here).
// NE = number of G-row blocks of EXTRA rows: NE = 1 is the plain likelihood (rows y', 1');
// NE = 4 serves prediction (predict.post, HX:655-673): rows 2.. of the extra block are the
// cross-correlations r(x_t)' of a chunk of G NE - 2 test sites, eliminated like every other row,
// so that afterwards they hold L'^-1 r(x_t) and mean / variance are D-weighted dot products.
//
// Bound: neither HBM nor MFMA -- n dependent elimination steps; algorithmic HBM traffic per
// evaluation is the parameter row in (8 P bytes) and 20 bytes out.
#include <algorithm>
#include <type_traits>

#include "ccgp_internal.h"
#include "chain_terms.h"
#include "fit_logic.h"
#include "nm_logic.h"

namespace ccgp {

namespace {

// the two tables of chain_exp (chain_terms.h) for the chain instances, which copy them to LDS once
static __device__ const unsigned long long kChainExpLoBits[kChainTable] = CCGP_CHAIN_EXP_LO_BITS;

// the chain's words behind the instance's carve: hi[256] | lo[256] | theta[4] | cand[4] | l, ljac, lprior, beta | go | accepted
// (the last two are the decision thread 0 publishes, 0.0 or 1.0: every word of the block is a double)
enum { kChainHi = 0, kChainLo = kChainTable, kChainTheta = 2 * kChainTable, kChainCand = kChainTheta + 4,
       kChainL = kChainCand + 4, kChainLj, kChainLp, kChainBeta, kChainGo, kChainAcc };
static_assert(kChainAcc + 1 == kChainLdsDoubles, "small_layout.h sizes the chain's words");

// The mode-0 log-likelihood of the CHAIN instances with its operations spelled out.  In the other instances the compiler
// contracts `n * kLog2Pi + n * log(cs)` to fma(log 2 pi, n, n log cs); inside the proposal loop the loop-invariant product
// n log 2 pi is hoisted out of the loop and the OTHER product would be fused -- one rounding elsewhere, 1 - 4 ulp of the value
// for every n that is no power of two.  A chain's likelihood must have the sets instance's bits, so: that instance's operations.
__device__ __forceinline__ double chain_loglik(int n, double log2pi, double log_cs, double logdet, double q_over_cs) {
#pragma clang fp contract(off)
  const double nl = n * log_cs;
  return -0.5 * ((__builtin_fma(log2pi, (double)n, nl) + logdet) + q_over_cs);
}

// the start's words of the FIT instances behind the instance's carve: hi[256] | lo[256] | go | ll | grad[kMaxD] | state[W]
// (go is the decision thread 0 publishes, 0.0 or 1.0: every word of the block is a double)
enum { kFitHi = 0, kFitLo = kChainTable, kFitGo = 2 * kChainTable, kFitLl, kFitGrad, kFitState = kFitGrad + kMaxD };
static_assert(kFitState == kFitLdsHead && fit_state_doubles(kMaxD) == fit_state_words(kMaxD) && fit_state_doubles(1) == fit_state_words(1),
              "small_layout.h sizes the start's words");
constexpr int kFitMaxEvals = 4096;   // evaluations of one start in one call (ccgp.h)

// The profiled log-likelihood of the FIT instances with its operations spelled out, for chain_loglik's reason: inside the
// evaluation loop the loop-invariant product n log 2 pi would be hoisted and the other product fused.  The operations are the
// ones the profiled instances compile to: fma(log 2 pi, n, n log cs_hat), then + log det, then + n.
__device__ __forceinline__ double fit_loglik(int n, double log2pi, double log_csh, double logdet) {
#pragma clang fp contract(off)
  const double nl = n * log_csh;
  return -0.5 * ((__builtin_fma(log2pi, (double)n, nl) + logdet) + (double)n);
}

// the search's state of the NM instances lies behind the chain's words (of which a search uses the tables, ljac, lprior and go)
enum { kNmState = kChainLdsDoubles };
static_assert(nm_state_doubles(kNmLdsQ) == nm_state_words(kNmLdsQ) && nm_state_doubles(3) == nm_state_words(3),
              "small_layout.h sizes the search's words");
constexpr int kNmMaxEvals = 4096;   // evaluations of one search in one call (ccgp.h)

// the start's words of the DFIT instances behind the instance's per-design carve: go | ld | grad[nv] | state[W(nv)]
// (small_layout.h: reg_design_fit_lds_doubles; go is the decision thread 0 publishes, 0.0 or 1.0)
enum { kDfGo = 0, kDfLd, kDfGrad };
constexpr int kDfMaxEvals = 4096;   // evaluations of one start in one call (ccgp.h)

struct RegArgs {
  const double* X;
  const double* y;
  int n, d;
  const double* params;
  int ldp, K;
  int draw0, B;
  double sigma2;
  int mode;
  double tau2;
  double* loglik;
  double* beta;
  int* status;
  // design-batched form (entropy criteria, BSQ:856-877): every evaluation has its OWN design
  // (X + b * x_stride) and all share one parameter row; only log det R_mixed is wanted
  // prediction (NE > 1): test sites, S = leading dimension of the (draw x test site) tables
  const double* Xt;
  int m, S;
  double* mean;
  double* var;
  size_t x_stride;     // 0: one shared design
  int shared_params;   // 1: params is a single row
  double* logdet;      // optional output: sum_k log d_k
  double* Rinv;        // INV = 1: n x n explicit inverse of the (normalised) mixed correlation matrix
  double* grad;        // INV = 2: d loglik / d params, Btot x P column-major (element (b, j) at grad[b + j * Btot])
  int Btot;
  int grid16;          // CCGP_OPT_SMALL_GRID16: 64 < n <= 104 on the 16 x 16 grid (measurements)
  double* fac;         // FAC instantiation: per draw a block of fac_stride doubles that keeps the factor for predict_sites_kernel
  size_t fac_stride;
  double* dgrad;       // INV = 3: d log det R / d X of the free rows, per design (n - n_fixed) x d column-major
  int n_fixed;         // INV = 3: rows below n_fixed are the fixed batch (D.old, BSQ:920-948): no gradient
  double* s2hat;       // PROF instantiations: the draw's own sigma2 = q / (n sum w^2) (sigma2.MLE, D1:411-415); `sigma2` is not read
  VarForm vf;          // prediction (NE > 1, FAC): per-draw sigma2 and Q indexed by the global draw, the variance form
  // sets form (SETS instantiations, ccgp_loglik_batch_sets): evaluation b belongs to training set set[b] and reads its design at
  // X + set[b] n d, its right-hand side at y + set[b] n and its sigma2 at sigma2_set[set[b]]; `sigma2` is not read
  // (the profiled gradient over sets, ccgp_profile_batch_sets, reads neither: sigma2_set stays null there)
  const int* set;
  const double* sigma2_set;
  ChainIO ch;          // CHAIN instantiations only
  FitIO fit;           // FIT instantiations only
  NmIO nm;             // NM instantiations only
  DesignFitIO dfit;    // DFIT instantiations only
  KernelFamily fam;    // FAM instantiations only: the handle's 1-D family (id, nu, norm); Gaussian in every other launch
};

// The 1-D families' correlation of one scaled squared distance -- corr_of_dist's family branch (ccgp_internal.h) -- as ONE
// compiled body for every FAM instance.  Inlined, matern_corr's quadrature is contracted by the compiler in each instantiation on
// its own, and a chain's or a search's likelihood must have the bits the sets instance gives that row, on either grid.  The call
// costs nothing beside ~150 terms of three exp each; every loop inside is bounded (matern_corr's 6000-term cap).
__device__ __noinline__ double family_corr(int id, double nu, double norm, double dist, int component) {
  if (id == CCGP_KERNEL_MATERN_SPLINE && component == 1) return spline_corr(dist);
  KernelFamily f;
  f.id = id; f.nu = nu; f.norm = norm;
  return matern_corr(f, dist);
}
// The component's correlation AND its derivative with respect to its own theta from one pass (spline_corr_grad /
// matern_corr_grad, ccgp_internal.h; CCGP_OPT_FAMILY_FUSED_GRAD): the body the gradient epilogue of every FAM + INV = 2 instance
// and family_dcorr_kernel call.  Not inlined for family_corr's reason: a sets row must have the single-set row's bits, and
// the entries ccgp_family_corr_dtheta returns are the ones the gradient sums.  Bounded by the 6000-term cap.
// Both come back by value (registers): a pointer to a caller's local would put the derivative through scratch.
struct CorrGrad { double r, dtheta; };
__device__ __noinline__ CorrGrad family_corr_grad(int id, double nu, double norm, double dist, double theta, int component) {
  CorrGrad o;
  if (id == CCGP_KERNEL_MATERN_SPLINE && component == 1) {
    o.r = spline_corr_grad(dist, theta, &o.dtheta);
    return o;
  }
  KernelFamily f;
  f.id = id; f.nu = nu; f.norm = norm;
  o.r = matern_corr_grad(f, dist, theta, &o.dtheta);
  return o;
}

// ccgp_family_corr_dtheta: one thread per entry (i, j) of the n x n table, no LDS, no barrier
__global__ __launch_bounds__(256) void family_dcorr_kernel(const double* x, int n, double theta, int q, KernelFamily fam,
                                                           double* out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * n) return;
  const int i = (int)(e % n), j = (int)(e / n);
  const double h = x[i] - x[j];
  out[e] = family_corr_grad(fam.id, fam.nu, fam.norm, theta_to_rate(fam, theta, q) * (h * h), theta, q).dtheta;
}

// ---- the factor a prediction keeps (round 5) ------------------------------------------------------------------------
// Rounds 2 - 4 predicted by carrying the cross-correlation rows of a CHUNK of test sites (30 at n <= 64, 62 above) through the
// elimination as extra rows, one workgroup per (draw, chunk): every chunk generated and factorised the draw's matrix again --
// five times for the 150 sites of a Ground-Vibrations test set.  Now the likelihood instantiation (NE = 1, FAC) factorises
// ONCE per draw and writes L' (unit lower), 1 / d, z'_y, z'_1, beta and 1'R^-1 1 to a block in HBM (11 KB at n = 50); beside it
// -- on a second stream, it needs nothing from the factorisation -- site_corr_kernel forms the test sites' correlation vectors
// r(x_t) with lane = test site; site_solve_kernel then does the forward substitution w' = L'^-1 r and predict.post's arithmetic,
// again lane = site, every matrix operand a broadcast LDS read.  Same operations in the same order per (draw, site) as the
// extra-row scheme, hence the same bits.
// (FacLayout, fac_col, lrect / ltri: small_layout.h, with the LDS carve of every kernel here)

template <int G>
__device__ __forceinline__ void mat_sync() {
  if constexpr (G == 16) {
    __syncthreads();
  } else {
    // one wave per matrix: its LDS operations are processed in order; only the compiler has to
    // be kept from moving the reads above the writes
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// FULL: n == G * NB exactly (the Heat-Exchanger design: n = 64 = 8 x 8): no padding rows, so the per-entry
// validity tests (r < n, c < n) and the index clamps disappear.  They compiled to one divergent branch per matrix
// entry and component (s_and_saveexec / s_cbranch_execz / s_or + hazard s_nops around every exp): ~10 of the
// ~45 instructions an entry costs in a kernel that is instruction-issue bound.
// Waves per SIMD the register allocator is asked to fit (A/B switches; defaults = what measured fastest, profiles/r03/):
// the kernel is bound by the latency of its per-column LDS round trip as much as by VALU issue, so for n <= 64 a
// fourth wave per SIMD (128 VGPRs, at the price of 84 B of scratch per lane in the generation phase) is worth 8.6 %
// on the Heat-Exchanger grid (9.15 -> 8.37 ms, same box); a fifth wave (102 VGPRs) spills the matrix itself: 17.2 ms.
// G = 16 (64 < n <= 128): 4 stays (5: 6.18 -> 8.23 ms on the 2-D grid).  Prediction instances (NE = 4): 3 instead of 2
// (Ground-Vibrations tables 4.52 -> 4.07 ms; 4: 4.83).
#ifndef CCGP_SMALL_OCC_G8
#define CCGP_SMALL_OCC_G8 4
#endif
#ifndef CCGP_SMALL_OCC_G16
#define CCGP_SMALL_OCC_G16 4
#endif
#ifndef CCGP_FAC_WIDE_MAX
#define CCGP_FAC_WIDE_MAX 64
#endif
#ifndef CCGP_SMALL_OCC_PRED
#define CCGP_SMALL_OCC_PRED 3
#endif
// INV: 0 = none, 1 = explicit inverse (solve(R), HX:454), 2 = analytic gradient of the profile-beta log-likelihood,
// 3 = gradient of log det R with respect to the design (per-design form, entropy criteria BSQ:856-948),
// 4 = leave-one-out mean and variance of every training point (ccgp_loo_batch)
// PROF: sigma2 concentrated out (ordinary kriging, `ord$sig2` HX:759-760; log.likeli D1:424-444): where the likelihood is
// finished the quadratic form q is at hand, so cs = sigma2 sum w^2 becomes the draw's own q / n, and the gradient epilogue
// reads that value instead of the caller's -- by the envelope theorem the closed form at (beta_hat, sigma2_hat) IS the
// gradient of the profiled likelihood.  A template parameter, not a branch: the n <= 64 instances sit at the edge of their
// register budget (CCGP_SMALL_OCC_G8 above) and the existing instantiations compile from unchanged code.
// SETS: many training sets of one shape in one launch (the lockstep fit of a simulation study): the evaluation's design,
// right-hand side and sigma2 come from its set, everything after the loads is the code of the single-set instances in the
// same order, hence their bits.  A template parameter for the same reason as PROF.  G = 16 has one matrix per workgroup, so
// the set's design goes into the shared xs slot; G = 8 keeps one copy per matrix where the per-design form keeps it.
// FAC with SETS (ccgp_predict_batch_sets, ccgp_krige_predict_batch_sets, ccgp_predict_summary_sets): the plain-likelihood sets
// instance that writes its FacLayout block as the FAC instance does, on both grids, so that one factorisation launch serves
// the rows of all training sets of a prediction; a template combination, not a branch, for the same reason.
// INV = 2 with PROF and SETS (ccgp_profile_batch_sets): the ordinary-kriging fits of many sets in lockstep.  The gradient
// epilogue takes its differences from xs and its right-hand side from zb, so it is the single-set instance's code as it is.
// CHAIN: a Metropolis chain per workgroup (ccgp_metro_segments_sets): the sets likelihood instance evaluating again and
// again.  The set's design is loaded once; then, per proposal, wave 0 forms the candidate theta + e_t and its portable terms
// (chain_terms.h) into th[] / w2[], the evaluation below runs as it is -- same operations in the same order as the sets
// instance, hence the likelihood bits ccgp_loglik_batch_sets gives that row -- and thread 0 decides, publishes the decision
// through LDS and, after one barrier, every thread reads the same word: go on with the next proposal or leave.  The trip
// count is bounded by n_prop[a]; no path waits on another workgroup.  A template parameter, as PROF and SETS are.
// FIT: an ordinary-kriging start per workgroup (ccgp_profile_fit_sets): the profiled-gradient sets instance (INV = 2, K = 1)
// evaluating again and again.  The set's design and the start's state (fit_logic.h) are loaded once; then, per evaluation,
// wave 0 forms theta = exp(trial) by the portable exp into th[] (w^2 = 1), generation, sweep with identity rows and gradient
// epilogue run as they are -- the operations of the sets instance in its order, hence the bits ccgp_profile_batch_sets gives
// that row -- with the likelihood and the gradient row left in LDS; thread 0 runs fit_feed on them, writes the trace and
// publishes one word, and after one barrier every thread reads it: go on with the next trial or leave.  The trip count is
// bounded by max_evals[a] <= 4096; no path waits on another workgroup.  On exit the state goes back to HBM.
// NM (with CHAIN): a Nelder-Mead search per workgroup (ccgp_laplace_search_sets): the chain instance with the search of
// nm_logic.h in place of the walk.  The set's design, the two tables and the search's state are loaded once; then, per
// evaluation, wave 0 forms the portable terms of the state's `trial` -- the chain's code with trial in place of theta + e_t --,
// the evaluation runs as it is, thread 0 forms val in logpost_rows' order, runs nm_feed on the LDS state, writes the trace and
// publishes one word, and after one barrier every thread reads it.  The trip count is bounded by max_evals[a] <= 4096; no
// path waits on another workgroup.  A failed factorisation is a non-finite value: the search goes on.  On exit the state
// goes back to HBM.
// DFIT: a start of the maximum-entropy design search per workgroup (ccgp_design_fit): the design-gradient instance (INV = 3)
// evaluating again and again.  The shared parameter row, the fixed rows D.old and the start's state (fit_logic.h, d = nv) are
// loaded once; then, per evaluation, all threads scatter the state's `trial` into the free rows of xs, generation, sweep with
// identity rows, reductions and the two-pass gradient epilogue run as they are -- the operations of the single call in its
// order, hence the bits ccgp_mixed_logdet_grad_designs gives that design -- with log det and the gradient (in variable order)
// left in LDS; thread 0 forms f = -(ld - ld_offset) and g = -grad, runs fit_feed, writes the trace and publishes one word,
// and after one barrier every thread reads it.  The trip count is bounded by max_evals[a] <= 4096; no path waits on another
// workgroup.  On exit the state goes back to HBM.
// FAM (CCGP_OPT_FAMILY_FUSED): the plain likelihood instance, with or without SETS / CHAIN / NM, generating the matrix of a 1-D
// family (d = 1: Matern for every component, or Matern + spline -- a run-time branch on a.fam.id inside family_corr) in place
// of the Gaussian one: per component q and entry (r, c), r >= c, what cov_kernel<1> forms -- rate = theta_to_rate(theta_q),
// h = x_r - x_c from the one coordinate in xs, the family's correlation of rate h^2, accumulated with fma(w_q^2, ., acc) --
// then the instance's own post_scale / post_shift.  The diagonal is an entry like any other (h = 0: exactly 1 per component),
// two coincident points give two equal rows and a zero pivot, a NaN coordinate a NaN matrix.  th[] keeps holding theta (under
// CHAIN / NM: what chain_rate writes); us[] and the expanded distance are not formed.  Everything after the generation phase
// is the instance's code unchanged.  Compiled for n <= 32 only (small_family_fused_supported): NB <= 2 on the 16 x 16 grid,
// NB <= 4 on the 8 x 8, general (non-FULL) instances.
// FAM with FAC, and FAM with INV = 4 (CCGP_OPT_FAMILY_FUSED_PREDICT): the same generation phase in front of the instance that
// keeps its factor for a prediction (both grids; the test sites' correlation vectors come from site_corr_family_kernel) and of
// the leave-one-out instance (16 x 16 grid).  Neither epilogue reads us[] or th[], so both run as they are.  No FAM instance
// carries extra rows (NE > 1 without INV): a family's prediction is the kept-factor scheme or the blocked sweep.
// FAM with PROF (value only) and FAM with INV = 2 -- plain, PROF, PROF + SETS -- (CCGP_OPT_FAMILY_FUSED_GRAD): the same
// generation phase in front of the profiled likelihood and of the gradient instance.  In the gradient epilogue a FAM branch
// stands in for the Gaussian regeneration: per pair (i >= j) and component q, family_corr_grad gives (R_q, D_q = d R_q /
// d theta_q) of rate_q (h h), h = x_i - x_j from xs; gs[q] += m R_q, hk[q] += m D_q; the weight column is 2 sigma2 w_q sum as
// ever, the theta column + sigma2 w_q^2 sum m D_q.  us[] and the expanded distance are not read; the diagonal gives D = 0.
template <int G, int NB, int NE, bool FULL = false, int INV = 0, bool FAC = false, bool PROF = false, bool SETS = false,
          bool CHAIN = false, bool FIT = false, bool NM = false, bool DFIT = false, bool FAM = false>
__global__ __launch_bounds__(256, INV ? 1 : (NE > 1 ? CCGP_SMALL_OCC_PRED : (G == 8 ? (NB > 8 ? 2 : CCGP_SMALL_OCC_G8) : CCGP_SMALL_OCC_G16)))
void small_reg_kernel(RegArgs a) {
  static_assert(!FAM || (!FULL && !FIT && !DFIT && G * NB <= kFamilyFusedMaxN &&
                         ((NE == 1 && !INV && !PROF) || (INV == 4 && !PROF) ||
                          (NE == 1 && !INV && PROF && !SETS && !CHAIN && !FAC) || (INV == 2 && (PROF || !SETS)))),
                "a 1-D family is generated by the general plain-likelihood instance (with or without SETS / CHAIN / NM, or keeping "
                "its factor), by the leave-one-out instance, by the value-only profiled instance and by the gradient instance "
                "(plain, profiled, profiled over sets), at n <= 32");
  static_assert(!INV || (G == 16 && NE == NB + 1 && !FULL), "the inverse / gradient runs one matrix per workgroup with n identity rows");
  static_assert(!FAC || (NE == 1 && !FULL && !INV), "the factor is kept by the plain likelihood instantiation");
  static_assert(!PROF || ((NE == 1 || INV == 2) && INV != 1 && INV != 3 && !FAC), "sigma2 is concentrated out of the likelihood and of its gradient only");
  static_assert(!SETS || ((NE == 1 && !INV && !PROF) || (INV == 2 && PROF && !FAC)),
                "the sets form exists for the plain likelihood (with or without the kept factor) and for the profiled gradient only");
  static_assert(!CHAIN || (SETS && G == 16 && NE == 1 && !INV && !PROF && !FAC), "a chain is the sets likelihood instance on the 16 x 16 grid");
  static_assert(!FIT || (SETS && PROF && INV == 2 && !CHAIN), "a fit is the profiled-gradient sets instance");
  static_assert(!NM || CHAIN, "a Laplace search is a chain instance with another step");
  static_assert(!DFIT || (INV == 3 && G == 16 && !PROF && !SETS && !CHAIN && !FIT), "a design search is the design-gradient instance, one workgroup per start");
  constexpr int TPM = G * G;       // threads per matrix
  constexpr int MPW = 256 / TPM;   // matrices per workgroup
  constexpr int NP = G * NB;       // padded order
  constexpr int XR = G * NE;       // extra rows (y', 1', then test sites)
  constexpr int MT = XR - 2;       // test sites per chunk
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // the factorisation a prediction waits for is ONE wave per draw running at the latency of its n columns, with the site
  // correlation kernel's waves issuing beside it on the same SIMDs: it goes first
  if constexpr (FAC) __builtin_amdgcn_s_setprio(3);
  const int n = a.n, d = a.d, K = a.K;
  const int tid = threadIdx.x, sub = tid / TPM, lt = tid % TPM;
  const int ty = lt % G, tx = lt / G;
  int b = a.draw0 + blockIdx.x * MPW + sub;
  const bool valid = b < a.draw0 + a.B;
  if (!valid) b = a.draw0 + a.B - 1;   // keep the wave alive (shared loads, barriers); results discarded

  const RegCarve cv(G, NB, NE, INV != 0, false, n, d, K);
  double* etab = smem + cv.etab;              // 2^(j/256) for exp_cov, shared by the workgroup
  double* xs = smem + cv.xs;                  // d x n, shared by the matrices of this workgroup
  double* mine = smem + cv.mat0 + (size_t)sub * cv.per_mat;
  double* us = mine + cv.us;
  double* th = mine + cv.th;
  double* w2 = mine + cv.w2;
  double* colbuf = mine + cv.colbuf;          // [2][NP + XR]
  double* dvec = mine + cv.dvec;
  double* zb = mine + cv.zb;                  // [2][NP]
  double* slack = mine + cv.slack;            // beta, 1'R^-1 1 for the epilogues
  double* ut = mine + cv.ut;                  // [K][XR]   (NE > 1, prediction)
  double* psum = mine + cv.psum;              // [3][XR][G] (NE > 1, prediction)
  double* zmat = mine + cv.zmat;              // [NP][NP + 2] (INV): row t = L'^-1 e_t, columns scaled by d_c^-1/2
  double* xt = smem + cv.xt;                  // [d][XR], shared by the workgroup (NE > 1)
  const int t0 = blockIdx.y * MT;             // first test site of this chunk

  const int pb = a.shared_params ? 0 : b;
  if (CCGP_SMALL_EXP_TABLE) exp_table_load(etab, tid, 256);
  // CHAIN: proposals used, draws accepted and factorisations failed so far (uniform over the workgroup), the chain's words
  double* cst = nullptr;
  int ct = 0, cacc = 0, cfail = 0;
  if constexpr (NM) {
    cst = smem + cv.total;
    const NmIO& nm = a.nm;
    const double* sg = nm.state + (size_t)b * nm.W;
    // a search that is not running, or has no evaluations to make, stays as it came (every thread reads the same words)
    if (nm.max_evals[b] <= 0 || sg[kNmCode] != (double)kNmRunning) {
      if (tid == 0) { nm.evals[b] = 0; nm.nfail[b] = 0; }
      return;
    }
    for (int e = tid; e < kChainTable; e += 256) {
      cst[kChainHi + e] = __longlong_as_double((long long)kExpTableBits[e]);
      cst[kChainLo + e] = __longlong_as_double((long long)kChainExpLoBits[e]);
    }
    for (int e = tid; e < nm.W; e += 256) cst[kNmState + e] = sg[e];
  } else if constexpr (CHAIN) {
    cst = smem + cv.total;
    const ChainIO& ch = a.ch;
    if (ch.n_prop[b] <= 0 || ch.stop_acc[b] <= 0) {   // nothing to do: the state as it came (every thread reads the same words)
      if (tid == 0) {
        ch.used[b] = 0; ch.nacc[b] = 0; ch.nfail[b] = 0;
        for (int j = 0; j < ch.p; ++j) ch.theta_fin[b + (size_t)j * a.B] = ch.theta0[b + (size_t)j * a.B];
        ch.l_fin[b] = ch.l0[b];
        ch.beta_fin[b] = ch.beta0[b];
      }
      return;
    }
    for (int e = tid; e < kChainTable; e += 256) {
      cst[kChainHi + e] = __longlong_as_double((long long)kExpTableBits[e]);
      cst[kChainLo + e] = __longlong_as_double((long long)kChainExpLoBits[e]);
    }
    if (tid < ch.p) cst[kChainTheta + tid] = ch.theta0[b + (size_t)tid * a.B];
    if (tid == 0) { cst[kChainL] = ch.l0[b]; cst[kChainBeta] = ch.beta0[b]; }
  }
  // FIT: evaluations made and factorisations failed so far in this call (uniform over the workgroup), the start's words
  double* fst = nullptr;
  int ft = 0, ffail = 0;
  if constexpr (FIT) {
    fst = smem + cv.total;
    const FitIO& fi = a.fit;
    const double* sg = fi.state + (size_t)b * fi.W;
    // a start that is not running, or has no evaluations to make, stays as it came (every thread reads the same words)
    if (fi.max_evals[b] <= 0 || sg[kFitCode] != (double)kFitRunning) {
      if (tid == 0) { fi.evals[b] = 0; fi.nfail[b] = 0; }
      return;
    }
    for (int e = tid; e < kChainTable; e += 256) {
      fst[kFitHi + e] = __longlong_as_double((long long)kExpTableBits[e]);
      fst[kFitLo + e] = __longlong_as_double((long long)kChainExpLoBits[e]);
    }
    for (int e = tid; e < fi.W; e += 256) fst[kFitState + e] = sg[e];
  }
  // DFIT: evaluations made and eliminations failed so far in this call (uniform over the workgroup), the start's words
  double* dfs = nullptr;
  int dft = 0, dffail = 0;
  if constexpr (DFIT) {
    dfs = smem + cv.xs_own + (size_t)d * n;   // behind the per-design carve
    const DesignFitIO& df = a.dfit;
    const double* sg = df.state + (size_t)b * df.W;
    // a start that is not running, or has no evaluations to make, stays as it came (every thread reads the same words)
    if (df.max_evals[b] <= 0 || sg[kFitCode] != (double)kFitRunning) {
      if (tid == 0) { df.evals[b] = 0; df.nfail[b] = 0; }
      return;
    }
    for (int e = tid; e < df.W; e += 256) dfs[kDfGrad + (n - a.n_fixed) * d + e] = sg[e];
  }
  int st = 0;   // SETS: this evaluation's training set
  if constexpr (DFIT) {
    // the fixed rows every start shares; the free rows come from the state's trial point, evaluation by evaluation
    xs = smem + cv.xs_own;
    const int nf = a.n_fixed;
    for (int e = tid; e < nf * d; e += 256) xs[(e / nf) * n + e % nf] = a.dfit.D_old[e];
  } else if constexpr (SETS) {
    // a matrix's threads are whole waves on both grids: the set index is wave-uniform, and saying so keeps it -- and the
    // addresses formed from it -- in scalar registers across the generation phase
    st = __builtin_amdgcn_readfirstlane(a.set[b]);
    const double* Xb = a.X + (size_t)st * n * d;
    if constexpr (MPW > 1) xs = smem + cv.xs_own + (size_t)sub * d * n;
    for (int e = lt; e < n * d; e += TPM) xs[e] = Xb[e];
  } else if (a.x_stride == 0) {
    for (int e = tid; e < n * d; e += 256) xs[e] = a.X[e];
  } else {
    // per-evaluation designs: each matrix keeps its own copy right behind the shared slot
    xs = smem + cv.xs_own + (size_t)sub * d * n;
    for (int e = lt; e < n * d; e += TPM) xs[e] = a.X[(size_t)b * a.x_stride + e];
  }
  if constexpr (!CHAIN && !FIT) {
    for (int e = lt; e < K * d; e += TPM) th[e] = a.params[pb + (size_t)(K + e) * a.ldp];
    if (lt < K) {
      const double w = a.params[pb + (size_t)lt * a.ldp];
      w2[lt] = w * w;
    }
  } else {
    __syncthreads();   // the tables, the start state and the design are in LDS
  }
  if constexpr (DFIT) __syncthreads();   // the start's state is in LDS
chain_next:
  if constexpr (DFIT) {
    // variable v = i d + k of the trial point is free row i, dimension k
    const int nf = a.n_fixed, nv = (n - nf) * d;
    const double* trial = fit_trial(dfs + kDfGrad + nv, nv);
    for (int e = tid; e < nv; e += 256) xs[(e % d) * n + nf + e / d] = trial[e];
  }
  if constexpr (NM) {
    if (tid < 64) {   // wave 0, every lane the same arithmetic; lane 0 writes
      const NmIO& nm = a.nm;
      const double* trial = nm_trial(cst + kNmState, nm.q);
      double cand[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) cand[j] = j < nm.q ? trial[j] : 0.0;
      const ChainTerms tm = chain_terms(nm.prior_id, cand, nm.prior_pars, cst + kChainHi, cst + kChainLo);
      if (tid == 0) {
        w2[0] = tm.w0 * tm.w0;
        w2[1] = tm.w1 * tm.w1;
        cst[kChainLj] = tm.lj;
        cst[kChainLp] = tm.lp;
      }
      for (int e = tid; e < 2 * d; e += 64) th[e] = chain_rate(tm, nm.prior_id, e / d, e % d);
    }
  } else if constexpr (CHAIN) {
    if (tid < 64) {   // wave 0, every lane the same arithmetic; lane 0 writes
      const ChainIO& ch = a.ch;
      const double* e = ch.steps + ((size_t)b * ch.T + ct) * ch.p;
      double cand[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) cand[j] = j < ch.p ? cst[kChainTheta + j] + e[j] : 0.0;
      const ChainTerms tm = chain_terms(ch.prior_id, cand, ch.prior_pars, cst + kChainHi, cst + kChainLo);
      if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cst[kChainCand + j] = cand[j];
        w2[0] = tm.w0 * tm.w0;
        w2[1] = tm.w1 * tm.w1;
        cst[kChainLj] = tm.lj;
        cst[kChainLp] = tm.lp;
      }
      // the 2 d rates: every lane holds tm, so lane e stores rate e (d <= 64: two passes at the most)
      for (int e = tid; e < 2 * d; e += 64) th[e] = chain_rate(tm, ch.prior_id, e / d, e % d);
    }
  }
  if constexpr (FIT) {
    if (tid < 64) {   // wave 0: the parameter row (1, theta) of the trial point, theta_k = exp(trial_k)
      const double* trial = fit_trial(fst + kFitState, d);
      for (int e = tid; e < d; e += 64) th[e] = fit_theta(trial[e], fst + kFitHi, fst + kFitLo);
      if (tid == 0) w2[0] = 1.0;
    }
  }
  if constexpr (NE > 1 && !INV) {
    for (int e = tid; e < d * XR; e += 256) {
      const int k = e / XR, r = e % XR, t = t0 + r - 2;
      xt[e] = (r >= 2 && t < a.m) ? a.Xt[t + (size_t)k * a.m] : 0.0;
    }
  }
  __syncthreads();
  for (int e = lt; e < (FAM ? 0 : K * n); e += TPM) {   // (a 1-D family takes its distance from the direct difference: no us[])
    const int c = e / n, i = e % n;
    double s = 0.0;
    for (int k = 0; k < d; ++k) { const double v = xs[k * n + i]; s += v * v * th[c * d + k]; }
    us[c * NP + i] = s;
  }
  if constexpr (NE > 1 && !INV) {
    for (int e = lt; e < K * XR; e += TPM) {
      const int c = e / XR, r = e % XR;
      double sq = 0.0;
      for (int k = 0; k < d; ++k) { const double v = xt[k * XR + r]; sq += v * v * th[c * d + k]; }
      ut[c * XR + r] = sq;
    }
  }
  __syncthreads();

  double sw = 0.0;
  for (int c = 0; c < K; ++c) sw += w2[c];
  double sigma2 = a.sigma2;
  if constexpr (SETS && !PROF) sigma2 = a.sigma2_set[st];   // PROF forms its own
  const double cs = sigma2 * sw;
  // (p^2 R1 + (1-p)^2 R2) / (p^2 + (1-p)^2) (HX:412) as a multiplication by the reciprocal: one
  // fp64 division costs ~30 instructions and this kernel is instruction-issue bound (<= 1 ulp apart)
  const double post_scale = (a.mode == 1 ? cs : 1.0) / sw;
  const double post_shift = a.mode == 1 ? a.tau2 : 0.0;

  // ---- generate the lower triangle and the right-hand-side row into registers ------------------
  // Per component q and column-block pair, the k-loop keeps the dot products
  // s[a][j] = sum_k (x_rk theta_qk) x_ck of all the thread's entries in registers, so each
  // (q, k) step costs the thread's row coordinates once per pair instead of three LDS reads
  // and a loop iteration per ENTRY (this kernel is instruction-issue bound).
  double M[NB][NB];   // M[a][b], a >= b
  double E[NE][NB];   // extra rows ty + G e: 0 -> y', 1 -> 1', 2.. -> r(x_t)' of this chunk's test sites
#pragma unroll
  for (int bb = 0; bb < NB; ++bb)
#pragma unroll
    for (int aa = bb; aa < NB; ++aa) M[aa][bb] = 0.0;
  int rowi[NB];   // clamped row of every row block (padding rows repeat row n-1; they are overwritten below)
#pragma unroll
  for (int aa = 0; aa < NB; ++aa) rowi[aa] = FULL ? ty + G * aa : min(ty + G * aa, n - 1);
  if constexpr (FAM) {
    // a 1-D family's entries as cov_kernel<1> forms them (cov.hip), component by component in its order
    for (int q = 0; q < K; ++q) {
      const double wq = w2[q], rate = theta_to_rate(a.fam, th[q], q);
#pragma unroll
      for (int bb = 0; bb < NB; ++bb) {
        const int c = tx + G * bb;
#pragma unroll
        for (int aa = 0; aa < NB; ++aa) {
          if (aa < bb) continue;
          const int r = ty + G * aa;
          if (r < n && c < n && r >= c) {
            const double h = xs[r] - xs[c];
            M[aa][bb] = fma(wq, family_corr(a.fam.id, a.fam.nu, a.fam.norm, rate * (h * h), q), M[aa][bb]);
          }
        }
      }
    }
  }
  // The exp of a matrix entry.  The extra-row prediction instances (NE > 1, no INV) take it through the range select: their
  // 12 x 11 lattice at n = 128 reaches exponents of 2^148.8, beyond the unselected polynomial's domain (below 2^148.47: include/ccgp.h), where rates of
  // 2^140 must still give R = I (tests/test_gpu_far_arguments.py).  Every other instance -- the likelihood, gradient, profile,
  // sets, chain and fit instances that the select was measured on and rejected for (profiles/exp_poly_range_select.md) -- keeps
  // exp_small as it was: the constexpr folds, and their code is the parent's.
  auto gen_exp = [&](double dist) {
    if constexpr (NE > 1 && !INV) return exp_small_ranged<!FULL>(dist, etab);
    else return exp_small<!FULL>(dist, etab);
  };
  for (int q = 0; q < (FAM ? 0 : K); ++q) {
    const double wq = w2[q];
#pragma unroll
    for (int bb0 = 0; bb0 < NB; bb0 += 2) {
      constexpr int kPair = 2;
      double sdot[NB][kPair];
#pragma unroll
      for (int aa = 0; aa < NB; ++aa) sdot[aa][0] = sdot[aa][1] = 0.0;
      const int c0 = FULL ? tx + G * bb0 : min(tx + G * bb0, n - 1);
      const int c1 = FULL ? tx + G * (bb0 + 1 < NB ? bb0 + 1 : bb0) : min(tx + G * (bb0 + 1), n - 1);
      for (int k = 0; k < d; ++k) {
        // all LDS reads of this dimension first (one round trip), then the arithmetic: left to itself the
        // compiler reuses one register pair for the row coordinates and waits after every single read
        const double* xk = xs + k * n;
        double xrow[NB];
#pragma unroll
        for (int aa = bb0; aa < NB; ++aa) xrow[aa] = xk[rowi[aa]];
        const double tq = th[q * d + k];
        const double xc0 = xk[c0], xc1 = xk[c1];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int aa = bb0; aa < NB; ++aa) {
          const double xr = xrow[aa] * tq;
          sdot[aa][0] = fma(xr, xc0, sdot[aa][0]);
          if (aa >= bb0 + 1 && bb0 + 1 < NB) sdot[aa][1] = fma(xr, xc1, sdot[aa][1]);
        }
      }
#pragma unroll
      for (int j = 0; j < kPair; ++j) {
        const int bb = bb0 + j;
        if (bb >= NB) continue;
        const int c = tx + G * bb;
#pragma unroll
        for (int aa = 0; aa < NB; ++aa) {
          // constant trip count + a test that folds away: with `aa = bb` as the lower bound the unroller left this
          // loop rolled for odd NB >= 9 (bb is only known once the two loops around it are unrolled), and ONE access
          // with a run-time index puts the whole matrix in scratch (1.6 KB per lane at NB = 13)
          if (aa < bb) continue;
          const int r = ty + G * aa;
          if constexpr (FULL) {
            // every (r, c) is a matrix entry; entries above the diagonal of the diagonal blocks (aa == bb, ty < tx)
            // are computed too and zeroed below -- cheaper than a divergent branch
            const double dist = (us[q * NP + r] + us[q * NP + c]) + (-2.0 * sdot[aa][j]);
            M[aa][bb] = fma(wq, gen_exp(dist), M[aa][bb]);
            // pin the finished entry here: without the branch the compiler sinks the tail of every exp (ldexp + mix)
            // to the end of the component loop and keeps two temporaries per entry alive until then (580 B of scratch)
            asm volatile("" : "+v"(M[aa][bb]));
          } else if (r < n && c < n && r >= c) {
            const double dist = (us[q * NP + r] + us[q * NP + c]) + (-2.0 * sdot[aa][j]);
            M[aa][bb] = fma(wq, gen_exp(dist), M[aa][bb]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int bb = 0; bb < NB; ++bb) {
    const int c = tx + G * bb;
#pragma unroll
    for (int aa = bb; aa < NB; ++aa) {
      const int r = ty + G * aa;
      if (FULL || (r < n && c < n)) M[aa][bb] = (aa > bb || r >= c) ? fma(post_scale, M[aa][bb], post_shift) : 0.0;
      else M[aa][bb] = r == c ? 1.0 : 0.0;   // identity on the padding
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int ridx = ty + G * e;
      double v = 0.0;
      if (FULL || c < n) {
        if (ridx == 0) v = DFIT ? 0.0 : SETS ? a.y[(size_t)st * n + c] : a.y[c];   // (a design search has no response)
        else if (ridx == 1) v = 1.0;
        else if (INV) v = (ridx - 2 == c) ? 1.0 : 0.0;   // identity rows: row 2 + t = e_t'
        else if (NE > 1 && t0 + ridx - 2 < a.m) {
          // Mixed.corr.vec (HX:425-431), corr.vec operation order (HX:373): (theta'x^2 - 2 X Theta x) + u_i
          double acc = 0.0;
          for (int q = 0; q < K; ++q) {
            double sd = 0.0;
            for (int k = 0; k < d; ++k) sd = fma(xs[k * n + c] * th[q * d + k], xt[k * XR + ridx], sd);
            const double dist = (ut[q * XR + ridx] - 2.0 * sd) + us[q * NP + c];
            acc = fma(w2[q], exp_small_ranged<!FULL>(dist, etab), acc);   // a cross vector passes no pivot test
          }
          v = acc / sw;
        }
      }
      E[e][bb] = v;
    }
  }

  // ---- L' D L'^T on registers; one column broadcast through LDS per step ------------------------
  int bad = 0, cur = 0;
  // a bare log-determinant (entropy criteria, BSQ:856-877: the reference calls det(), nothing can "fail") keeps 0
  const double ptol = (DFIT || a.logdet) ? 0.0 : pivot_tolerance(a.mode, n);
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
#pragma unroll 1
    for (int kk = 0; kk < G; ++kk) {
      const int k = G * kb + kk;
      if (bad || (!FULL && k >= n)) break;
      double* cb = colbuf + cur * (NP + XR);
      if (tx == kk) {
#pragma unroll
        for (int aa = kb; aa < NB; ++aa) cb[ty + G * aa] = M[aa][kb];
#pragma unroll
        for (int e = 0; e < NE; ++e)
          if (!INV || e < kb + 2) cb[NP + ty + G * e] = E[e][kb];
      }
      mat_sync<G>();
      // every thread of the matrix reads the same word; handing it over through v_readfirstlane tells the compiler
      // that it -- and with it `bad`, the loop exit and the buffer toggle -- is wave-uniform: scalar branch and
      // scalar address arithmetic instead of exec-mask bookkeeping per column
      const double piv_v = cb[k];
      const double piv = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(piv_v)),
                                          __builtin_amdgcn_readfirstlane(__double2loint(piv_v)));
      if (!(piv > ptol)) { bad = k + 1; break; }   // uniform over the matrix's threads (pivot_tolerance: ccgp_internal.h)
      if constexpr (INV == 3) {
        if (__builtin_isinf(piv)) { bad = k + 1; break; }   // the design gradient's failure rule: pivot <= 0 or not finite
      }
      // 1 / pivot by v_rcp_f64 + two Newton steps (full precision, ~6 instructions instead of ~30)
      double rinv = __builtin_amdgcn_rcp(piv);
      rinv = fma(fma(-piv, rinv, 1.0), rinv, rinv);
      rinv = fma(fma(-piv, rinv, 1.0), rinv, rinv);
      if (lt == 0) dvec[k] = piv;
      if constexpr (FAC) {
        // column k of L' (the values every thread forms as lc below), into the row-major packed factor: entry (i, k) of row i
        if (valid) {
          double* Lp = a.fac + (size_t)b * a.fac_stride + FacLayout(n).L + fac_col(n, k) - (k + 1);
          for (int i = k + 1 + lt; i < n; i += TPM) Lp[i] = cb[i] * rinv;
        }
      }
      double lc[NB], lr[NB];
#pragma unroll
      for (int bb = kb; bb < NB; ++bb) lc[bb] = cb[tx + G * bb] * rinv;
      if (tx <= kk) lc[kb] = 0.0;   // columns <= k are finished
#pragma unroll
      for (int aa = kb; aa < NB; ++aa) lr[aa] = cb[ty + G * aa];
      // FULL instantiation (n = G NB, the Heat-Exchanger grid): rows <= k of the diagonal block are NOT masked: lr[kb]
      // only reaches M[kb][kb], and there a row r <= k meets either a finished column (protected by the lc mask
      // above) or a column c > k >= r, i.e. an entry above the diagonal that nothing reads.  Three instructions per
      // column less in an issue-bound kernel.  The general instantiation keeps the mask (round-2 advisor): the
      // unnormalised above-diagonal entries could reach Inf on a nearly singular matrix, and Inf * 0 = NaN would
      // then leak into finished entries with status still 0.
      if constexpr (!FULL) {
        if (ty <= kk) lr[kb] = 0.0;   // rows <= k are finished
      }
      // identity rows (INV): row 2 + t = e_t' is still exactly zero left of column t, so at step k only the rows
      // t <= k have anything to subtract: extra-row blocks e > (k + 2) / G are skipped (kb is unrolled: static)
      constexpr int NEmax = NE;
      const int ne_live = INV ? (kb + 2 < NEmax ? kb + 2 : NEmax) : NEmax;
      double le[NE];
#pragma unroll
      for (int e = 0; e < NE; ++e)
        if (e < ne_live) le[e] = cb[NP + ty + G * e];
#pragma unroll
      for (int bb = kb; bb < NB; ++bb) {
#pragma unroll
        for (int aa = bb; aa < NB; ++aa) M[aa][bb] = fma(-lr[aa], lc[bb], M[aa][bb]);
#pragma unroll
        for (int e = 0; e < NE; ++e)
          if (e < ne_live) E[e][bb] = fma(-le[e], lc[bb], E[e][bb]);
      }
      cur ^= 1;
    }
  }
  // z'_y[c] and z'_1[c] sit in threads ty = 0 / 1
  if (ty < 2) {
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) zb[ty * NP + tx + G * bb] = E[0][bb];
  }
  mat_sync<G>();

  // ---- reductions (first wave of the matrix's threads) --------------------------------------------
  if (lt < 64) {
    const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
    double logdet = 0.0, s11 = 0.0, s1y = 0.0, syy = 0.0;
    if (!bad)
      for (int k = lt; k < n; k += 64) {
        const double dk = dvec[k], zy = zb[k], z1 = zb[NP + k];
        logdet += log(dk);
        s11 += z1 * z1 / dk;
        s1y += z1 * zy / dk;
        syy += zy * zy / dk;
      }
    for (int off = 32; off > 0; off >>= 1) {
      logdet += __shfl_xor(logdet, off, 64);
      s11 += __shfl_xor(s11, off, 64);
      s1y += __shfl_xor(s1y, off, 64);
      syy += __shfl_xor(syy, off, 64);
    }
    const double kLog2Pi = 1.8378770664093454835606594728112;
    double beta = 0.0, ll, q = 0.0;
    if (a.mode == 0) {
      beta = s1y / s11;
      if (!bad)
        for (int k = lt; k < n; k += 64) {
          const double r = zb[k] - beta * zb[NP + k];
          q += r * r / dvec[k];
        }
      for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
      if constexpr (PROF) {
        // q / cs = n at cs = q / n: l_p = -(n log 2 pi + n log cs_hat + log det R + n) / 2; q = 0 (a constant y): +Inf
        const double csh = q / n;
        if constexpr (FIT) ll = fit_loglik(n, kLog2Pi, log(csh), logdet);
        else ll = -0.5 * (n * kLog2Pi + n * log(csh) + logdet + n);
        if (lt == 0) slack[2] = csh;   // for the gradient epilogue
        if constexpr (!FIT) {
          if (lt == 0 && valid && blockIdx.y == 0) a.s2hat[b] = bad ? kNaN : csh / sw;
        }
      } else if constexpr (CHAIN) {
        ll = chain_loglik(n, kLog2Pi, log(cs), logdet, q / cs);
      } else {
        ll = -0.5 * (n * kLog2Pi + n * log(cs) + logdet + q / cs);
      }
    } else {
      ll = -0.5 * (n * kLog2Pi + logdet + syy);
    }
    if (bad) { ll = kNaN; beta = kNaN; }
    if constexpr (FIT) {
      if (lt == 0) fst[kFitLl] = ll;
    }
    if constexpr (DFIT) {
      if (lt == 0) dfs[kDfLd] = bad ? kNaN : logdet;
    }
    if (lt == 0) {
      slack[0] = beta;      // for the epilogues
      slack[1] = s11;
      // Q = (y - beta 1)'R^-1 (y - beta 1) as the profiled likelihood sums it (PROF above: q = n sum w^2 sigma2_hat), for the
      // variance forms of the prediction epilogues
      if constexpr (NE > 1) slack[3] = q;
    }
    if constexpr (FAC) {
      if (valid) {
        const FacLayout fl(n);
        double* F = a.fac + (size_t)b * a.fac_stride;
        if (lt == 0) { F[0] = beta; F[1] = s11; F[2] = bad ? 1.0 : 0.0; F[3] = sw; F[4] = q; }
        for (int c = lt; c < n; c += 64) {
          F[fl.rd + c] = bad ? 0.0 : 1.0 / dvec[c];
          F[fl.zy + c] = zb[c];
          F[fl.z1 + c] = zb[NP + c];
        }
      }
    }
    if (lt == 0 && valid && blockIdx.y == 0) {
      if (a.loglik) a.loglik[b] = ll;
      if (a.beta) a.beta[b] = beta;
      if (a.status) a.status[b] = bad;
      if (a.logdet) a.logdet[b] = bad ? kNaN : logdet;
      if constexpr (NE > 1 || FAC) {
        if (a.vf.q) a.vf.q[b] = bad ? kNaN : q;
      }
    }
    if constexpr (NM) {
      if (lt == 0) {   // the step of laplace_sets' search on this evaluation's value
        const NmIO& nm = a.nm;
        const double val = chain_value(ll, cst[kChainLj], cst[kChainLp]);
        if (nm.tr_val) {
          const size_t at = (size_t)b * nm.T + ct;
          nm.tr_val[at] = val;
          nm.tr_status[at] = bad;
        }
        nm_feed(cst + kNmState, val);
        const int go = cst[kNmState + kNmCode] == (double)kNmRunning && ct + 1 < nm.max_evals[b] && ct + 1 < kNmMaxEvals;
        cst[kChainGo] = go ? 1.0 : 0.0;
      }
    } else if constexpr (CHAIN) {
      if (lt == 0) {   // the accept / reject step of HX:505-535 on this proposal's value
        const ChainIO& ch = a.ch;
        const size_t at = (size_t)b * ch.T + ct;
        const double val = chain_value(ll, cst[kChainLj], cst[kChainLp]);
        const int acc = __builtin_isfinite(val) && (val - cst[kChainL]) > ch.logu[at];
        if (ch.tr_val) { ch.tr_val[at] = val; ch.tr_beta[at] = beta; ch.tr_status[at] = bad; ch.tr_acc[at] = acc; }
        if (acc) {
          const size_t k = (size_t)b * ch.M + cacc;
          for (int j = 0; j < ch.p; ++j) {
            ch.draws[k * ch.p + j] = cst[kChainCand + j];
            cst[kChainTheta + j] = cst[kChainCand + j];
          }
          ch.draw_val[k] = val;
          ch.draw_beta[k] = beta;
          cst[kChainL] = val;
          cst[kChainBeta] = beta;
        }
        const int used = ct + 1, nacc = cacc + acc;
        const int go = nacc < ch.stop_acc[b] && used < ch.n_prop[b];
        cst[kChainGo] = go ? 1.0 : 0.0;
        cst[kChainAcc] = acc ? 1.0 : 0.0;
        if (!go) {
          ch.used[b] = used; ch.nacc[b] = nacc; ch.nfail[b] = cfail + (bad != 0);
          for (int j = 0; j < ch.p; ++j) ch.theta_fin[b + (size_t)j * a.B] = cst[kChainTheta + j];
          ch.l_fin[b] = cst[kChainL];
          ch.beta_fin[b] = cst[kChainBeta];
        }
      }
    }
  }
  if constexpr (NM) {
    __syncthreads();
    const int go = __builtin_amdgcn_readfirstlane(cst[kChainGo] != 0.0);
    ct += 1;
    cfail += bad != 0;
    if (go) goto chain_next;
    const NmIO& nm = a.nm;
    double* sg = nm.state + (size_t)b * nm.W;
    for (int e = tid; e < nm.W; e += 256) sg[e] = cst[kNmState + e];
    if (tid == 0) { nm.evals[b] = ct; nm.nfail[b] = cfail; }
    return;
  } else if constexpr (CHAIN) {
    __syncthreads();
    const int go = __builtin_amdgcn_readfirstlane(cst[kChainGo] != 0.0);
    cacc += __builtin_amdgcn_readfirstlane(cst[kChainAcc] != 0.0);
    ct += 1;
    cfail += bad != 0;
    if (go) goto chain_next;
    return;
  }
  if constexpr (INV) {
    // R^-1 = Z' D^-1 Z with Z[t][c] = (L'^-1)[c][t] (zero for c < t).  Round 4: the columns are scaled by d_c^-1/2 on the
    // way to LDS, so an entry of R^-1 is a plain dot product of two rows -- two LDS reads and one FMA per term instead of
    // three reads, a multiplication and an FMA -- and the row stride NP + 2 keeps 16-byte alignment: the dot products
    // start at the even column below i (the entries left of the diagonal are exact zeros) and read two terms per
    // ds_read_b128 (conflict-free: consecutive lanes are 2 (NP + 2) dwords = 4 banks mod 64 apart).
    constexpr int ZS = NP + 2;
    typedef double d2v __attribute__((ext_vector_type(2)));
    const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
    mat_sync<G>();
    for (int c = lt; c < NP; c += TPM) dvec[c] = (bad || c >= n) ? 0.0 : sqrt(1.0 / dvec[c]);
    mat_sync<G>();
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int t = ty + G * e - 2;
#pragma unroll
      for (int bb = 0; bb < NB; ++bb) {
        const int c = tx + G * bb;
        if (t >= 0 && t < NP) zmat[t * ZS + c] = (t < n && c < n) ? E[e][bb] * dvec[c] : 0.0;
      }
    }
    mat_sync<G>();
    // rows i and j of the scaled Z: sum over c >= i (i >= j), two terms per step
    auto row_dot = [&](int i, int j) {
      const d2v* zi = reinterpret_cast<const d2v*>(zmat + i * ZS);
      const d2v* zj = reinterpret_cast<const d2v*>(zmat + j * ZS);
      double acc0 = 0.0, acc1 = 0.0;
      for (int h = i >> 1; h < NP / 2; ++h) {
        const d2v u = zi[h], v = zj[h];
        acc0 = fma(u[0], v[0], acc0);
        acc1 = fma(u[1], v[1], acc1);
      }
      return acc0 + acc1;
    };
    if constexpr (INV == 1) {
      if (valid)
        for (int idx = lt; idx < n * n; idx += TPM) {
          const int i = idx % n, j = idx / n;
          if (i < j) continue;
          double acc = row_dot(i, j);
          if (bad) acc = kNaN;
          a.Rinv[i + (size_t)j * n] = acc;
          a.Rinv[j + (size_t)i * n] = acc;
        }
    } else if constexpr (INV == 2) {
      // ---- gradient (build-defined extension; the reference differentiates numerically, HX:493) ------------------
      //   M = (alpha alpha' - Sigma^-1) / 2,  Sigma = cs R,  cs = sigma2 sum w^2,  alpha = Sigma^-1 (y - beta 1)
      //   d loglik / d w_q      =  2 sigma2 w_q   sum_ab M_ab R_q,ab
      //   d loglik / d theta_qk = -  sigma2 w_q^2 sum_ab M_ab (x_ak - x_bk)^2 R_q,ab
      // (the profile-beta term drops out: d loglik / d beta = 0 at beta_hat).  R^-1 entries come from Z as in the
      // inverse; R_q is regenerated from X; every thread takes pairs (a >= b), off-diagonal pairs count twice.
      // Round 4: the pair's R^-1 entry (an n-long dot product: the O(n^3) part) and m = M_ab are formed ONCE per pass
      // over the pairs, and a pass carries QG components x KG dimensions of accumulators -- K = 2, d = 4 (Heat Exchanger)
      // or K = 3, d = 5 is ONE pass; round 3 walked the pairs K ceil(d / 16) times, recomputing R^-1 every time.
      double* alpha = colbuf;                                  // [NP]   (the column buffers are free now)
      double* part = mine + cv.part;                           // [4][kGradSlots] wave partial sums
      const double beta = slack[0];
      // the profiled mode differs here only: this draw's cs_hat = q / n and sigma2_hat = cs_hat / sum w^2 (what s2hat[b] holds)
      const double csg = PROF ? slack[2] : cs;
      const double s2g = PROF ? csg / sw : a.sigma2;
      const bool nograd = bad || (PROF && !(csg > 0.0));   // q = 0: the likelihood is +Inf and has no gradient
      double* resid = zb;                                      // (z_y - beta z_1)_c d_c^-1/2 in place of z_y
      for (int c = lt; c < NP; c += TPM) resid[c] = c < n ? (zb[c] - beta * zb[NP + c]) * dvec[c] : 0.0;
      mat_sync<G>();
      for (int i = lt; i < n; i += TPM) {
        double s = 0.0;
        for (int c = i; c < n; ++c) s = fma(zmat[i * ZS + c], resid[c], s);
        alpha[i] = s / csg;
      }
      mat_sync<G>();
      const int lane64 = lt & 63, wv = lt >> 6;
      auto contract = [&](auto qg_tag, auto kg_tag) {
        constexpr int QG = decltype(qg_tag)::value, KG = decltype(kg_tag)::value;
        static_assert(QG * (1 + KG) <= kGradSlots, "wave partial sums");
        for (int q0 = 0; q0 < K; q0 += QG) {
          for (int k0 = 0; k0 < d; k0 += KG) {
            double gs[QG], hk[QG][KG];
#pragma unroll
            for (int qq = 0; qq < QG; ++qq) {
              gs[qq] = 0.0;
#pragma unroll
              for (int k = 0; k < KG; ++k) hk[qq][k] = 0.0;
            }
            if (!bad)
              for (int idx = lt; idx < n * n; idx += TPM) {
                const int i = idx % n, j = idx / n;
                if (i < j) continue;
                const double m = (i == j ? 0.5 : 1.0) * (alpha[i] * alpha[j] - row_dot(i, j) / csg);
                double df2[KG];
#pragma unroll
                for (int k = 0; k < KG; ++k) {
                  const int kk = k0 + k < d ? k0 + k : d - 1;
                  const double df = xs[kk * n + i] - xs[kk * n + j];
                  df2[k] = df * df;
                }
#pragma unroll
                for (int qq = 0; qq < QG; ++qq) {
                  const int q = q0 + qq;
                  if (q >= K) break;
                  if constexpr (FAM) {
                    // a 1-D family: value and d / d theta_q of the component's correlation from the direct difference, as
                    // the generation phase forms its distance; the diagonal gives (1, 0)
                    const double h = xs[i] - xs[j];
                    const CorrGrad cg = family_corr_grad(a.fam.id, a.fam.nu, a.fam.norm, theta_to_rate(a.fam, th[q], q) * (h * h), th[q], q);
                    gs[qq] += m * cg.r;
                    hk[qq][0] += m * cg.dtheta;
                    continue;
                  }
                  double sd = 0.0;
                  for (int k = 0; k < d; ++k) sd = fma(xs[k * n + i] * th[q * d + k], xs[k * n + j], sd);
                  const double dist = (us[q * NP + i] + us[q * NP + j]) + (-2.0 * sd);
                  const double v = m * exp_small<true>(dist, etab);
                  gs[qq] += v;
#pragma unroll
                  for (int k = 0; k < KG; ++k) hk[qq][k] = fma(v, df2[k], hk[qq][k]);
                }
              }
#pragma unroll
            for (int qq = 0; qq < QG; ++qq) {
              for (int off = 32; off > 0; off >>= 1) {
                gs[qq] += __shfl_xor(gs[qq], off, 64);
#pragma unroll
                for (int k = 0; k < KG; ++k) hk[qq][k] += __shfl_xor(hk[qq][k], off, 64);
              }
              if (lane64 == 0) {
                part[wv * kGradSlots + qq * (1 + KG)] = gs[qq];
#pragma unroll
                for (int k = 0; k < KG; ++k) part[wv * kGradSlots + qq * (1 + KG) + 1 + k] = hk[qq][k];
              }
            }
            mat_sync<G>();
            if (lt < QG * (1 + KG) && valid) {
              const int qq = lt / (1 + KG), slot = lt % (1 + KG), q = q0 + qq;
              const double tot = (part[lt] + part[kGradSlots + lt]) + (part[2 * kGradSlots + lt] + part[3 * kGradSlots + lt]);
              if constexpr (FIT) {
                // the row (1, theta): w = 1, and only the theta columns are wanted; they stay in LDS for thread 0
                if (q < K && slot != 0 && k0 + slot - 1 < d) fst[kFitGrad + k0 + slot - 1] = nograd ? kNaN : -s2g * tot;
              } else if (q < K) {
                const double wq = a.params[pb + (size_t)q * a.ldp];
                if (slot == 0) {
                  if (k0 == 0) a.grad[b + (size_t)q * a.Btot] = nograd ? kNaN : 2.0 * s2g * wq * tot;
                } else if (k0 + slot - 1 < d) {
                  // (a 1-D family's sum carries m d R_q / d theta_q itself: no minus sign)
                  a.grad[b + (size_t)(K + q * d + k0 + slot - 1) * a.Btot] = nograd ? kNaN : (FAM ? s2g : -s2g) * wq * wq * tot;
                }
              }
            }
            mat_sync<G>();
          }
        }
      };
      if constexpr (FAM) contract(std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{});   // d = 1
      else if (d <= 8) contract(std::integral_constant<int, 3>{}, std::integral_constant<int, 8>{});
      else contract(std::integral_constant<int, 1>{}, std::integral_constant<int, 16>{});
    } else if constexpr (INV == 4) {
      // ---- leave-one-out tables (ccgp_loo_batch; Dubrule 1983) ----------------------------------------------------------
      // Everything comes from the scaled Z already in LDS: g_i = (R^-1)_ii = row_dot(i, i), and (R^-1 1)_i, (R^-1 y)_i are
      // row i of Z against the two scaled right-hand-side columns, as alpha is formed for INV = 2.  One thread per training
      // point, each sum in index order; s11, beta and Q are the likelihood's own (slack).  O(n^2) after the factorisation.
      double* ry = zb;          // z_y d^-1/2 in place of z_y
      double* r1 = zb + NP;     // z_1 d^-1/2 in place of z_1
      for (int c = lt; c < NP; c += TPM) {
        const double sc = c < n ? dvec[c] : 0.0;
        ry[c] = c < n ? zb[c] * sc : 0.0;
        r1[c] = c < n ? zb[NP + c] * sc : 0.0;
      }
      mat_sync<G>();
      const double beta = slack[0], s11 = slack[1], Q = slack[3];
      const double s2 = a.vf.sigma2_row ? a.vf.sigma2_row[b] : a.sigma2;
      for (int i = lt; i < n; i += TPM) {
        const double g = row_dot(i, i);
        double v1 = 0.0, vy = 0.0;
        for (int c = i; c < n; ++c) {
          const double z = zmat[i * ZS + c];
          v1 = fma(z, r1[c], v1);
          vy = fma(z, ry[c], vy);
        }
        double mean, var;
        loo_point(a.vf.form, s2, a.y[i], g, v1, vy, s11, beta, Q, n, &mean, &var);
        if (bad) { mean = kNaN; var = kNaN; }
        if (valid) {
          a.mean[b + (size_t)i * a.S] = mean;
          a.var[b + (size_t)i * a.S] = var;
        }
      }
    } else {
      // ---- design gradient (entropy criteria, BSQ:856-948; the reference's optim() differences numerically) --------
      //   d log det R / d x_ik = -4 sum_{j != i} (R^-1)_ij (x_ik - x_jk) sum_q (w_q^2 / sw) theta_qk R_q,ij
      // for the free rows i >= n_fixed.  Per row, not a handful of scalars as in INV = 2, so the reduction is a TWO-PASS
      // split rather than LDS atomics: pass 1 forms every needed R^-1 entry once (the n-long dot product, the O(n^3)
      // part) and parks it in the part of Z that row_dot never reads; pass 2 gives each thread one (row, 8 dimensions)
      // and sums over j in a fixed order.  Atomic additions would make the bits depend on the order the waves arrive
      // in, and a design's result must not depend on what else is in the batch (the optimiser's starts are independent).
      //   where R^-1_ij (i > j) is parked: Z[i][j] for j <= i - 2 (row_dot reads row r from column 2 floor(r / 2) >= r - 1
      //   on), Z[i][NP] for j = i - 1 (the row's padding columns NP, NP + 1 are never read either)
      const int nf = a.n_fixed, nfree = n - nf;
      if (!bad)
        for (int idx = lt; idx < n * n; idx += TPM) {
          const int i = idx % n, j = idx / n;
          if (i <= j || i < nf) continue;   // (fixed, fixed) pairs feed no free row
          const double r = row_dot(i, j);
          zmat[i * ZS + (j + 1 == i ? NP : j)] = r;
        }
      mat_sync<G>();
      constexpr int KC = 8;
      const int nkc = (d + KC - 1) / KC;
      const double rsw = 1.0 / sw;   // the normalisation of R (HX:412)
      for (int item = lt; item < nfree * nkc; item += TPM) {
        const int i = nf + item % nfree, k0 = (item / nfree) * KC;
        double acc[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) acc[k] = 0.0;
        if (!bad)
          for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            const int hi = i > j ? i : j, lo = i > j ? j : i;
            const double rij = zmat[hi * ZS + (lo + 1 == hi ? NP : lo)];
            double df[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) {
              const int kk = k0 + k < d ? k0 + k : d - 1;
              df[k] = xs[kk * n + i] - xs[kk * n + j];
            }
            for (int q = 0; q < K; ++q) {
              double sd = 0.0;
              for (int k = 0; k < d; ++k) sd = fma(xs[k * n + hi] * th[q * d + k], xs[k * n + lo], sd);
              const double dist = (us[q * NP + hi] + us[q * NP + lo]) + (-2.0 * sd);
              const double v = rij * w2[q] * exp_small<true>(dist, etab);
#pragma unroll
              for (int k = 0; k < KC; ++k) {
                const int kk = k0 + k < d ? k0 + k : d - 1;
                acc[k] = fma(v * th[q * d + kk], df[k], acc[k]);
              }
            }
          }
        if constexpr (DFIT) {
          // the same values, in variable order, for thread 0
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k0 + k < d) dfs[kDfGrad + (i - nf) * d + k0 + k] = bad ? kNaN : -4.0 * rsw * acc[k];
        } else if (valid) {
          double* g = a.dgrad + (size_t)b * nfree * d;
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (k0 + k < d) g[(i - nf) + (size_t)(k0 + k) * nfree] = bad ? kNaN : -4.0 * rsw * acc[k];
        }
      }
      if constexpr (DFIT) {
        __syncthreads();   // log det and the gradient row are in LDS: thread 0 takes the step of design._Start.feed
        const DesignFitIO& df = a.dfit;
        const int nv = nfree * d;
        if (tid == 0) {
          double* sw_ = dfs + kDfGrad + nv;
          double* gx = dfs + kDfGrad;
          const double f = design_fit_value(dfs[kDfLd], df.ld_offset);
          for (int v = 0; v < nv; ++v) gx[v] = design_fit_grad(gx[v]);
          if (df.tr_f) {
            const size_t at = (size_t)b * df.T + dft;
            df.tr_f[at] = f;
            df.tr_status[at] = bad;
          }
          fit_feed(sw_, f, gx, bad == 0);
          const int go = sw_[kFitCode] == (double)kFitRunning && dft + 1 < df.max_evals[b] && dft + 1 < kDfMaxEvals;
          dfs[kDfGo] = go ? 1.0 : 0.0;
        }
        __syncthreads();
        const int go = __builtin_amdgcn_readfirstlane(dfs[kDfGo] != 0.0);
        dft += 1;
        dffail += bad != 0;
        if (go) goto chain_next;
        double* sg = df.state + (size_t)b * df.W;
        for (int e = tid; e < df.W; e += 256) sg[e] = dfs[kDfGrad + nv + e];
        if (tid == 0) { df.evals[b] = dft; df.nfail[b] = dffail; }
      }
    }
    if constexpr (FIT) {
      // the epilogue's last barrier has made ll and the gradient row visible: thread 0 takes the step of design._Start.feed
      const FitIO& fi = a.fit;
      if (tid == 0) {
        double* sw_ = fst + kFitState;
        const double* th_ = th;
        double gx[kMaxD];
        for (int k = 0; k < d; ++k) gx[k] = fit_grad(fst[kFitGrad + k], th_[k]);
        const double f = fit_value(fst[kFitLl]);
        if (fi.tr_f) {
          const size_t at = (size_t)b * fi.T + ft;
          fi.tr_f[at] = f;
          fi.tr_status[at] = bad;
        }
        fit_feed(sw_, f, gx, bad == 0);
        const int go = sw_[kFitCode] == (double)kFitRunning && ft + 1 < fi.max_evals[b] && ft + 1 < kFitMaxEvals;
        fst[kFitGo] = go ? 1.0 : 0.0;
      }
      __syncthreads();
      const int go = __builtin_amdgcn_readfirstlane(fst[kFitGo] != 0.0);
      ft += 1;
      ffail += bad != 0;
      if (go) goto chain_next;
      double* sg = fi.state + (size_t)b * fi.W;
      for (int e = tid; e < fi.W; e += 256) sg[e] = fst[kFitState + e];
      if (tid == 0) { fi.evals[b] = ft; fi.nfail[b] = ffail; }
    }
    return;
  }
  if constexpr (NE > 1) {
    // mean = beta + (z_y - beta z_1).w ,  var = sigma2 (1 - w.w + (1 - z_1.w)^2 / (z_1.z_1)),
    // dot products weighted by 1/d_k; w' = extra row of the test site (predict.post, HX:667-670)
    mat_sync<G>();
    const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
    double rd[NB];
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) {
      const int c = tx + G * bb;
      rd[bb] = (c < n && !bad) ? 1.0 / dvec[c] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      double ww = 0.0, z1w = 0.0, zyw = 0.0;
#pragma unroll
      for (int bb = 0; bb < NB; ++bb) {
        const int c = tx + G * bb;
        if (c < n) {
          const double w = E[e][bb], wr = w * rd[bb];
          ww = fma(w, wr, ww);
          z1w = fma(zb[NP + c], wr, z1w);
          zyw = fma(zb[c], wr, zyw);
        }
      }
      const int ridx = ty + G * e;
      psum[(0 * XR + ridx) * G + tx] = ww;
      psum[(1 * XR + ridx) * G + tx] = z1w;
      psum[(2 * XR + ridx) * G + tx] = zyw;
    }
    mat_sync<G>();
    const double beta = slack[0], s11 = slack[1], Q = slack[3];
    const double s2 = a.vf.sigma2_row ? a.vf.sigma2_row[b] : a.sigma2;
    for (int ridx = 2 + lt; ridx < XR; ridx += TPM) {
      const int t = t0 + ridx - 2;
      if (t >= a.m || !valid) continue;
      double ww = 0.0, z1w = 0.0, zyw = 0.0;
#pragma unroll
      for (int x = 0; x < G; ++x) {
        ww += psum[(0 * XR + ridx) * G + x];
        z1w += psum[(1 * XR + ridx) * G + x];
        zyw += psum[(2 * XR + ridx) * G + x];
      }
      const double u = 1.0 - z1w;
      double mean = beta + (zyw - beta * z1w);
      double var = predict_variance(a.vf.form, s2, ww, u, s11, Q, n);
      if (bad) { mean = kNaN; var = kNaN; }
      a.mean[b + (size_t)t * a.S] = mean;
      a.var[b + (size_t)t * a.S] = var;
    }
  }
}

// calls f(std::integral_constant<int, I>{}) for the I in [Lo, Hi] nearest to v: a run-time block count picks the instance
template <int Lo, int Hi, class F>
void pick(int v, F&& f) {
  if constexpr (Lo == Hi) f(std::integral_constant<int, Lo>{});
  else if (v <= Lo) f(std::integral_constant<int, Lo>{});
  else pick<Lo + 1, Hi>(v, f);
}

// A launcher was handed a 1-D family at a shape no FAM instance is compiled for.  The routes never say so
// (small_family_fused_supported, small_layout.h); should one, nothing is launched and the call fails at its launch check --
// as a refused kernel attribute does -- instead of running the Gaussian kernel in the family's place.
void no_family_instance() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> guard(attr_mutex());
  std::string& slot = attr_errors()[dev & 63];
  if (!slot.empty()) return;
  slot = "small_reg.hip: no instance generates this kernel family at this shape";
  attr_error_mask().fetch_or(1ull << (dev & 63));
}

// the arguments every launcher shares: one design, profile-beta likelihood of draw 0 unless the launcher says otherwise
RegArgs reg_args(const double* X, int n, int d, const double* y, DrawView dv) {
  RegArgs a{};
  a.X = X; a.y = y; a.n = n; a.d = d; a.params = dv.params; a.ldp = dv.ldp; a.K = dv.K;
  a.draw0 = 0; a.B = 1; a.sigma2 = 1.0; a.mode = 0; a.tau2 = 0.0;
  return a;
}

template <int G, int NB, int NE = 1>
void launch_one(hipStream_t s, const RegArgs& a) {
  constexpr int MPW = 256 / (G * G);
  // the sets form keeps a design per matrix where a workgroup holds several matrices (G = 8), as the per-design form does
  const bool own_design = a.set ? MPW > 1 : a.x_stride != 0;
  const size_t lds = sizeof(double) * reg_lds_doubles(G, NB, NE, false, own_design, a.n, a.d, a.K);
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, false>, "small_reg_kernel");
    if constexpr (NE == 1) raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, true>, "small_reg_kernel<full>");
  });
  void (*kernel)(RegArgs) = small_reg_kernel<G, NB, NE, false>;
  if constexpr (NE == 1) {
    if (a.set) {   // the sets form of the same two instances (general, FULL): the FULL one where the single-set call takes it
      static unsigned long long sets_mask = 0;
      once_per_device(sets_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, false, 0, false, false, true>, "small_reg_kernel<sets>");
        raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, true, 0, false, false, true>, "small_reg_kernel<full, sets>");
      });
      if (a.n == G * NB) kernel = small_reg_kernel<G, NB, NE, true, 0, false, false, true>;
      else kernel = small_reg_kernel<G, NB, NE, false, 0, false, false, true>;
      if (a.fac) {   // the sets form of the instance that keeps its factor (ccgp_predict_batch_sets and its kin)
        static unsigned long long sets_fac_mask = 0;
        once_per_device(sets_fac_mask, [] {
          raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, false, 0, true, false, true>, "small_reg_kernel<fac, sets>");
        });
        kernel = small_reg_kernel<G, NB, NE, false, 0, true, false, true>;
      }
    } else if (a.fac) {   // the likelihood instantiation that keeps its factor for site_solve_kernel
      static unsigned long long fac_mask = 0;
      once_per_device(fac_mask, [] { raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, false, 0, true>, "small_reg_kernel<fac>"); });
      kernel = small_reg_kernel<G, NB, NE, false, 0, true>;
    } else if (a.s2hat) {   // sigma2 concentrated out: the same two instances (general, FULL) compiled with PROF
      static unsigned long long prof_mask = 0;
      once_per_device(prof_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, false, 0, false, true>, "small_reg_kernel<profiled>");
        raise_lds_limit((const void*)small_reg_kernel<G, NB, NE, true, 0, false, true>, "small_reg_kernel<full, profiled>");
      });
      if (a.n == G * NB && a.x_stride == 0) kernel = small_reg_kernel<G, NB, NE, true, 0, false, true>;
      else kernel = small_reg_kernel<G, NB, NE, false, 0, false, true>;
    } else if (a.n == G * NB && a.x_stride == 0) {
      kernel = small_reg_kernel<G, NB, NE, true>;
    }
  }
  if (a.fam.id != 0) {   // a 1-D family (CCGP_OPT_FAMILY_FUSED): the general instance compiled with FAM, single-set or sets form
    if constexpr (NE == 1 && G * NB <= kFamilyFusedMaxN) {
      static unsigned long long fam_mask = 0;
      once_per_device(fam_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<G, NB, 1, false, 0, false, false, false, false, false, false, false, true>, "small_reg_kernel<family>");
        raise_lds_limit((const void*)small_reg_kernel<G, NB, 1, false, 0, false, false, true, false, false, false, false, true>, "small_reg_kernel<family, sets>");
      });
      if (a.set) kernel = small_reg_kernel<G, NB, 1, false, 0, false, false, true, false, false, false, false, true>;
      else kernel = small_reg_kernel<G, NB, 1, false, 0, false, false, false, false, false, false, false, true>;
      if (a.fac && !a.set) {   // CCGP_OPT_FAMILY_FUSED_PREDICT: the instance that keeps its factor for site_solve_kernel
        static unsigned long long fam_fac_mask = 0;
        once_per_device(fam_fac_mask, [] {
          raise_lds_limit((const void*)small_reg_kernel<G, NB, 1, false, 0, true, false, false, false, false, false, false, true>, "small_reg_kernel<family, fac>");
        });
        kernel = small_reg_kernel<G, NB, 1, false, 0, true, false, false, false, false, false, false, true>;
      }
      if (a.s2hat && !a.set && !a.fac) {   // CCGP_OPT_FAMILY_FUSED_GRAD: sigma2 concentrated out, value only
        static unsigned long long fam_prof_mask = 0;
        once_per_device(fam_prof_mask, [] {
          raise_lds_limit((const void*)small_reg_kernel<G, NB, 1, false, 0, false, true, false, false, false, false, false, true>, "small_reg_kernel<family, profiled>");
        });
        kernel = small_reg_kernel<G, NB, 1, false, 0, false, true, false, false, false, false, false, true>;
      }
    } else {
      no_family_instance();
      return;
    }
  }
  const int chunks = NE > 1 ? (a.m + (G * NE - 2) - 1) / (G * NE - 2) : 1;
  const int kMaxGrid = 1 << 20;
  RegArgs c = a;
  for (int b0 = 0; b0 < a.B; b0 += kMaxGrid * MPW) {
    c.draw0 = a.draw0 + b0;
    c.B = a.B - b0 < kMaxGrid * MPW ? a.B - b0 : kMaxGrid * MPW;
    hipLaunchKernelGGL(kernel, dim3((c.B + MPW - 1) / MPW, chunks), dim3(256), lds, s, c);
  }
}


// ---- prediction from the kept factor: lane = test site ---------------------------------------------------------------
struct SiteArgs {
  const double* fac;       // ns blocks of fac_stride doubles (FacLayout)
  size_t fac_stride;
  const double* X;         // n x d, column-major
  const double* params;    // draws, column-major with leading dimension ldp
  int ldp;
  int n, d, K;
  const double* Xt;        // m x d, column-major
  int m, S, draw0;         // this launch serves draws draw0 .. of the S x m tables; fac / rs are indexed from 0
  double sigma2;
  double* mean;
  double* var;
  double* rs;              // per (draw, 64-site batch) NPF x 64 doubles: the correlation vectors, lane-major
  int nbatch, npf;         // ceil(m / 64); n rounded up to a multiple of 8
  VarForm vf;              // per-draw sigma2 indexed by the global draw (nullptr: sigma2), the variance form; Q comes from the factor header
  const int* set;          // site_corr_kernel<K, true>: draw gb belongs to training set set[gb]: X + set[gb] n d, Xt + set[gb] m d
};

// r_i(x_t) = Mixed.corr.vec (HX:425-431) in corr.vec's operation order (HX:373: (theta'x^2 - 2 X Theta x) + u_i) for one draw and
// up to four batches of 64 test sites (one wave each): the scaled training coordinates x_ik theta_qk and u_qi = sum_k theta_qk
// x_ik^2 are formed once per workgroup in LDS and read by broadcast; a lane's site coordinates sit in LDS too ([k][lane]).
// Needs nothing from the factorisation: runs beside it.
// SETS (ccgp_predict_batch_sets and its kin): the draw's design and test sites are those of its training set; a template
// parameter, not a branch, as in small_reg_kernel: the single-set instance compiles from unchanged code, and the arithmetic
// per (draw, site) and its order are the same.  site_solve_kernel reads neither and serves both forms as it is.
template <int KC, bool SETS = false>
__global__ __launch_bounds__(256, 4) void site_corr_kernel(SiteArgs a) {
  constexpr int RB = 8;
  typedef double d2v __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, nbatch = a.nbatch, npf = a.npf;
  const int batch = blockIdx.x * (nthr >> 6) + wave;
  const int n = a.n, d = a.d, m = a.m, gb = a.draw0 + b;
  if constexpr (SETS) {
    const int st = __builtin_amdgcn_readfirstlane(a.set[gb]);   // uniform over the workgroup: the addresses stay scalar
    a.X += (size_t)st * n * d;
    a.Xt += (size_t)st * m * d;
  }
  const SiteCorrCarve cv(npf, d, KC, nthr >> 6);
  double *th = smem + cv.th, *w2 = smem + cv.w2, *us = smem + cv.us, *xs = smem + cv.xs;
  double* xw = smem + cv.xw + (size_t)wave * d * 64; // this wave's test sites, [k][lane]
  for (int e = tid; e < KC * d; e += nthr) th[e] = a.params[gb + (size_t)(KC + e) * a.ldp];
  if (tid < KC) { const double w = a.params[gb + (size_t)tid * a.ldp]; w2[tid] = w * w; }
  const int t = batch * 64 + lane;
  const int tc = t < m ? t : m - 1;                  // lanes beyond m compute a valid site; nobody reads their column
  if (batch < nbatch)
    for (int k = 0; k < d; ++k) xw[k * 64 + lane] = a.Xt[tc + (size_t)k * m];
  __syncthreads();
  for (int e = tid; e < KC * d * npf; e += nthr) {
    const int i = e % npf, qk = e / npf;             // qk = q * d + k
    xs[e] = i < n ? a.X[i + (size_t)(qk % d) * n] * th[qk] : 0.0;
  }
  for (int e = tid; e < KC * n; e += nthr) {
    const int c = e / n, i = e % n;
    double s = 0.0;
    for (int k = 0; k < d; ++k) { const double v = a.X[i + (size_t)k * n]; s += v * v * th[c * d + k]; }
    us[c * npf + i] = s;
  }
  __syncthreads();
  if (batch >= nbatch) return;
  double sw = 0.0;
  for (int c = 0; c < KC; ++c) sw += w2[c];
  double* __restrict__ rs = a.rs + ((size_t)b * nbatch + batch) * npf * 64 + lane;
  const double* xl = xw + lane;
  double ut[KC];
#pragma unroll
  for (int q = 0; q < KC; ++q) {
    double sq = 0.0;
    for (int k = 0; k < d; ++k) { const double v = xl[k * 64]; sq += v * v * th[q * d + k]; }
    ut[q] = sq;
  }
  for (int i0 = 0; i0 < n; i0 += RB) {
    double sd[KC][RB];
#pragma unroll
    for (int q = 0; q < KC; ++q)
#pragma unroll
      for (int j = 0; j < RB; ++j) sd[q][j] = 0.0;
    double xn = xl[0];
    for (int k = 0; k < d; ++k) {
      const double x = xn;
      xn = xl[(k + 1 < d ? k + 1 : k) * 64];         // the next dimension's coordinate is under way during this one's FMAs
#pragma unroll
      for (int q = 0; q < KC; ++q) {
        const d2v* xv = reinterpret_cast<const d2v*>(xs + (size_t)(q * d + k) * npf + i0);
        const d2v v0 = xv[0], v1 = xv[1], v2 = xv[2], v3 = xv[3];
        sd[q][0] = fma(v0[0], x, sd[q][0]); sd[q][1] = fma(v0[1], x, sd[q][1]);
        sd[q][2] = fma(v1[0], x, sd[q][2]); sd[q][3] = fma(v1[1], x, sd[q][3]);
        sd[q][4] = fma(v2[0], x, sd[q][4]); sd[q][5] = fma(v2[1], x, sd[q][5]);
        sd[q][6] = fma(v3[0], x, sd[q][6]); sd[q][7] = fma(v3[1], x, sd[q][7]);
      }
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      if (i0 + j < n) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < KC; ++q) {
          const double dist = (ut[q] - 2.0 * sd[q][j]) + us[q * npf + i0 + j];
          acc = fma(w2[q], exp_small_ranged<true>(dist, nullptr), acc);   // a cross vector passes no pivot test
        }
        rs[(size_t)(i0 + j) * 64] = acc / sw;
      }
    }
  }
}

// The 1-D families' counterpart (CCGP_OPT_FAMILY_FUSED_PREDICT; d = 1): the same rs layout -- per (draw, batch of 64 sites)
// npf x 64 doubles, row i at stride 64, lane = site -- with the entries cov_kernel<1> forms for a cross block: per component q
// ascending, rate_q = theta_to_rate(theta_q), h = x_t - x_i from the direct difference, fma(w_q^2, corr(rate_q (h h)), acc);
// then acc / sum w^2 as site_corr_kernel divides, or, under the two-family kernel, acc as it is (corr.vec.combined never
// divides, D1F:479: cov.hip's raw_mix).  An entry costs the Matern quadrature (130 - 190 terms of three exp each), so the
// mapping spreads ENTRIES, not sites: one wave = one (draw, site batch, training row i), four rows per workgroup, grid
// (nbatch ceil(n / 4), draws) -- all n rows on one wave would leave a single-model call (S = 1, m = 50) as one wave running
// n K quadratures in sequence.  The parameters are wave-uniform reads of the draw's row.  family_corr is the body the matrix
// entries call: cross entries and matrix entries share one compiled quadrature.  Lanes with t >= m compute a valid site that
// nobody reads; rows n .. npf - 1 are not written (site_solve_kernel masks them).  No LDS, no barrier; every loop is bounded
// (K <= 3 components, matern_corr's 6000-term cap).  Needs nothing from the factorisation: runs beside it.
__global__ __launch_bounds__(256) void site_corr_family_kernel(SiteArgs a, KernelFamily fam) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = a.n, m = a.m, K = a.K, nbatch = a.nbatch, npf = a.npf;
  const int nrb = (n + 3) / 4;                       // groups of four training rows
  const int batch = blockIdx.x / nrb, i = (blockIdx.x % nrb) * 4 + wave;
  const int b = blockIdx.y, gb = a.draw0 + b;
  if (i >= n || batch >= nbatch) return;             // (wave-uniform; nothing below waits for another wave)
  const int t = batch * 64 + lane;
  const int tc = t < m ? t : m - 1;
  const double h = a.Xt[tc] - a.X[i];
  const double h2 = h * h;
  double sw = 0.0, acc = 0.0;
  for (int q = 0; q < K; ++q) {
    const double w = a.params[gb + (size_t)q * a.ldp];
    sw += w * w;
  }
  for (int q = 0; q < K; ++q) {
    const double w = a.params[gb + (size_t)q * a.ldp];
    const double rate = theta_to_rate(fam, a.params[gb + (size_t)(K + q) * a.ldp], q);
    acc = fma(w * w, family_corr(fam.id, fam.nu, fam.norm, rate * h2, q), acc);
  }
  a.rs[(((size_t)b * nbatch + batch) * npf + i) * 64 + lane] = fam.id == CCGP_KERNEL_MATERN_SPLINE ? acc : acc / sw;
}

// One workgroup per (draw, group of up to four batches of 64 test sites), one wave per batch.  The draw's factor block comes
// into LDS once per workgroup (one linear coalesced stream; L' re-laid by row blocks) and every factor operand is then a
// broadcast LDS read.  [A first version read them through scalar loads, one SGPR operand per FMA: 153 us per Ground-Vibrations
// set at n = 50 against 181 for the extra-row scheme -- 10 - 37 KB of L' per wave through a scalar cache that a CU's waves share
// is a latency chain, not a stream.]  Fully unrolled so that w' lives in registers with static indices:
// w'_i = r_i - sum_{k<i} L'_ik w'_k, one accumulator per row, ascending k as the rank-1 updates of the extra-row scheme applied
// them; eight rows at a time: their sums over the finished columns are eight independent chains, then the block's own triangle
// row by row.  Then the three D-weighted dot products in that scheme's summation order (per column class x = c mod GS, classes
// in ascending order; GS = 8 for n <= 64, 16 above: the thread grids the extra rows were spread over): the bits of rounds 2 - 4.
template <int NPF>
__global__ __launch_bounds__(256, NPF <= 48 ? 3 : 2) void site_solve_kernel(SiteArgs a) {
  constexpr int NBL = NPF / 8;
  constexpr int GS = NPF <= 64 ? 8 : 16;
  typedef double d2v __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, nbatch = a.nbatch;
  const int batch = blockIdx.x * (nthr >> 6) + wave;
  const int n = a.n, m = a.m;
  const FacLayout fl(n);
  const double* __restrict__ Fg = a.fac + (size_t)b * a.fac_stride;
  const SiteSolveCarve cv(n);
  double *F = smem + cv.F, *L = smem + cv.L;                     // the block's head as it is in HBM, and L' in row blocks of 8
  for (int e = tid; e < fl.head; e += nthr) F[e] = Fg[e];
  {
    // L' arrives as one linear, coalesced stream (four loads in flight per thread); a thread finds the column of its
    // element by walking the column starts forward
    const double* __restrict__ Lg = Fg + fl.L;
    const int total = n * (n - 1) / 2;
    int k = 0, cs = 0, len = n - 1;                  // column k holds rows k + 1 .. n - 1 at [cs, cs + len)
    for (int e0 = tid; e0 < total; e0 += 4 * nthr) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = e0 + u * nthr < total ? Lg[e0 + u * nthr] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * nthr;
        if (e < total) {
          while (e >= cs + len) { cs += len; --len; ++k; }
          const int i = k + 1 + (e - cs), I = i >> 3, j = i & 7;
          L[k < 8 * I ? lrect(I, k, j) : ltri(I, j, k - 8 * I)] = v[u];
        }
      }
    }
  }
  __syncthreads();
  if (batch >= nbatch) return;
  const int t = batch * 64 + lane;
  const double* __restrict__ rs = a.rs + ((size_t)b * nbatch + batch) * NPF * 64 + lane;

  double w[NPF];
  // the next row block's correlation entries are requested a block ahead where the registers allow (w alone is 2 NPF of them);
  // the scheduling barriers keep the compiler from hoisting every block's loads to the top (1.1 KB of scratch per lane at NPF = 96)
  constexpr bool AHEAD = NPF <= 56;
  double nxt[8];
  if constexpr (AHEAD) {
#pragma unroll
    for (int j = 0; j < 8; ++j) nxt[j] = j < n ? rs[(size_t)j * 64] : 0.0;
  }
#pragma unroll
  for (int I = 0; I < NBL; ++I) {
    double acc[8];
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (AHEAD) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = nxt[j];
      if (I + 1 < NBL) {
#pragma unroll
        for (int j = 0; j < 8; ++j) nxt[j] = (8 * (I + 1) + j < n) ? rs[(size_t)(8 * (I + 1) + j) * 64] : 0.0;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = (8 * I + j < n) ? rs[(size_t)(8 * I + j) * 64] : 0.0;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (8 * I < n) {
      // column k + 1's four ds_read_b128 are issued before column k's eight FMAs, and no further: left alone the scheduler
      // hoists the reads of dozens of columns and spills w
      d2v v0, v1, v2, v3;
      if (I > 0) {
        const d2v* c = reinterpret_cast<const d2v*>(L + lrect(I, 0, 0));
        v0 = c[0]; v1 = c[1]; v2 = c[2]; v3 = c[3];
      }
#pragma unroll
      for (int k = 0; k < 8 * I; ++k) {
        d2v n0 = v0, n1 = v1, n2 = v2, n3 = v3;
        if (k + 1 < 8 * I) {
          const d2v* c = reinterpret_cast<const d2v*>(L + lrect(I, k + 1, 0));
          n0 = c[0]; n1 = c[1]; n2 = c[2]; n3 = c[3];
        }
        const double wk = -w[k];
        acc[0] = fma(wk, v0[0], acc[0]); acc[1] = fma(wk, v0[1], acc[1]);
        acc[2] = fma(wk, v1[0], acc[2]); acc[3] = fma(wk, v1[1], acc[3]);
        acc[4] = fma(wk, v2[0], acc[4]); acc[5] = fma(wk, v2[1], acc[5]);
        acc[6] = fma(wk, v3[0], acc[6]); acc[7] = fma(wk, v3[1], acc[7]);
        __builtin_amdgcn_sched_barrier(0);
        v0 = n0; v1 = n1; v2 = n2; v3 = n3;
      }
#pragma unroll
      for (int j = 1; j < 8; ++j)
#pragma unroll
        for (int c = 0; c < j; ++c) acc[j] = fma(-acc[c], L[ltri(I, j, c)], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) w[8 * I + j] = (8 * I + j < n) ? acc[j] : 0.0;
  }

  double ww = 0.0, z1w = 0.0, zyw = 0.0;
#pragma unroll
  for (int x = 0; x < GS; ++x) {
    double pw = 0.0, p1 = 0.0, py = 0.0;
#pragma unroll
    for (int c = x; c < NPF; c += GS) {
      if (c < n) {
        const double wc = w[c], wr = wc * F[fl.rd + c];
        pw = fma(wc, wr, pw);
        p1 = fma(F[fl.z1 + c], wr, p1);
        py = fma(F[fl.zy + c], wr, py);
      }
    }
    ww += pw;
    z1w += p1;
    zyw += py;
  }
  if (t >= m) return;
  const double beta = F[0], s11 = F[1];
  const double u = 1.0 - z1w;
  double mean = beta + (zyw - beta * z1w);
  const double s2 = a.vf.sigma2_row ? a.vf.sigma2_row[a.draw0 + b] : a.sigma2;
  double var = predict_variance(a.vf.form, s2, ww, u, s11, F[4], n);
  if (F[2] != 0.0) mean = var = __longlong_as_double(0x7ff8000000000000LL);
  a.mean[(a.draw0 + b) + (size_t)t * a.S] = mean;
  a.var[(a.draw0 + b) + (size_t)t * a.S] = var;
}

static dim3 site_grid(int nbatch, int ns, int* wpb) {
  *wpb = nbatch < 4 ? nbatch : 4;                                  // waves (site batches) per workgroup
  return dim3((nbatch + *wpb - 1) / *wpb, ns);
}
static void launch_site_corr(hipStream_t s, const SiteArgs& a, int ns, const KernelFamily& fam) {
  if (fam.id != 0) {   // a 1-D family: one wave per (draw, site batch, training row)
    hipLaunchKernelGGL(site_corr_family_kernel, dim3((unsigned)a.nbatch * (unsigned)((a.n + 3) / 4), ns), dim3(256), 0, s, a, fam);
    return;
  }
  int wpb;
  const dim3 grid = site_grid(a.nbatch, ns, &wpb), block(64 * wpb);
  const size_t lds = sizeof(double) * SiteCorrCarve(a.npf, a.d, a.K, wpb).total;
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)site_corr_kernel<1>, "site_corr_kernel");
    raise_lds_limit((const void*)site_corr_kernel<2>, "site_corr_kernel");
    raise_lds_limit((const void*)site_corr_kernel<3>, "site_corr_kernel");
  });
  if (a.set) {
    static unsigned long long sets_mask = 0;
    once_per_device(sets_mask, [] {
      raise_lds_limit((const void*)site_corr_kernel<1, true>, "site_corr_kernel<sets>");
      raise_lds_limit((const void*)site_corr_kernel<2, true>, "site_corr_kernel<sets>");
      raise_lds_limit((const void*)site_corr_kernel<3, true>, "site_corr_kernel<sets>");
    });
    if (a.K == 1) hipLaunchKernelGGL((site_corr_kernel<1, true>), grid, block, lds, s, a);
    else if (a.K == 2) hipLaunchKernelGGL((site_corr_kernel<2, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((site_corr_kernel<3, true>), grid, block, lds, s, a);
    return;
  }
  if (a.K == 1) hipLaunchKernelGGL(site_corr_kernel<1>, grid, block, lds, s, a);
  else if (a.K == 2) hipLaunchKernelGGL(site_corr_kernel<2>, grid, block, lds, s, a);
  else hipLaunchKernelGGL(site_corr_kernel<3>, grid, block, lds, s, a);
}
static void launch_site_solve(hipStream_t s, const SiteArgs& a, int ns) {
  int wpb;
  const dim3 grid = site_grid(a.nbatch, ns, &wpb), block(64 * wpb);
  pick<1, 13>(a.npf / 8, [&](auto nbl) {
    constexpr int NPF = 8 * decltype(nbl)::value;
    static unsigned long long attr_mask = 0;
    once_per_device(attr_mask, [] { raise_lds_limit((const void*)site_solve_kernel<NPF>, "site_solve_kernel"); });
    hipLaunchKernelGGL(site_solve_kernel<NPF>, grid, block, sizeof(double) * SiteSolveCarve(a.n).total, s, a);
  });
}

// ---- explicit inverse of ONE draw's matrix (solve(R), HX:454), gradient, design gradient: one workgroup per matrix ------
template <int NB, int INV, bool PROF = false, bool SETS = false>
static void launch_inv(hipStream_t s, const RegArgs& a) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)small_reg_kernel<16, NB, NB + 1, false, INV, false, PROF, SETS>,
                    INV == 1 ? "small_reg_kernel<inverse>" : INV == 2 ? "small_reg_kernel<gradient>" :
                    INV == 3 ? "small_reg_kernel<design gradient>" : "small_reg_kernel<leave-one-out>");
  });
  const size_t lds = sizeof(double) * reg_lds_doubles(16, NB, NB + 1, true, a.x_stride != 0, a.n, a.d, a.K);
  void (*kernel)(RegArgs) = small_reg_kernel<16, NB, NB + 1, false, INV, false, PROF, SETS>;
  if (a.fam.id != 0) {   // a 1-D family (CCGP_OPT_FAMILY_FUSED_PREDICT): the leave-one-out instance compiled with FAM
    if constexpr (INV == 4 && !PROF && !SETS && 16 * NB <= kFamilyFusedMaxN) {
      static unsigned long long fam_mask = 0;
      once_per_device(fam_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<16, NB, NB + 1, false, 4, false, false, false, false, false, false, false, true>,
                        "small_reg_kernel<family, leave-one-out>");
      });
      kernel = small_reg_kernel<16, NB, NB + 1, false, 4, false, false, false, false, false, false, false, true>;
    } else if constexpr (INV == 2 && (PROF || !SETS) && 16 * NB <= kFamilyFusedMaxN) {
      // CCGP_OPT_FAMILY_FUSED_GRAD: the gradient instance (plain, profiled, profiled over sets) compiled with FAM
      static unsigned long long fam_mask = 0;
      once_per_device(fam_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<16, NB, NB + 1, false, 2, false, PROF, SETS, false, false, false, false, true>,
                        "small_reg_kernel<family, gradient>");
      });
      kernel = small_reg_kernel<16, NB, NB + 1, false, 2, false, PROF, SETS, false, false, false, false, true>;
    } else {
      no_family_instance();
      return;
    }
  }
  const int kMaxGrid = 1 << 20;
  RegArgs c = a;
  for (int b0 = 0; b0 < a.B; b0 += kMaxGrid) {
    c.draw0 = a.draw0 + b0;
    c.B = a.B - b0 < kMaxGrid ? a.B - b0 : kMaxGrid;
    hipLaunchKernelGGL(kernel, dim3(c.B, 1), dim3(256), lds, s, c);
  }
}
template <int INV, bool PROF = false, bool SETS = false>
static void dispatch_inv(hipStream_t s, const RegArgs& a) {
  pick<1, 8>((a.n + 15) / 16, [&](auto nb) { launch_inv<decltype(nb)::value, INV, PROF, SETS>(s, a); });
}

template <int NE = 1>
static void dispatch(hipStream_t s, const RegArgs& a) {
  const int n = a.n;
  // A handful of evaluations (Metro's one proposal per logpost call, a speculative batch of a few candidates) is a
  // LATENCY problem: one wave per matrix leaves the chip empty and runs the whole elimination on 64 lanes; the
  // 16 x 16 grid puts four waves on each matrix (n = 64, one evaluation: 41 -> 25 us of kernel time).
  // (with the factor kept -- prediction -- the four-wave form up to 2048 draws: its one factorisation per draw is the critical
  // path of the call and a wave per SIMD is all that 1000 draws fill anyway)
  const bool wide = NE == 1 && a.x_stride == 0 && a.B <= (a.fac ? CCGP_FAC_WIDE_MAX : 64);
  if constexpr (NE == 1) {
    // 64 < n <= 104 (BASELINE config 3: maximin-100): still ONE WAVE per matrix on the 8 x 8 grid, with up to 13 x 13
    // blocks per thread (two waves per SIMD: up to 256 VGPRs) -- at n = 100 1.68 x the minimal FMAs instead of the
    // 2.75 x of the 16 x 16 grid at NB = 7, no s_barrier, and the per-column overhead (pivot, reciprocal, column
    // broadcast) is paid by one wave instead of four: 25.7 k -> ~10 k VALU instructions per evaluation, 6.06 -> 5.07 ms
    // per 103 680 evaluations on the same box, same bits (profiles/r04).  CCGP_OPT_SMALL_GRID16: the 16 x 16 grid (A/B).
    if (n > 64 && n <= 104 && !wide && small_reg_fits8(n, a.d, a.K, a.x_stride != 0) && !a.grid16) {
      pick<9, 13>((n + 7) / 8, [&](auto nb) { launch_one<8, decltype(nb)::value, NE>(s, a); });
      return;
    }
  }
  if (n <= 64 && !wide) pick<1, 8>((n + 7) / 8, [&](auto nb) { launch_one<8, decltype(nb)::value, NE>(s, a); });
  // (the prediction instances only come here with n > 64)
  else pick<(NE == 1 ? 1 : 5), 8>((n + 15) / 16, [&](auto nb) { launch_one<16, decltype(nb)::value, NE>(s, a); });
}

// The sets form's grid (small_reg_sets_grid, small_layout.h): a lockstep step of a few dozen matrices is the latency case of
// dispatch() above and takes four waves per matrix; a larger call takes one wave per matrix up to 13 x 13 blocks.
static void dispatch_sets(hipStream_t s, const RegArgs& a) {
  const int n = a.n;
  if (small_reg_sets_grid(n, a.d, a.K, a.B) == 8) {
    if (n <= 64) pick<1, 8>((n + 7) / 8, [&](auto nb) { launch_one<8, decltype(nb)::value, 1>(s, a); });
    else pick<9, 13>((n + 7) / 8, [&](auto nb) { launch_one<8, decltype(nb)::value, 1>(s, a); });
    return;
  }
  pick<1, 8>((n + 15) / 16, [&](auto nb) { launch_one<16, decltype(nb)::value, 1>(s, a); });
}

// the chain instances: the sets likelihood instance of the 16 x 16 grid (general, FULL) compiled with CHAIN, one workgroup
// per chain, the chain's words behind the instance's carve
template <int NB>
static void launch_chain(hipStream_t s, const RegArgs& a) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)small_reg_kernel<16, NB, 1, false, 0, false, false, true, true>, "small_reg_kernel<chain>");
    raise_lds_limit((const void*)small_reg_kernel<16, NB, 1, true, 0, false, false, true, true>, "small_reg_kernel<full, chain>");
  });
  const size_t lds = sizeof(double) * reg_chain_lds_doubles(NB, a.n, a.d, a.K);
  void (*kernel)(RegArgs) = small_reg_kernel<16, NB, 1, false, 0, false, false, true, true>;
  if (a.n == 16 * NB) kernel = small_reg_kernel<16, NB, 1, true, 0, false, false, true, true>;
  if (a.fam.id != 0) {   // a 1-D family: the general chain instance compiled with FAM
    if constexpr (16 * NB <= kFamilyFusedMaxN) {
      static unsigned long long fam_mask = 0;
      once_per_device(fam_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<16, NB, 1, false, 0, false, false, true, true, false, false, false, true>, "small_reg_kernel<family, chain>");
      });
      kernel = small_reg_kernel<16, NB, 1, false, 0, false, false, true, true, false, false, false, true>;
    } else {
      no_family_instance();
      return;
    }
  }
  hipLaunchKernelGGL(kernel, dim3(a.B, 1), dim3(256), lds, s, a);
}

// the search instances: the chain instances compiled with NM, one workgroup per search, the search's words behind the chain's
template <int NB>
static void launch_nm(hipStream_t s, const RegArgs& a) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)small_reg_kernel<16, NB, 1, false, 0, false, false, true, true, false, true>, "small_reg_kernel<nm>");
    raise_lds_limit((const void*)small_reg_kernel<16, NB, 1, true, 0, false, false, true, true, false, true>, "small_reg_kernel<full, nm>");
  });
  const size_t lds = sizeof(double) * reg_nm_lds_doubles(NB, a.n, a.d, a.K);
  void (*kernel)(RegArgs) = small_reg_kernel<16, NB, 1, false, 0, false, false, true, true, false, true>;
  if (a.n == 16 * NB) kernel = small_reg_kernel<16, NB, 1, true, 0, false, false, true, true, false, true>;
  if (a.fam.id != 0) {   // a 1-D family: the general search instance compiled with FAM
    if constexpr (16 * NB <= kFamilyFusedMaxN) {
      static unsigned long long fam_mask = 0;
      once_per_device(fam_mask, [] {
        raise_lds_limit((const void*)small_reg_kernel<16, NB, 1, false, 0, false, false, true, true, false, true, false, true>, "small_reg_kernel<family, nm>");
      });
      kernel = small_reg_kernel<16, NB, 1, false, 0, false, false, true, true, false, true, false, true>;
    } else {
      no_family_instance();
      return;
    }
  }
  hipLaunchKernelGGL(kernel, dim3(a.B, 1), dim3(256), lds, s, a);
}

// the fit instances: the profiled-gradient sets instance compiled with FIT, one workgroup per start, the start's words behind
// the instance's carve
template <int NB>
static void launch_fit(hipStream_t s, const RegArgs& a) {
  static unsigned long long attr_mask = 0;
  void (*kernel)(RegArgs) = small_reg_kernel<16, NB, NB + 1, false, 2, false, true, true, false, true>;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)small_reg_kernel<16, NB, NB + 1, false, 2, false, true, true, false, true>, "small_reg_kernel<fit>");
  });
  const size_t lds = sizeof(double) * reg_fit_lds_doubles(NB, a.n, a.d);
  hipLaunchKernelGGL(kernel, dim3(a.B, 1), dim3(256), lds, s, a);
}

// the design-search instances: the design-gradient instance compiled with DFIT, one workgroup per start, the start's words
// behind the instance's per-design carve
template <int NB>
static void launch_dfit(hipStream_t s, const RegArgs& a) {
  static unsigned long long attr_mask = 0;
  void (*kernel)(RegArgs) = small_reg_kernel<16, NB, NB + 1, false, 3, false, false, false, false, false, false, true>;
  once_per_device(attr_mask, [] {
    raise_lds_limit((const void*)small_reg_kernel<16, NB, NB + 1, false, 3, false, false, false, false, false, false, true>,
                    "small_reg_kernel<design fit>");
  });
  const size_t lds = sizeof(double) * reg_design_fit_lds_doubles(NB, a.n, a.d, a.K, (a.n - a.n_fixed) * a.d);
  hipLaunchKernelGGL(kernel, dim3(a.B, 1), dim3(256), lds, s, a);
}

}  // namespace

// ccgp_design_fit where small_route_design_fit says Reg: A starts sharing the parameter row of dv and the fixed rows of io;
// arrays as DesignFitIO lays them out; every pointer a device pointer
void launch_small_reg_design_fit(hipStream_t s, int n, int d, DrawView dv, int n_fixed, int A, const DesignFitIO& io) {
  RegArgs a = reg_args(nullptr, n, d, nullptr, dv);   // no design array: the free rows come from the states
  a.B = A; a.x_stride = (size_t)n * d; a.shared_params = 1; a.n_fixed = n_fixed; a.dfit = io;
  pick<1, 8>((n + 15) / 16, [&](auto nb) { launch_dfit<decltype(nb)::value>(s, a); });
}

// ccgp_laplace_search_sets where small_route_nm says Reg: A searches, search a on training set set[a]; arrays as NmIO lays
// them out; every pointer a device pointer
void launch_small_reg_nm_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2,
                              const int* set, int A, const NmIO& io, KernelFamily fam) {
  DrawView dv{nullptr, A, 2, d, fam};
  RegArgs a = reg_args(Xs, n, d, ys, dv);
  a.B = A; a.set = set; a.sigma2_set = sigma2; a.nm = io; a.fam = fam;
  pick<1, 8>((n + 15) / 16, [&](auto nb) { launch_nm<decltype(nb)::value>(s, a); });
}

// ccgp_profile_fit_sets where small_route_fit says Reg: A starts, start a on training set set[a]; arrays as FitIO lays them
// out; every pointer a device pointer
void launch_small_reg_fit_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const int* set, int A,
                               const FitIO& io) {
  DrawView dv{nullptr, A, 1, d, KernelFamily{}};
  RegArgs a = reg_args(Xs, n, d, ys, dv);
  a.B = A; a.set = set; a.Btot = A; a.fit = io;
  pick<1, 8>((n + 15) / 16, [&](auto nb) { launch_fit<decltype(nb)::value>(s, a); });
}

// ccgp_metro_segments_sets where small_route_chain says Reg: A chains, chain a on training set set[a]; arrays as ChainIO
// lays them out (theta0 / theta_fin A x p column-major); every pointer a device pointer
void launch_small_reg_chain_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2,
                                 const int* set, int A, const ChainIO& io, KernelFamily fam) {
  DrawView dv{nullptr, A, 2, d, fam};
  RegArgs a = reg_args(Xs, n, d, ys, dv);
  a.B = A; a.set = set; a.sigma2_set = sigma2; a.ch = io; a.fam = fam;
  pick<1, 8>((n + 15) / 16, [&](auto nb) { launch_chain<decltype(nb)::value>(s, a); });
}

// ccgp_loglik_batch_sets where small_route_sets says Reg: the B rows of dv, row b on training set set[b] of the C sets at
// Xs (C blocks of n x d, column-major each), ys (C blocks of n) and sigma2 (C values)
void launch_small_reg_loglik_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2,
                                  const int* set, DrawView dv, int B, int mean_mode, double tau2, double* loglik,
                                  double* beta, int* status) {
  RegArgs a = reg_args(Xs, n, d, ys, dv);
  a.B = B; a.mode = mean_mode; a.tau2 = tau2; a.set = set; a.sigma2_set = sigma2;
  a.loglik = loglik; a.beta = beta; a.status = status; a.fam = dv.fam;
  dispatch_sets(s, a);
}

// ccgp_profile_batch_sets where small_route_profile_grad_sets says Reg: launch_small_reg_profile with a gradient, row b on
// training set set[b]; one workgroup per row, one launch
void launch_small_reg_profile_grad_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const int* set,
                                        DrawView dv, int B, double* loglik, double* s2hat, double* beta, double* grad,
                                        int* status) {
  RegArgs a = reg_args(Xs, n, d, ys, dv);
  a.B = B; a.set = set;
  a.loglik = loglik; a.beta = beta; a.status = status; a.s2hat = s2hat; a.grad = grad; a.Btot = B; a.fam = dv.fam;
  dispatch_inv<2, true, true>(s, a);
}

void launch_small_reg_inverse(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int draw,
                              double sigma2, double* Rinv, double* loglik, double* beta, int* status) {
  RegArgs a = reg_args(X, n, d, y, dv);
  a.draw0 = draw; a.sigma2 = sigma2;
  a.loglik = loglik; a.beta = beta; a.status = status; a.Rinv = Rinv;
  dispatch_inv<1>(s, a);
}

// d loglik / d params for B draws (ccgp_loglik_grad_batch, n <= 128): one workgroup per draw on the same scheme
void launch_small_reg_grad(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int B,
                           double sigma2, double* loglik, double* beta, double* grad, int* status) {
  RegArgs a = reg_args(X, n, d, y, dv);
  a.B = B; a.sigma2 = sigma2;
  a.loglik = loglik; a.beta = beta; a.status = status; a.grad = grad; a.Btot = B; a.fam = dv.fam;
  dispatch_inv<2>(s, a);
}

// the leave-one-out tables of B draws (ccgp_loo_batch, ccgp_loo_summary): one workgroup per draw, one launch
void launch_small_reg_loo(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int B, double sigma2,
                          VarForm vf, double* mean, double* var, double* beta, int* status) {
  RegArgs a = reg_args(X, n, d, y, dv);
  a.B = B; a.sigma2 = sigma2; a.vf = vf;
  a.beta = beta; a.status = status; a.mean = mean; a.var = var; a.S = B; a.fam = dv.fam;
  dispatch_inv<4>(s, a);
}

// ccgp_profile_batch at n <= 128: likelihood with sigma2 concentrated out, the draw's sigma2_hat, and (grad != nullptr) the
// gradient at (beta_hat, sigma2_hat), all from the one factorisation per draw of the instances above
void launch_small_reg_profile(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int B,
                              double* loglik, double* s2hat, double* beta, double* grad, int* status, bool grid16) {
  RegArgs a = reg_args(X, n, d, y, dv);
  a.B = B; a.loglik = loglik; a.beta = beta; a.status = status; a.s2hat = s2hat; a.fam = dv.fam;
  if (grad) {
    a.grad = grad; a.Btot = B;
    dispatch_inv<2, true>(s, a);
  } else {
    a.grid16 = grid16;
    dispatch(s, a);
  }
}

// ccgp_family_corr_dtheta: the n x n table of d R_q / d theta_q, one thread per entry
void launch_family_dcorr(hipStream_t s, const double* x, int n, double theta, int q, KernelFamily fam, double* out) {
  const size_t entries = (size_t)n * n;
  hipLaunchKernelGGL(family_dcorr_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, x, n, theta, q, fam, out);
}

// log det R_mixed for B candidate designs (Xs = B blocks of n x d, column-major each) under ONE parameter row
static RegArgs design_args(const double* Xs, int n, int d, DrawView dv, int B, double* logdet, int* status) {
  RegArgs a = reg_args(Xs, n, d, Xs, dv);   // the right-hand-side rows are not used; any n readable doubles will do
  a.B = B; a.status = status; a.x_stride = (size_t)n * d; a.shared_params = 1; a.logdet = logdet;
  return a;
}

// d log det R_mixed / d X for B candidate designs sharing one parameter row (ccgp_mixed_logdet_grad_designs, n <= 128):
// one workgroup per design; log det as launch_small_reg_logdet_designs computes it, the gradient of rows >= n_fixed in dgrad
void launch_small_reg_logdet_grad_designs(hipStream_t s, const double* Xs, int n, int d, DrawView dv, int B, int n_fixed,
                                          double* logdet, double* dgrad, int* status) {
  RegArgs a = design_args(Xs, n, d, dv, B, logdet, status);
  a.dgrad = dgrad; a.n_fixed = n_fixed;
  dispatch_inv<3>(s, a);
}

void launch_small_reg_loglik(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv,
                             int B, double sigma2, int mean_mode, double tau2, double* loglik,
                             double* beta, int* status, bool grid16) {
  RegArgs a = reg_args(X, n, d, y, dv);
  a.B = B; a.sigma2 = sigma2; a.mode = mean_mode; a.tau2 = tau2;
  a.loglik = loglik; a.beta = beta; a.status = status; a.grid16 = grid16; a.fam = dv.fam;
  dispatch(s, a);
}

// Entropy = -det(R) (BSQ:856-861), Augmented.Mixed.Entropy = -det(R_all)/det(R_old) (BSQ:869-877, Schur complement)
void launch_small_reg_logdet_designs(hipStream_t s, const double* Xs, int n, int d, DrawView dv, int B,
                                     double* logdet, int* status) {
  dispatch(s, design_args(Xs, n, d, dv, B, logdet, status));
}

// predict.post for S draws x m test sites (mean / var are S x m column-major).  scratch (scratch_bytes, may be null): with at
// least small_reg_sites_scratch() bytes per draw of a chunk the kept-factor scheme runs (one factorisation per draw, then
// lane = test site); otherwise the extra-row scheme.
void launch_small_reg_predict(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv,
                              int S, const double* Xtest, int m, double sigma2, double* mean, double* var,
                              double* beta, int* status, void* scratch, size_t scratch_bytes, hipStream_t aux,
                              hipEvent_t ev_fork, hipEvent_t ev_join, VarForm vf) {
  RegArgs a = reg_args(X, n, d, y, dv);
  a.B = S; a.sigma2 = sigma2; a.vf = vf;
  a.beta = beta; a.status = status; a.Xt = Xtest; a.m = m; a.S = S; a.mean = mean; a.var = var; a.fam = dv.fam;
  const size_t per = small_reg_sites_scratch(n, d, dv.K, m);
  if (scratch && small_reg_sites_supported(n, d, dv.K) && scratch_bytes >= per) {
    const FacLayout fl(n);
    const int nbatch = (m + 63) / 64;
    const int chunk = (int)std::min<size_t>((size_t)S, std::min<size_t>(scratch_bytes / per, 32768));
    double* fac = static_cast<double*>(scratch);
    double* rs = fac + (size_t)chunk * fl.total;
    for (int s0 = 0; s0 < S; s0 += chunk) {
      const int ns = std::min(chunk, S - s0);
      SiteArgs sa{fac, (size_t)fl.total, X, dv.params, dv.ldp, n, d, dv.K, Xtest, m, S, s0, sigma2, mean, var, rs, nbatch, fl.npf, vf,
                  nullptr};
      // the correlation vectors need nothing from the factorisation: on the second stream beside it (the factorisation is ONE
      // wave per draw -- 1000 draws leave three quarters of the wave slots empty -- and runs at the latency of its n columns)
      if (aux && ev_fork && ev_join) {
        (void)hipEventRecord(ev_fork, s);
        (void)hipStreamWaitEvent(aux, ev_fork, 0);
        launch_site_corr(aux, sa, ns, dv.fam);
        (void)hipEventRecord(ev_join, aux);
      } else {
        launch_site_corr(s, sa, ns, dv.fam);
      }
      RegArgs f = a;
      f.Xt = nullptr; f.m = 0; f.mean = f.var = nullptr;
      f.draw0 = s0; f.B = ns;
      f.fac = fac - (size_t)s0 * fl.total;     // the kernel indexes the block by the draw's global number
      f.fac_stride = (size_t)fl.total;
      dispatch<1>(s, f);
      if (aux && ev_fork && ev_join) (void)hipStreamWaitEvent(s, ev_join, 0);
      launch_site_solve(s, sa, ns);
    }
    return;
  }
  // (a 1-D family never comes here: predict_run secures the scratch before it takes this route, and launch_one has no
  // extra-row instance to give it)
  dispatch<kPredictNE>(s, a);
}

// predict.post for B rows over C training sets of one shape in ONE set of launches per chunk of rows (ccgp_predict_batch_sets
// and its kin on the kept-factor scheme): row b on set set[b] -- design Xs + set[b] n d, responses ys + set[b] n, test sites
// Xtests + set[b] m d -- with its own sigma2 (vf.sigma2_row, indexed by the row; never null here).  mean / var are B x m
// column-major.  scratch holds small_reg_sites_scratch() bytes per row of a chunk, at least one row.  The launches are those
// of launch_small_reg_predict's kept-factor branch with the sets instances: factorisation (FAC + SETS), correlation vectors
// (site_corr_kernel<K, true>, beside it on the second stream) and site_solve_kernel as it is.
void launch_small_reg_predict_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2_set,
                                   const int* set, DrawView dv, int B, const double* Xtests, int m, double* mean, double* var,
                                   double* beta, int* status, void* scratch, size_t scratch_bytes, hipStream_t aux,
                                   hipEvent_t ev_fork, hipEvent_t ev_join, VarForm vf) {
  RegArgs a = reg_args(Xs, n, d, ys, dv);
  a.vf = vf; a.beta = beta; a.status = status; a.S = B; a.set = set; a.sigma2_set = sigma2_set;
  const size_t per = small_reg_sites_scratch(n, d, dv.K, m);
  const FacLayout fl(n);
  const int nbatch = (m + 63) / 64;
  const int chunk = (int)std::min<size_t>((size_t)B, std::min<size_t>(scratch_bytes / per, 32768));
  double* fac = static_cast<double*>(scratch);
  double* rs = fac + (size_t)chunk * fl.total;
  for (int s0 = 0; s0 < B; s0 += chunk) {
    const int ns = std::min(chunk, B - s0);
    SiteArgs sa{fac, (size_t)fl.total, Xs, dv.params, dv.ldp, n, d, dv.K, Xtests, m, B, s0, 1.0, mean, var, rs, nbatch, fl.npf, vf, set};
    if (aux && ev_fork && ev_join) {
      (void)hipEventRecord(ev_fork, s);
      (void)hipStreamWaitEvent(aux, ev_fork, 0);
      launch_site_corr(aux, sa, ns, dv.fam);
      (void)hipEventRecord(ev_join, aux);
    } else {
      launch_site_corr(s, sa, ns, dv.fam);
    }
    RegArgs f = a;
    f.draw0 = s0; f.B = ns;
    f.fac = fac - (size_t)s0 * fl.total;     // the kernel indexes the block by the row's global number
    f.fac_stride = (size_t)fl.total;
    dispatch_sets(s, f);
    if (aux && ev_fork && ev_join) (void)hipStreamWaitEvent(s, ev_join, 0);
    launch_site_solve(s, sa, ns);
  }
}

}  // namespace ccgp
