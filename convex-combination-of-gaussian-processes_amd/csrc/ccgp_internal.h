// Internal declarations shared by the HIP translation units of libccgp (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ccgp.h"
#include "exp_table.h"
#include "small_layout.h"   // kSmallMaxN, kMaxD, kMaxK, kLdsBytes, kExpTableDoubles; the small-n carves and route predicates

namespace ccgp {

constexpr int kTile = 128;       // block size of the blocked Cholesky (rows/cols per tile)

// When does a factorisation "fail" (status != 0, NaN -- the reference's NA)?
//   mean mode 1 (cond.like, HX:561-572): the reference only runs mnormt::dmnorm, whose chol() stops at a
//     NON-POSITIVE pivot -> threshold 0.
//   mean mode 0 (logpost, HX:454-460): the reference first calls solve(R), and base R's solve() refuses a matrix whose
//     reciprocal condition number is below .Machine$double.eps ("system is computationally singular") -> R.Inv <- NA.
//     The device has no condition estimate; it uses a necessary condition that comes for free: the correlation
//     matrix has a unit diagonal and its smallest LDL' pivot d_min bounds the smallest eigenvalue from above, so
//     d_min <= n eps  =>  cond_2(R) >= 1 / (n eps), and the 1-norm condition number LAPACK estimates can be n times
//     cond_2.  A pivot <= n * DBL_EPSILON therefore fails the evaluation.  (A threshold of eps alone is not enough: a
//     duplicated design point leaves a pivot of the size of the rounding error of an n-term sum of squares -- the
//     n = 300 matrix of tests/test_gpu_parity.py::test_non_positive_definite_maps_to_na passed a threshold of eps;
//     before round 3 the threshold was 0 here too, and such a matrix failed or "succeeded" depending on the sign of
//     that rounding error.)
constexpr double kSolvePivotEps = 2.220446049250313e-16;
__host__ __device__ inline double pivot_tolerance(int mean_mode, int n) { return mean_mode == 0 ? n * kSolvePivotEps : 0.0; }

}  // namespace ccgp

namespace ccgp {

// one timed launch group: events are recorded on the handle's stream and only read back
// (hipEventElapsedTime) in ccgp_get_timing, so timing never synchronises the pipeline.
struct TimedSpan {
  int id;
  hipEvent_t e0, e1;
};

// correlation family of the component GPs (ccgp_set_kernel)
struct KernelFamily {
  int id = 0;        // CCGP_KERNEL_GAUSS | CCGP_KERNEL_MATERN | CCGP_KERNEL_MATERN_SPLINE
  double nu = 0.0;   // Matern smoothness
  double norm = 0.0; // 1 / (Gamma(nu) 2^(nu-1))
};

}  // namespace ccgp

namespace ccgp {
constexpr int kPullSlices = 4;
struct Buffer {
  void* ptr = nullptr;
  size_t bytes = 0;
};
}

struct ccgp_handle {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  size_t ws_limit = size_t(24) << 30;   // ccgp_create replaces this by 3/4 of the device's memory
  int opt_small_grid16 = 0;             // CCGP_OPT_SMALL_GRID16
  int opt_predict_factor = 1;           // CCGP_OPT_PREDICT_FACTOR
  int opt_fuse_diag = 1;                // CCGP_OPT_FUSE_DIAG
  int opt_tail_strips = 1;              // CCGP_OPT_TAIL_STRIPS
  int opt_wide_offsets = 0;             // CCGP_OPT_WIDE_OFFSETS
  int opt_fused_solve = 1;              // CCGP_OPT_FUSED_SOLVE: 0 = update + trsm launches, 1 = diagonal launch + tiles solved in the update workgroup where the batch fills whole steps, 2 = wherever possible
  int opt_family_fused = 0;             // CCGP_OPT_FAMILY_FUSED: 1 = the 1-D families take the register-resident evaluator where small_family_fused_supported says so
  int opt_family_fused_predict = 0;     // CCGP_OPT_FAMILY_FUSED_PREDICT: 1 = their prediction and leave-one-out too (small_family_fused_predict_supported / _loo_supported)
  int opt_family_fused_grad = 0;        // CCGP_OPT_FAMILY_FUSED_GRAD: 1 = their analytic gradient and profiled mode too (small_family_fused_grad_supported / _profile_supported)
  int opt_sched = 3;                    // CCGP_OPT_SCHED: 0 = one launch per phase and block column, 1 = dataflow scheduler with two workgroups per CU, 2 = with one, 3 = by chunk size
  int opt_sched_policy = 11;            // CCGP_OPT_SCHED_POLICY bit 0: a CU's second workgroup only takes work while a backlog exists; bit 1: XCD-local synchronisation
  int sched_timeout_ms = 30000;         // a scheduler wait longer than this aborts the sweep (CCGP_SCHED_TIMEOUT_MS)
  int sched_backlog_min = 0;            // 0: one XCD's share of the CUs (CCGP_SCHED_BACKLOG overrides)
  int n_cus = 256;                      // multiProcessorCount of the handle's device
  unsigned long long* sched_prof_dev = nullptr;   // where the last scheduled sweep left its per-workgroup time account (policy bit 2)
  int sched_prof_wgs = 0;
  // the grow-only buffers (capi.hip: ensure): device scratch; the staging of the host-pointer entry points; the pinned
  // host buffer through which their inputs and results cross PCIe in one copy each
  ccgp::Buffer ws, stage, pin;
  size_t pin_in = 0;     // bytes of `pin` holding the inputs of the call in flight (results land behind them)
  int debug_fill = -1;   // ccgp_debug_fill_scratch: 0..255 = every buffer allocated from now on starts filled with this byte
  hipStream_t aux_stream = nullptr;     // second stream of the kept-factor prediction (ccgp_reserve, or first use)
  hipEvent_t aux_fork = nullptr, aux_join = nullptr;
  hipEvent_t pull_ev[ccgp::kPullSlices] = {};   // one per slice of a large result on its way back (capi.hip: pull)
  std::string err;
  ccgp::KernelFamily fam;
  unsigned timing = 0;   // bit i set: launch groups with id i are bracketed by HIP events
  std::vector<ccgp::TimedSpan> spans;
  size_t spans_used = 0;
};

namespace ccgp {

// Layout of one draw on the device: column-major B x P, element (b, j) at params[b + j*ldp].
struct DrawView {
  const double* params;
  int ldp;  // = B
  int K;
  int d;
  KernelFamily fam;
};

// ---- the variance form of a prediction (ccgp_krige_predict_batch, ccgp.h) ---------------------------------------------
// What the three prediction epilogues (small_reg_kernel<NE > 1>, site_solve_kernel, predict_finish_kernel) take beyond the
// scalar sigma2: a per-row sigma2 indexed by the GLOBAL row (nullptr: the scalar), the form (uniform per launch: a kernel
// argument, so no kernel is instantiated twice), and where each row's Q = (y - beta 1)'R^-1 (y - beta 1) goes (indexed
// like sigma2_row; may be nullptr).  All zero: predict.post as ccgp_predict_batch computes it.
struct VarForm {
  const double* sigma2_row;
  int form;
  double* q;
};
#if defined(__HIPCC__)
// (form, sigma2_b, ww = r'R^-1 r, u = 1 - 1'R^-1 r, s11 = 1'R^-1 1, Q_b, n) -> the predictive variance:
//   CCGP_VAR_ORDINARY  sigma2 (1 - ww + u^2 / s11)       predict.post, HX:669 / D1:490
//   CCGP_VAR_PLUGIN    sigma2 (1 - ww)                   mlegp's se.fit^2: no term for the estimated mean
//   CCGP_VAR_UNBIASED  Q / (n - 1) (1 - ww + u^2 / s11)  D1:504-516
__device__ __forceinline__ double predict_variance(int form, double sigma2, double ww, double u, double s11, double Q,
                                                   int n) {
  // branches, not selects: the form is uniform, and a second division computed for every form costs site_solve_kernel<8> a wave
  if (form == CCGP_VAR_PLUGIN) return sigma2 * (1.0 - ww);
  if (form == CCGP_VAR_UNBIASED) sigma2 = Q / (n - 1);
  return sigma2 * (1.0 - ww + u * u / s11);
}
// Leave-one-out at training point i from the full-data quantities (Dubrule 1983): g = (R^-1)_ii, v1 = (R^-1 1)_i,
// vy = (R^-1 y)_i, s11 = 1'R^-1 1, beta, Q = (y - beta 1)'R^-1 (y - beta 1):
//   c = g - v1^2 / s11,  a = vy - beta v1,  mean = y_i - a / c                 predict.post on the n - 1 other points
//   CCGP_VAR_ORDINARY  sigma2 / c          CCGP_VAR_PLUGIN  sigma2 / g          CCGP_VAR_UNBIASED  (Q - a^2 / c) / (n - 2) / c
__device__ __forceinline__ void loo_point(int form, double sigma2, double yi, double g, double v1, double vy, double s11,
                                          double beta, double Q, int n, double* mean, double* var) {
  const double c = g - v1 * v1 / s11, a = vy - beta * v1;
  *mean = yi - a / c;
  if (form == CCGP_VAR_PLUGIN) *var = sigma2 / g;
  else if (form == CCGP_VAR_UNBIASED) *var = (Q - a * a / c) / (n - 2) / c;
  else *var = sigma2 / c;
}
#endif

// ---- cov.hip -------------------------------------------------------------------------
// Dense cross / Gram matrix for ONE draw: out[t + i*ldo], t in [0,m) rows of A (m x d),
// i in [0,n) rows of Bm (n x d).  normalise: divide by sum w^2 (Mixed.corr.*).
void launch_cov_dense(hipStream_t s, const double* A, int m, const double* Bm, int n, int d,
                      DrawView dv, int draw, double* out, int ldo);

// Batched lower-triangle tile writer for the blocked path: for draw b0+z, writes
// s*R_mixed + t into the lower tiles of an npad x npad column-major matrix (identity on
// the padding), z in [0, nb).  scale/shift: mode 0 -> (1, 0); mode 1 -> (sigma2*sum w^2, tau2).
// upad (nb x K x npad): u[z][c][i] = sum_k theta_ck x_ik^2 of draw b0 + z, written here once per draw and read by every
// covariance tile of that draw.
void launch_cov_tiles(hipStream_t s, const double* X, int n, int d, DrawView dv, int b0, int nb,
                      double* Abase, size_t batch_stride, int npad, int mean_mode, double sigma2,
                      double tau2, int ld, double* xpad = nullptr, double* upad = nullptr);
void launch_cov_cross_batched(hipStream_t s, const double* Xtest, int m, const double* X, int n, int d,
                              DrawView dv, int b0, int nb, double* Abase, size_t batch_stride, int ldo);

// ---- summary.hip ---------------------------------------------------------------------
// predict_summary_kernel stages a site's (mu, 1 / sigma) pairs in LDS up to this many draws and streams them from the
// (L2-resident) tables beyond: 2 x 8 B x 2048 = 32 KiB of static LDS, which holds the reference's S = 1000 with room and
// still lets four workgroups share a CU's 160 KiB.
constexpr int kSummaryLdsDraws = 2048;
// prediction()'s per-site summaries (HX:686-703) of the S x m tables d_mean / d_var over the draws with d_status == 0:
// d_out is m x (4 + n_probs) column-major (ccgp_predict_summary); probs is a HOST array; d_idx (S ints) and d_count
// (1 int) are scratch.  Two launches on s.
void launch_predict_summary(hipStream_t s, const double* d_mean, const double* d_var, const int* d_status, int S, int m,
                            const double* probs, int n_probs, const double* d_y_at, int* d_idx, int* d_count,
                            double* d_out);
// the sets form (ccgp_predict_summary_sets): C sets in one grid of (site, set).  d_mean / d_var: B x m column-major with the
// rows grouped by set; d_off / d_nb (C ints each): a set's first row and its number of rows; d_idx (B ints) and d_count
// (C ints) are scratch; d_y_at: C blocks of m or nullptr; d_out: C blocks of m x (4 + n_probs) -- the block of a set
// without rows is not written.  any_staged / any_streamed: some set has at most / more than kSummaryLdsDraws rows.
void launch_predict_summary_sets(hipStream_t s, const double* d_mean, const double* d_var, const int* d_status, int B, int m,
                                 int C, const int* d_off, const int* d_nb, bool any_staged, bool any_streamed,
                                 const double* probs, int n_probs, const double* d_y_at, int* d_idx, int* d_count,
                                 double* d_out);

// ---- small.hip -----------------------------------------------------------------------
// In-LDS evaluator, one workgroup per (draw, chunk of unit rows): explicit inverse (solve(R), HX:454) and gradient for the
// n <= 128 shapes whose register-resident inverse instance does not fit (small_lds_bytes, small_pick_mtile: small_layout.h)
void launch_small_inverse(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int draw,
                          double sigma2, double* Rinv, double* loglik, double* beta, int* status);
int small_grad_chunks(int n, int d);
// gpart: scratch of B * small_grad_chunks(n, d) * P doubles.  s2hat != nullptr: the profiled mode (ccgp_profile_batch) --
// sigma2 is not read, every draw is evaluated at its own sigma2_hat, which lands in s2hat[B]
void launch_small_grad(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv,
                       int B, double sigma2, double* loglik, double* beta, double* grad,
                       int* status, double* gpart, double* s2hat = nullptr);

// ---- small_reg.hip: register-resident evaluator (n <= 128); the small_reg_*_supported predicates: small_layout.h ---------
void launch_small_reg_predict(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv,
                              int S, const double* Xtest, int m, double sigma2, double* mean, double* var,
                              double* beta, int* status, void* scratch = nullptr, size_t scratch_bytes = 0,
                              hipStream_t aux = nullptr, hipEvent_t ev_fork = nullptr, hipEvent_t ev_join = nullptr,
                              VarForm vf = VarForm{});
void launch_small_reg_logdet_designs(hipStream_t s, const double* Xs, int n, int d, DrawView dv, int B,
                                     double* logdet, int* status);
// solve(R) of ONE draw (logpost with R.Inv, HX:454) on the register-resident scheme; likelihood and beta of the same
// factorisation come with it
void launch_small_reg_inverse(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int draw,
                              double sigma2, double* Rinv, double* loglik, double* beta, int* status);
void launch_small_reg_grad(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int B,
                           double sigma2, double* loglik, double* beta, double* grad, int* status);
// ccgp_profile_batch at n <= 128: sigma2 concentrated out; grad may be nullptr (value only: the likelihood instances)
void launch_small_reg_profile(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int B,
                              double* loglik, double* s2hat, double* beta, double* grad, int* status, bool grid16 = false);
// d log det R_mixed / d X of the rows >= n_fixed for B candidate designs (entropy criteria, BSQ:856-948); dgrad holds
// per design (n - n_fixed) x d column-major
void launch_small_reg_logdet_grad_designs(hipStream_t s, const double* Xs, int n, int d, DrawView dv, int B, int n_fixed,
                                          double* logdet, double* dgrad, int* status);
void launch_small_reg_loglik(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv,
                             int B, double sigma2, int mean_mode, double tau2, double* loglik,
                             double* beta, int* status, bool grid16 = false);
// the sets form of launch_small_reg_loglik (ccgp_loglik_batch_sets where small_route_sets says Reg): row b on set set[b]
void launch_small_reg_loglik_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2,
                                  const int* set, DrawView dv, int B, int mean_mode, double tau2, double* loglik,
                                  double* beta, int* status);
// the sets form of launch_small_reg_profile with a gradient (ccgp_profile_batch_sets where small_route_profile_grad_sets says
// Reg): row b on set set[b], grad B x P column-major with leading dimension B
void launch_small_reg_profile_grad_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const int* set,
                                        DrawView dv, int B, double* loglik, double* s2hat, double* beta, double* grad,
                                        int* status);
// ccgp_family_corr_dtheta: d R_q / d theta_q of component q under the 1-D family `fam`, entry by entry (any n; x: n
// coordinates, out: n x n), from the device function the gradient epilogue of the FAM instances calls
void launch_family_dcorr(hipStream_t s, const double* x, int n, double theta, int q, KernelFamily fam, double* out);
// Metropolis chains on the device (ccgp_metro_segments_sets where small_route_chain says Reg): what chain a = workgroup a of
// A reads and leaves, every pointer a device pointer.  theta0 / theta_fin: A x p column-major (element j of chain a at
// [a + j A]); steps [A][T][p], logu [A][T]; the accepted draws [A][M][p] with their values and betas [A][M]; the trace
// [A][T], all four or none
struct ChainIO {
  int prior_id, p, T, M;
  const double* prior_pars;   // 4 values where the prior reads them
  const double *theta0, *l0, *beta0;
  const double *steps, *logu;
  const int *n_prop, *stop_acc;
  int *used, *nacc, *nfail;
  double *draws, *draw_val, *draw_beta;
  double *theta_fin, *l_fin, *beta_fin;
  double *tr_val, *tr_beta;
  int *tr_status, *tr_acc;
};
// (fam: the handle's family -- other than Gaussian where CCGP_OPT_FAMILY_FUSED routes a 1-D family here: the FAM instances)
void launch_small_reg_chain_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2,
                                 const int* set, int A, const ChainIO& io, KernelFamily fam = KernelFamily{});
// the ordinary-kriging fits on the device (ccgp_profile_fit_sets where small_route_fit says Reg): what start a = workgroup a
// of A reads and leaves, every pointer a device pointer.  state [A][W] in and out (fit_logic.h), max_evals / evals / nfail
// [A], the trace [A][T], both or none
struct FitIO {
  double* state;
  int W, T;
  const int* max_evals;
  int *evals, *nfail;
  double* tr_f;
  int* tr_status;
};
void launch_small_reg_fit_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const int* set, int A,
                               const FitIO& io);
// the maximum-entropy design search on the device (ccgp_design_fit where small_route_design_fit says Reg): what start a =
// workgroup a of A reads and leaves, every pointer a device pointer.  D_old: the n_fixed fixed rows every start shares
// (n_fixed x d column-major, not read where n_fixed == 0); state [A][W] in and out (fit_logic.h with d = nv), max_evals /
// evals / nfail [A], the trace [A][T], both or none
struct DesignFitIO {
  const double* D_old;
  double ld_offset;
  double* state;
  int W, T;
  const int* max_evals;
  int *evals, *nfail;
  double* tr_f;
  int* tr_status;
};
void launch_small_reg_design_fit(hipStream_t s, int n, int d, DrawView dv, int n_fixed, int A, const DesignFitIO& io);
// the Laplace search on the device (ccgp_laplace_search_sets where small_route_nm says Reg): what search a = workgroup a of A
// reads and leaves, every pointer a device pointer.  state [A][W] in and out (nm_logic.h), max_evals / evals / nfail [A], the
// trace [A][T], both or none
struct NmIO {
  int prior_id, q;
  const double* prior_pars;   // 4 values where the prior reads them
  double* state;
  int W, T;
  const int* max_evals;
  int *evals, *nfail;
  double* tr_val;
  int* tr_status;
};
void launch_small_reg_nm_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2,
                              const int* set, int A, const NmIO& io, KernelFamily fam = KernelFamily{});
// leave-one-out mean / variance of every training point for B draws (ccgp_loo_batch where small_route_loo says Reg): one
// workgroup per draw on the inverse instances' scheme; mean / var are B x n column-major, sigma2 is the scalar that
// vf.sigma2_row (indexed by draw) replaces, vf.q (may be nullptr) receives Q per draw
void launch_small_reg_loo(hipStream_t s, const double* X, int n, int d, const double* y, DrawView dv, int B, double sigma2,
                          VarForm vf, double* mean, double* var, double* beta, int* status);
// the sets form of launch_small_reg_predict's kept-factor scheme (ccgp_predict_batch_sets and its kin): row b on set set[b],
// its own sigma2 at vf.sigma2_row[b] (never null), mean / var B x m column-major; scratch: small_reg_sites_scratch() bytes
// per row of a chunk, at least one row
void launch_small_reg_predict_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const double* sigma2_set,
                                   const int* set, DrawView dv, int B, const double* Xtests, int m, double* mean, double* var,
                                   double* beta, int* status, void* scratch, size_t scratch_bytes, hipStream_t aux,
                                   hipEvent_t ev_fork, hipEvent_t ev_join, VarForm vf);

// ---- cgp.hip: the composite GP comparator (CGP / predict.CGP, GV:58-317), n <= 128 -------------------------------------
// LDS carve of cgp_state_kernel, in doubles:
//   A[ld][n]: the working matrix (lower triangle + rows y', 1'; G in the strict upper triangle), ld odd >= n + 2
//   xs[d][n] | y | s | sqrt s | s before scaling | e^2 | temp | Q^-1 1 | x0[d] | theta[d] | alpha[d] | bw theta[d] | red[8]
struct CgpCarve {
  int ld;
  size_t A, xs, yv, s, rs, sn, e2, tv, uv, x0, th, al, tb, red, total;
  CCGP_HD CgpCarve(int n, int d) {
    ld = (n + 2) | 1;
    A = 0;
    xs = A + (size_t)ld * n;
    yv = xs + (size_t)n * d;
    s = yv + n; rs = s + n; sn = rs + n; e2 = sn + n; tv = e2 + n; uv = tv + n;
    x0 = uv + n; th = x0 + d; al = th + d; tb = al + d;
    red = tb + d;
    total = red + 8;
  }
};
// what a `keep` evaluation leaves in HBM for cgp_predict_kernel, in doubles: the factor (n x n column-major: unit-lower L'
// below the diagonal, the pivots on it) | Q^-1 1 | s | e^2 | temp | sf, beta, tau2, 1'Q^-1 1 -- from s on in the order of
// ccgp_cgp_predict's out_state, which is one copy
struct CgpKeep {
  size_t F, u, s, res2, temp, sc, total;
  CCGP_HD CgpKeep(int n) {
    F = 0; u = (size_t)n * n; s = u + n; res2 = s + n; temp = res2 + n; sc = temp + n; total = sc + 8;
  }
};
inline bool cgp_supported(int n, int d) { return n >= 1 && n <= kSmallMaxN && d >= 1 && lds_fits(CgpCarve(n, d).total); }
// nb evaluations of the CGP state (GV:108-129; with skip, GV:168-197): params nb x (2 d + 2) column-major with leading
// dimension ldp; skip (nb, -1 = none) and loo may be nullptr; keep != nullptr: evaluation 0 leaves its CgpKeep(n) there
void launch_cgp_state(hipStream_t s, const double* X, int n, int d, const double* y, const double* params, int ldp, int nb,
                      const int* skip, double* val, double* beta, double* tau2, double* loo, int* status, double* keep);
// the sets form (ccgp_cgp_state_batch_sets): evaluation b on training set set[b] of the blocks at Xs / ys; no kept state
void launch_cgp_state_sets(hipStream_t s, const double* Xs, int n, int d, const double* ys, const int* set,
                           const double* params, int ldp, int nb, const int* skip, double* val, double* beta, double* tau2,
                           double* loo, int* status);
// the sets form that keeps (ccgp_cgp_predict_sets): as launch_cgp_state_sets without held-out rows, and EVERY evaluation
// leaves its state: evaluation b at keep + b CgpKeep(n).total
void launch_cgp_state_sets_keep(hipStream_t s, const double* Xs, int n, int d, const double* ys, const int* set,
                                const double* params, int ldp, int nb, double* val, double* beta, double* tau2, int* status,
                                double* keep);
// the CGP refinement on the device (ccgp_cgp_fit_sets): what the two launches of a round read and leave, every pointer a device
// pointer.  With P = d + 3 variables and R = 1 + 2 P rows per start: state [A][W] in and out (fit_logic.h with d = P),
// max_evals / evals / nfail / set / gate [A], the trace [A][T], both or none; rows A R x (2 d + 2) column-major with leading
// dimension ldp = A R, row_set / val / beta / tau2 / status [A R]: start a's evaluation is rows a R .. a R + R - 1
struct CgpFitIO {
  double* state;
  int W, T;
  const int* max_evals;
  int *evals, *nfail;
  double* tr_f;
  int* tr_status;
  const int* set;
  int* gate;
  double step;
  double* rows;
  int ldp;
  int* row_set;
  double *val, *beta, *tau2;
  int* status;
};
// the gated sets evaluation of the A R rows at io.rows: a workgroup whose start's gate is closed leaves at once
void launch_cgp_state_gated(hipStream_t s, const double* Xs, int n, int d, const double* ys, const CgpFitIO& io, int A);
// one wave per start: gradient from the round's values, the step of ccgp_fit_feed, the trace, the next rows or the gate closed.
// init: before the first evaluation -- counters zeroed, first rows written, gates set
void launch_cgp_fit_step(hipStream_t s, int d, int A, const CgpFitIO& io, bool init);
// predict.CGP (GV:287-307) at m sites from a kept state; row: that state's parameter row, contiguous; out m x 6 column-major
void launch_cgp_predict(hipStream_t s, const double* X, int n, int d, const double* row, const double* Xtest, int m,
                        const double* keep, const int* status, double* out);
// its sets form behind launch_cgp_state_sets_keep: row r of the nb (grid y) on set set[r] -- design Xs + set[r] n d, sites
// Xtests + set[r] m d -- from the state at keep + r CgpKeep(n).total and row r of params (nb x (2 d + 2) column-major, leading
// dimension ldp); status[r] != 0: NaN; out: nb blocks of m x 6 column-major
void launch_cgp_predict_sets(hipStream_t s, const double* Xs, int n, int d, const int* set, const double* params, int ldp,
                             int nb, const double* Xtests, int m, const double* keep, const int* status, double* out);

// ---- blocked.hip ---------------------------------------------------------------------
struct BlockedWs {
  double* A;        // nb matrices of ld x npad (lower tiles + right-hand-side / extra tile rows)
  double* invd;     // nb x nt x 128 x 128 inverses of the diagonal blocks
  double* z;        // nb x nt log-det partials
  double* fin;      // nb x 2: s11 = 1'R^-1 1 and beta per matrix (prediction pass)
  double* xpad;     // npad x kMaxD: the design zero-padded to npad rows (scalar-load source of cov_kernel's columns)
  double* upad;     // nb x kMaxK x npad: u[z][c][i] = sum_k theta_ck x_ik^2 (round 4: shared by cov_kernel and the update)
  double* sched;    // scratch of the dataflow scheduler (sched_ws_bytes): task slots, counters, queue control
  size_t a_stride;  // elements between consecutive matrices
  int ld;           // npad + 128 * (1 + ne)
  int ne;           // extra full tile rows (ceil(m / 128) for prediction, else 0)
};
// optional extra work riding on a blocked sweep (n > 128)
enum { kJobLogdet = -1, kJobNone = 0, kJobPredict = 1, kJobInverse = 2, kJobGrad = 3, kJobLoo = 4 };   // >= kJobInverse: identity rows ride along
struct BlockedJob {
  int kind;
  // kJobPredict (a10 + a11): m cross-correlation rows ride along as extra tile rows
  const double* Xtest;  // m x d, device
  int m, S;
  double* mean;         // S x m column-major, device
  double* var;
  VarForm vf;           // per-row sigma2, variance form, Q per row (all zero: predict.post with the scalar sigma2)
  // kJobInverse (solve(R), HX:454): identity rows ride along; Rinv = n x n per matrix of the chunk
  double* Rinv;
  // kJobGrad: d loglik / d params; grad is Btot x P column-major
  double* grad;
  int Btot;
  double* gpart;        // scratch: nb x blocked_grad_partials(npad) x P partial sums
  double* alpha;        // scratch: nb x npad,  R^-1 (y - beta 1)
  // kJobLoo (ccgp_loo_batch): identity rows ride along; the leave-one-out tables go to mean / var (S x n column-major, S in
  // `S`), the form, the per-row sigma2 and Q (never nullptr here: CCGP_VAR_UNBIASED reads it back) are in vf
  // kJobLogdet: log det of the normalised mixed correlation matrix (entropy criteria, BSQ:856-877), indexed like loglik
  double* logdet;
  // any kind (kJobNone: nothing else rides): the profiled mode of ccgp_profile_batch.  finish_kernel concentrates sigma2 out
  // and leaves each matrix's sigma2_hat here, indexed like loglik; the gradient stages read it instead of the scalar
  double* s2hat;
};
bool blocked_grad_supported(int d, int K);
size_t blocked_grad_partials(int npad);   // partial sums per matrix and parameter (gpart = nb x this x P)
size_t blocked_ws_bytes(int npad, int nb, int ne);
size_t sched_ws_bytes(int nt, int nb, int ne);
BlockedWs blocked_carve(void* ws, int npad, int nb, int ne);
// factorise nb matrices in place and finish the likelihood; loglik/beta/status are
// indexed from draw b0.
void blocked_loglik(ccgp_handle* h, const double* X, int n, int d, const double* y, DrawView dv,
                    int b0, int nb, int npad, double sigma2, int mean_mode, double tau2,
                    BlockedWs w, double* loglik, double* beta, int* status,
                    const BlockedJob* job = nullptr);

// forward-substitute the m cross-correlation rows held in E (S blocks of lde x npad, lde = 128 ceil(m / 128),
// row t of block s = r(x_t)' for draw s) through the KEPT factors in w and finish mean / var (S x m)
void blocked_predict_from_factors(ccgp_handle* h, const BlockedWs& w, int n, int npad, int S, int s0, int ns, double* E,
                                  size_t e_stride, int lde, int m, const int* status, double sigma2,
                                  double* mean, double* var);

// ---- special.cpp ---------------------------------------------------------------------
void halton_base2(int N, double* out);
double qigamma_host(double p, double alpha, double beta);   // the __host__ __device__ originals: special_math.h

// ---- helpers -------------------------------------------------------------------------
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Kernel attributes (dynamic-LDS ceiling) are per device: a process that holds handles on several
// GPUs must set them once on EACH.  `mask` is a function-local static, one bit per device.  Handles of
// different shards (ccgp_multi) call in from different host threads, possibly for the same device: the
// lock is held until the attributes are set, so nobody launches before they are.
inline std::mutex& attr_mutex() {
  static std::mutex m;
  return m;
}
template <class F>
inline void once_per_device(unsigned long long& mask, F set_attributes) {
  std::lock_guard<std::mutex> guard(attr_mutex());
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (mask & bit) return;
  set_attributes();
  mask |= bit;
}

// exp(x) for the covariance kernels (x = -theta-weighted squared distance, x <= 0 up to rounding).
//
// Round 3: table-driven.  exp(x) = 2^m * T[j] * e^r with n = rint(x * 256 / ln 2) = 256 m + j, T[j] = 2^(j/256)
// (256 correctly rounded doubles in LDS, exp_table.h) and |r| <= ln 2 / 512, where a degree-4 polynomial is enough
// (truncation r^5 / 120 <= 4e-17).  n comes out of the "magic number" trick: t = fma(x, 256/ln2, 1.5 * 2^52) holds
// n in the low dword of its mantissa (no v_rndne_f64, no v_cvt_i32_f64) and n as a double is t - 1.5 * 2^52.
// 11 fp64 instructions (max, fma, add, 2 fma for r, 3 fma + mul + fma for T + T (e^r - 1), ldexp) plus 3 cheap
// 32-bit ones and one LDS read, against 17 + 2 for the library routine's degree-11 polynomial that rounds 1 and 2
// used (explicit three-operand v_fma_f64: hipcc's two-address v_fmac_f64 form needs a v_mov_b64 per step) -- in
// kernels that are fp64-VALU-issue bound (PMC: cov_kernel 98 % CU-busy at 0.25 of the HBM peak; 3 x 19 of its 86
// instructions per entry were exp).  Error: <= 1.3 ulp over 2 * 10^5 arguments in [-700, 0] against a 50-digit
// exp (exact-FMA emulation; the library routine: < 1 ulp); tests hold 1e-13 on entries.
// The argument is clamped at -1000 for the index computation only (the magic-number trick needs |n| < 2^31); r is
// formed from the ORIGINAL x, so a NaN distance stays NaN, and v_ldexp_f64 underflows gradually to 0 -- down to dist = 750.
// Beyond the floor the reduction no longer cancels: r ~ -dist, the quartic grows like dist^4 / 24 against the fixed 2^-1443 of
// the clamped index, so the unselected value is 0 only up to dist ~ 1e28, then positive (2^95 -> 5e-322, 2^200 -> 1.4e-195)
// and +Inf from ~1e78 and at dist = +Inf, where exp(-dist) is 0 (base R: exp(-Inf) = 0).  Hence the closing range select:
// dist > 750 returns exactly 0 (2^-1082 is under half the smallest subnormal, so every argument that had the right value
// keeps its bits), and a NaN dist fails the compare and stays NaN ("Beyond exp's range").
static __device__ const unsigned long long kExpTableBits[kExpTableDoubles] = CCGP_EXP_TABLE_BITS;

// cooperative copy of the table into LDS (call before a barrier that precedes the first exp_cov)
__device__ __forceinline__ void exp_table_load(double* tab, int tid, int nthreads) {
  for (int e = tid; e < kExpTableDoubles; e += nthreads) tab[e] = __longlong_as_double((long long)kExpTableBits[e]);
}

// exp(-dist): the negation rides on the source modifiers of the first two instructions that read it.  Constants
// sit in SGPRs where the instruction has a single one (gfx9 VOP3: one constant-bus operand), so only 1.5 * 2^52 and
// 1/6 occupy VGPR pairs.
__device__ __forceinline__ double exp_cov(double dist, const double* tab) {
#if !defined(__HIP_DEVICE_COMPILE__)
  (void)tab;
  return exp(-dist);   // host pass of the same translation unit: never called
#else
  const double kScale = __longlong_as_double(0x40771547652b82feLL);     // 256 / ln 2
  const double kNegCHi = __longlong_as_double(0xbf662e42fe000000LL);    // -(ln 2 / 256), 24 trailing zero bits: n * hi is exact
  const double kNegCLo = __longlong_as_double(0xbd9f473de6af278fLL);
  const double kMagic = 6755399441055744.0;                             // 1.5 * 2^52
  const double c4 = __longlong_as_double(0x3fa5555555555555LL), c3 = __longlong_as_double(0x3fc5555555555555LL);
  const double kFloor = -1000.0;
  double xc, t, r, p;
  asm("v_max_f64 %0, -%1, %2" : "=v"(xc) : "v"(dist), "s"(kFloor));    // no canonicalising second v_max
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(t) : "v"(xc), "s"(kScale), "v"(kMagic));
  const double nf = t - kMagic;
  const int n = __double2loint(t);
  asm("v_fma_f64 %0, %1, %2, -%3" : "=v"(r) : "s"(kNegCHi), "v"(nf), "v"(dist));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "s"(kNegCLo), "v"(nf), "v"(r));
  const double tj = tab[n & 255];
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(r), "s"(c4), "v"(c3));
  asm("v_fma_f64 %0, %1, %2, 0.5" : "=v"(p) : "v"(r), "v"(p));
  asm("v_fma_f64 %0, %1, %2, 1.0" : "=v"(p) : "v"(r), "v"(p));
  const double q = r * p;                                               // e^r - 1
  double v;
  asm("v_fma_f64 %0, %1, %2, %1" : "=v"(v) : "v"(tj), "v"(q));         // T + T (e^r - 1)
  return dist > 750.0 ? 0.0 : __builtin_amdgcn_ldexp(v, n >> 8);
#endif
}

// One component's term of one mixed-covariance entry: acc + w_c^2 exp(-((u_row + u_col) - 2 sdot)) (HX:352-356, HX:412), in
// ONE operation order for every producer of a blocked-path entry.
__device__ __forceinline__ double cov_mix_term(double acc, double wc, double u_row, double u_col, double sdot,
                                               const double* tab) {
  const double dist = fma(-2.0, sdot, u_row + u_col);
  return fma(wc, exp_cov(dist, tab), acc);
}

// exp(-dist) WITHOUT a table: the device library's argument reduction and degree-11 polynomial as explicit
// three-operand v_fma_f64 (rounds 1-2; same bits as the library's exp): 17 fp64 instructions + 2.  Kept for the
// register-resident small-n evaluators, where the table variant measured no faster (round 3, profiles/r03/): their
// waves already wait on LDS (column broadcasts of the elimination) and 65 data-dependent table reads per thread add
// bank conflicts to that queue.
// SC: Horner constants as scalar (SGPR) operands instead of VGPRs -- see below
template <bool SC = false>
__device__ __forceinline__ double exp_cov_poly(double dist) {
  const double x = -dist;
#if !defined(__HIP_DEVICE_COMPILE__)
  return exp(x);   // host pass of the same translation unit: never called
#else
  const double kLog2e = __longlong_as_double(0x3ff71547652b82feLL);
  const double kNegLn2Hi = __longlong_as_double(0xbfe62e42fefa39efLL);
  const double kNegLn2Lo = __longlong_as_double(0xbc7abc9e3b39803fLL);
  const double c11 = __longlong_as_double(0x3e5ade156a5dcb37LL), c10 = __longlong_as_double(0x3e928af3fca7ab0cLL),
               c9 = __longlong_as_double(0x3ec71dee623fde64LL), c8 = __longlong_as_double(0x3efa01997c89e6b0LL),
               c7 = __longlong_as_double(0x3f2a01a014761f6eLL), c6 = __longlong_as_double(0x3f56c16c1852b7b0LL),
               c5 = __longlong_as_double(0x3f81111111122322LL), c4 = __longlong_as_double(0x3fa55555555502a1LL),
               c3 = __longlong_as_double(0x3fc5555555555511LL), c2 = __longlong_as_double(0x3fe000000000000bLL);
  const double n = __builtin_rint(x * kLog2e);
  double r = __builtin_fma(kNegLn2Hi, n, x);
  r = __builtin_fma(kNegLn2Lo, n, r);
  double p;
  // Horner constants: "v" operands hold 20 VGPRs, which at four waves per SIMD the compiler re-materialises with ~1.7
  // v_mov_b64 per exp; as "s" operands (a VOP3 instruction takes one scalar operand) they cost SGPRs only.  Which is
  // faster depends on what the register allocator makes of the rest of the kernel (same-box A/B, profiles/r03):
  // scalar constants gain 2 % in the general n = 100 kernel (6.23 -> 6.10 ms) and lose 10 % in the n = 64 FULL
  // instantiation (8.38 -> 9.20 ms: 148 instead of 84 B of scratch), so the caller chooses.
  if constexpr (SC) {
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(r), "s"(c11), "v"(c10));
#define CCGP_FMA3(D, A, B, C) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(D) : "v"(A), "v"(B), "s"(C))
    CCGP_FMA3(p, r, p, c9);
    CCGP_FMA3(p, r, p, c8);
    CCGP_FMA3(p, r, p, c7);
    CCGP_FMA3(p, r, p, c6);
    CCGP_FMA3(p, r, p, c5);
    CCGP_FMA3(p, r, p, c4);
    CCGP_FMA3(p, r, p, c3);
    CCGP_FMA3(p, r, p, c2);
#undef CCGP_FMA3
  } else {
#define CCGP_FMA3(D, A, B, C) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(D) : "v"(A), "v"(B), "v"(C))
    CCGP_FMA3(p, r, c11, c10);
    CCGP_FMA3(p, r, p, c9);
    CCGP_FMA3(p, r, p, c8);
    CCGP_FMA3(p, r, p, c7);
    CCGP_FMA3(p, r, p, c6);
    CCGP_FMA3(p, r, p, c5);
    CCGP_FMA3(p, r, p, c4);
    CCGP_FMA3(p, r, p, c3);
    CCGP_FMA3(p, r, p, c2);
  }
#undef CCGP_FMA3
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  return __builtin_amdgcn_ldexp(p, (int)n);
#endif
}

// the exp of the small-n evaluators (small_reg.hip, small.hip): CCGP_SMALL_EXP_TABLE (small_layout.h) 0 = polynomial, 1 = table
template <bool SC = false>
__device__ __forceinline__ double exp_small(double dist, const double* tab) {
#if CCGP_SMALL_EXP_TABLE
  return exp_cov(dist, tab);
#else
  (void)tab;
  return exp_cov_poly<SC>(dist);
#endif
}

// exp(-dist) with a range select.  exp_cov_poly's reduction has no meaning once n no longer resolves x: dist = +Inf gives
// fma(-ln2, -Inf, -Inf) = NaN, a finite dist beyond ~1e45 a garbage r whose polynomial overflows -- where exp(-dist) is 0 (base R:
// exp(-Inf) = 0).  Such a dist is a rate that overflows against a coordinate difference: outside every fit's bounds, not outside
// the raw entry points.  Beyond 750 exp_cov_poly's ldexp already returns 0 (2^-1082 p is under half the smallest subnormal), so
// every argument that had the right value keeps its bits; a NaN dist fails the compare and stays NaN.  Here and not inside
// exp_cov_poly: there the select cost the register-resident small-n evaluators 1.7 % (cfg2) and 4.8 % (cfg3) against a
// run-to-run spread of 0.1 % (profiles/exp_poly_range_select.md).  Callers: the CGP kernels (cgp.hip) and every CROSS-correlation
// vector of the small-n evaluators (test site x training points: small_reg_kernel's extra rows, site_corr_kernel) -- a cross
// vector passes no pivot test, so a wrong exponential there would reach a mean and a variance with status 0.  The matrix
// generation loops of small_reg.hip / small.hip call exp_small unselected; their domain is stated in include/ccgp.h.
template <bool SC = false>
__device__ __forceinline__ double exp_poly_ranged(double dist) { return dist > 750.0 ? 0.0 : exp_cov_poly<SC>(dist); }
template <bool SC = false>
__device__ __forceinline__ double exp_small_ranged(double dist, const double* tab) {
#if CCGP_SMALL_EXP_TABLE
  return exp_cov(dist, tab);   // selects itself
#else
  (void)tab;
  return exp_poly_ranged<SC>(dist);
#endif
}

// ---- correlation families ---------------------------------------------------------------------------
// Every kernel forms the weighted squared distance  dist = sum_k rate_k (x_ik - x_jk)^2  and then the correlation:
// the Gaussian family in the reference's expanded form, the 1-D families from the direct difference x_i - x_j, as
// their scripts do (U <- abs(A - t(A)), D1:368-374).  Gaussian (HX:328-356): rate = theta,
// corr = exp(-dist).  Matern (1-D scripts, D1:348-351): corr = z^nu K_nu(z) / (Gamma(nu) 2^(nu-1)) with
// z = 2 sqrt(nu) |h| / theta, so rate = 4 nu / theta^2 and z = sqrt(dist); d = 1 only, as in the reference.
// Two-family script (D1F:346-357, D1F:453-462): component 1 Matern as above, component 2 the non-negative
// cubic spline  1 - 6u^2 + 6u^3 (u <= 1/2), 2(1-u)^3 (u <= 1), 0 beyond, u = |h| / theta: rate = 1/theta^2.
__device__ __forceinline__ double theta_to_rate(const KernelFamily& f, double theta, int component = 0) {
  if (f.id == 0) return theta;
  if (f.id == 2 && component == 1) return 1.0 / (theta * theta);
  return 4.0 * f.nu / (theta * theta);
}
// both take the squared scaled distance as the kernel forms it, rate (x_i - x_j)^2 from the direct difference: exactly 0
// where the points coincide and NaN where a coordinate is (sqrt and every comparison below let a NaN through)
__device__ __forceinline__ double spline_corr(double u2) {
  const double u = sqrt(u2);
  if (u <= 0.5) return 1.0 - 6.0 * u * u + 6.0 * u * u * u;
  if (u <= 1.0) { const double v = 1.0 - u; return 2.0 * v * v * v; }
  return u > 1.0 ? 0.0 : u;   // NaN stays NaN (the reference's NA)
}
// z^nu K_nu(z) / (Gamma(nu) 2^(nu-1)) from  K_nu(z) = int_0^inf exp(-z cosh t) cosh(nu t) dt  by the
// trapezoidal rule (the integrand is entire and decays double-exponentially, so the rule converges
// geometrically) with step 0.15 / max(1, sqrt z): ~130 - 190 terms of three exp each -- the Matern family is for the
// reference's small 1-D designs (n = 8), not a throughput path.  Three switches:
//   z^2 <= 9e-20 (z <= 3e-10): exactly 1; 1 - f < 1.1e-18 there for every nu > 1 (at nu -> 1 it is z^2 |log z| / 2).
//   z^2 <= 1e-10 and nu >= 1.5: 1 - z^2 / (4 (nu - 1)); what it drops is below z^3 / 3 = 3.3e-16 (largest at nu = 1.5,
//     where f = (1 + z) exp(-z)).  NOT for nu < 1.5: the next term, of order (z / 2)^(2 nu) Gamma(-nu) / Gamma(nu),
//     cancels the kept one into z^2 log z as nu -> 1 (2.5e-9 relative at nu = 1.0001, z = 1e-6).
//   otherwise the rule.  Its rounding is that of the exponent nu log z - z and of the terms' exponents, ~eps times their
//     size: below z = 1e-5 that size is nu |log z| <= 1.5 * 22, above it <= 10 * 11.5, and for large z it is z, the
//     conditioning of exp(-z).
// Held by tests/test_special.py (the same rule in libm arithmetic) and tests/test_gpu_family_corr_exact.py (this code)
// to 5e-14 + 4 eps z relative against a 40-digit evaluation for nu from 1.0001 to 10 and z from 1e-9 to 740.  The last
// product is grouped so that a subnormal exp() is multiplied once, by a factor below 1: within two quanta down to 0.
__device__ inline double matern_corr(const KernelFamily& f, double z2) {
  if (!(z2 > 9e-20)) return z2 == z2 ? 1.0 : z2;
  if (z2 <= 1e-10 && f.nu >= 1.5) return 1.0 - z2 / (4.0 * (f.nu - 1.0));
  // z > 1e6: exactly 0, as the rule's last factor exp(nu log z - z) already is there (nu log z - z < -745 for every nu below
  // 7e4) -- stated ahead of the rule because z2 = +Inf (z beyond 1.3e154, whose square overflows) makes the step 0 and the
  // first term's exponent Inf * 0 = NaN, where base R's z^nu K_nu(z) is 0 (tests/test_gpu_far_arguments.py)
  if (z2 > 1e12) return 0.0;
  const double z = sqrt(z2);
  const double hs = 0.15 / fmax(1.0, sqrt(z));
  double s = 0.5;
  for (int k = 1; k < 6000; ++k) {
    const double t = k * hs;
    const double et = exp(t);
    const double c1 = 0.5 * (et + 1.0 / et) - 1.0;        // cosh t - 1
    // exp(-z (cosh t - 1)) cosh(nu t) with each exponent formed BEFORE exponentiating: exp(nu t) alone
    // overflows for large nu t long before the product does
    const double g = 0.5 * (exp(f.nu * t - z * c1) + exp(-f.nu * t - z * c1));
    s += g;
    if (g < 1e-17 * s && f.nu * t < z * c1) break;
  }
  return exp(f.nu * log(z) - z) * (hs * s * f.norm);
}
// ---- d corr / d theta of the two families (build-defined extension: the reference differentiates numerically) ----------
// Spline, u = |h| / theta: d f / d theta = -u f'(u) / theta = (12 u^2 - 18 u^3) / theta (u <= 1/2), 6 u (1 - u)^2 / theta
// (u <= 1), 0 beyond; non-negative everywhere, exactly 0 where the points coincide, NaN where a coordinate is.
// Returns the value as spline_corr forms it and writes the derivative.
__device__ __forceinline__ double spline_corr_grad(double u2, double theta, double* dth) {
  const double u = sqrt(u2);
  if (u <= 0.5) { *dth = (12.0 * u * u - 18.0 * u * u * u) / theta; return 1.0 - 6.0 * u * u + 6.0 * u * u * u; }
  if (u <= 1.0) { const double v = 1.0 - u; *dth = 6.0 * u * v * v / theta; return 2.0 * v * v * v; }
  *dth = u > 1.0 ? 0.0 : u;
  return u > 1.0 ? 0.0 : u;
}
// Matern, z = 2 sqrt(nu) |h| / theta:  d f / d theta = z^(nu+1) K_(nu-1)(z) / (Gamma(nu) 2^(nu-1) theta), from
// d/dz [z^nu K_nu] = -z^nu K_(nu-1) and dz / d theta = -z / theta: positive, no cancellation.  K_(nu-1) by matern_corr's
// own trapezoidal rule with order nu - 1 -- the same step, the same 6000-term cap, the same stopping test with nu - 1 in
// place of nu -- in ONE loop with the value's sum: exp(t) and cosh t - 1 are shared, and each sum stops adding where
// its own test says so, so the value is what matern_corr's operations give.  The exponent (nu + 1) log z - z is formed
// before exponentiating.  The rule serves every z^2 > 9e-20: the two-term series' derivative, z^2 / (2 (nu - 1) theta),
// is off by a relative z at nu = 1.5, so where matern_corr takes the series for the value the loop runs for the
// derivative alone.  At z^2 <= 9e-20 the derivative is exactly 0 (its true value is below 2.1e-18 / theta); a NaN goes
// through.  Held by tests/test_family_grad_host.py (the same rule in libm arithmetic) and
// tests/test_gpu_family_fused_grad.py (this code) against a 40-digit evaluation.
__device__ inline double matern_corr_grad(const KernelFamily& f, double z2, double theta, double* dth) {
  if (!(z2 > 9e-20)) { *dth = z2 == z2 ? 0.0 : z2; return z2 == z2 ? 1.0 : z2; }
  if (z2 > 1e12) { *dth = 0.0; return 0.0; }   // matern_corr's early return: both exp() factors are 0 beyond z = 1e6, and z2 = +Inf gave NaN
  const bool series = z2 <= 1e-10 && f.nu >= 1.5;
  const double z = sqrt(z2);
  const double hs = 0.15 / fmax(1.0, sqrt(z));
  const double num = f.nu - 1.0;
  double s = 0.5, sd = 0.5;
  bool run = !series, rund = true;
  for (int k = 1; k < 6000; ++k) {
    const double t = k * hs;
    const double et = exp(t);
    const double c1 = 0.5 * (et + 1.0 / et) - 1.0;        // cosh t - 1
    if (run) {
      const double g = 0.5 * (exp(f.nu * t - z * c1) + exp(-f.nu * t - z * c1));
      s += g;
      if (g < 1e-17 * s && f.nu * t < z * c1) run = false;
    }
    if (rund) {
      const double g = 0.5 * (exp(num * t - z * c1) + exp(-num * t - z * c1));
      sd += g;
      if (g < 1e-17 * sd && num * t < z * c1) rund = false;
    }
    if (!run && !rund) break;
  }
  const double lz = log(z);
  // The factor may exceed 1 (1 / theta), which would multiply the quantum a subnormal exp() is rounded to: below e = -700
  // the exponent is raised by 64 (exact: e and 64 are multiples of ulp(e)) and exp(-64) goes into the factor, so that the
  // one product is the only operation that rounds to a subnormal.
  const double e = (f.nu + 1.0) * lz - z, fac = (hs * sd * f.norm) / theta;
  *dth = e < -700.0 ? exp(e + 64.0) * (fac * 1.6038108905486378e-28) : exp(e) * fac;
  return series ? 1.0 - z2 / (4.0 * (f.nu - 1.0)) : exp(f.nu * lz - z) * (hs * s * f.norm);
}
__device__ __forceinline__ double corr_of_dist(const KernelFamily& f, double dist, const double* tab, int component = 0) {
  if (f.id == 0) return exp_cov(dist, tab);
  if (f.id == 2 && component == 1) return spline_corr(dist);
  return matern_corr(f, dist);
}

// Raise a kernel's dynamic-LDS ceiling to the 160 KiB of a gfx950 CU.  A refusal is remembered PER DEVICE (first one
// wins) and reported by that device's next C-ABI call's launch check instead of surfacing later as an opaque launch
// failure.  raise_lds_limit runs inside once_per_device's lambda, i.e. with attr_mutex held; readers (shard threads of
// ccgp_multi among them) look at an atomic mask first and take the mutex only when their device has an entry.
inline std::string* attr_errors() {
  static std::string e[64];
  return e;
}
inline std::atomic<unsigned long long>& attr_error_mask() {
  static std::atomic<unsigned long long> m{0};
  return m;
}
inline void raise_lds_limit(const void* kernel, const char* name) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes - 64);
  if (e == hipSuccess) return;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::string& slot = attr_errors()[dev & 63];
  if (slot.empty()) {
    slot = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for ") + name + ": " + hipGetErrorString(e);
    attr_error_mask().fetch_or(1ull << (dev & 63));
  }
}
// empty when every attribute request on `device` went through
inline std::string attr_error(int device) {
  if (!(attr_error_mask().load() & (1ull << (device & 63)))) return std::string();
  std::lock_guard<std::mutex> guard(attr_mutex());
  return attr_errors()[device & 63];
}

struct ScopedTimer {
  ccgp_handle* h;
  TimedSpan* sp = nullptr;
  hipStream_t st;
  ScopedTimer(ccgp_handle* hh, int id, hipStream_t stream = nullptr) : h(hh), st(stream ? stream : hh->stream) {
    if (!((h->timing >> id) & 1u)) return;
    if (h->spans_used == h->spans.size()) {
      TimedSpan t{};
      (void)hipEventCreate(&t.e0);
      (void)hipEventCreate(&t.e1);
      h->spans.push_back(t);
    }
    sp = &h->spans[h->spans_used++];
    sp->id = id;
    (void)hipEventRecord(sp->e0, st);
  }
  ~ScopedTimer() {
    if (sp) (void)hipEventRecord(sp->e1, st);
  }
};

}  // namespace ccgp
