/*
 * libccgp -- C ABI of the MI355X-native Combined-GP evaluation path.
 *
 * The reference (oharari/Convex-Combination-of-Gaussian-Processes) has no FFI: its
 * "API" is a set of global R functions.  Each entry point below replaces the
 * arithmetic of one or more of those functions; the R-side .Call() stub that binds
 * it is in r/ccgp_shim.c and shown in INTEGRATION.md.  Reference abbreviations:
 *   HX  = Heat Exchanger Emulator/Combined GP Heat Exchanger.R
 *   ANI = 2D Codes and Designs/2D Combined GP Anisotropic Public.R
 *   ADV = 2D Codes and Designs/2D Combined GP Isotropic Advanced.R
 *   GV  = Ground Vibrations Emulator/Combined GP Ground Vibrations.R
 *
 * Conventions
 *   - every matrix is fp64, COLUMN-MAJOR (R's native layout), no padding:
 *     X is n x d (X[i + k*n]); a parameter matrix with B draws is B x P
 *     (params[b + j*B]).
 *   - one draw of K component GPs in d dimensions is the row
 *        ( w_1..w_K , theta_{1,1..d} , ... , theta_{K,1..d} ),   P = K + K*d,
 *     and means  Sigma = sigma2 * sum_c w_c^2 R_c(theta_c),
 *                R_c[i,j] = exp(-sum_k theta_ck (x_ik - x_jk)^2).
 *     The reference's (p, theta1, theta2) isotropic draw (HX:408-415) is
 *     w = (p, 1-p), theta_1k = theta1, theta_2k = theta2; its anisotropic draw
 *     (ANI:399-406) is theta_1 = (theta1,theta2), theta_2 = (1+lambda)(theta1,theta2).
 *   - the caller owns every buffer; the library allocates only device scratch kept
 *     in the handle.  A handle is bound to ONE HIP device and is not re-entrant
 *     (R is single-threaded; one handle per host thread / per GPU process); ccgp_multi
 *     (below) puts several devices behind one call.
 *   - return value: 0 ok, <0 error (ccgp_last_error), >0 = number of evaluations in
 *     the batch whose factorisation met a non-positive pivot.  Per-evaluation
 *     status[b] = 0 or 1-based index of the first bad pivot; such an evaluation
 *     returns NaN -- the reference's NA from try(solve(R)) (HX:454-455).
 *   - domain of the rates: base R has exp(-x) = 0 for every x beyond 745, +Inf
 *     included.  The raw correlation entry points, everything computed on the blocked
 *     sweep (n > 128 and the n <= 128 shapes routed there) and every cross-correlation
 *     vector (test site x training points) on every route return exactly 0 for such an
 *     exponent at ANY finite magnitude and at +Inf (NaN stays NaN), and so does the
 *     extra-row prediction of the register-resident evaluator (n > 104, K > 3 or
 *     CCGP_OPT_PREDICT_FACTOR = 0), matrix and cross rows alike.  The matrix
 *     generation of the other register- and LDS-resident n <= 128 evaluators is exact in
 *     that sense for exponents below 2^148.47 (3.3e44), a worst-case bound: its reduced
 *     argument is the rounding residue of n = rint(x log2 e), up to ulp(n) ln 2 / 2, and
 *     the degree-11 polynomial overflows from 2^95.4, i.e. possibly from n = 2^149; beyond
 *     that -- rates of 2^140 on an integer lattice wider than 11 x 10 -- an evaluation is
 *     either still right or FAILS under the contract above (status = a pivot index,
 *     NaN outputs, counted in the return value) -- never a finite wrong value, never
 *     a non-finite value with status 0.  Such rates lie outside every fit's bounds.
 *   - "_dev" entry points take DEVICE pointers and only enqueue work on the
 *     handle's stream (no allocation, no synchronisation once the workspace has
 *     been sized by ccgp_reserve); the others take HOST pointers and block.
 *     The kept-factor prediction also uses a second stream of the handle's, forked
 *     from and joined back into the handle's stream inside the call: to the caller
 *     the call is ordered on the handle's stream alone.
 */
#ifndef CCGP_H
#define CCGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ccgp_handle ccgp_handle;

enum {
  CCGP_OK = 0,
  CCGP_EINVAL = -1,       /* bad argument */
  CCGP_EHIP = -2,         /* a HIP runtime call failed */
  CCGP_ENOMEM = -3,       /* device workspace allocation failed */
  CCGP_EUNSUPPORTED = -4  /* combination not implemented (message says which) */
};

/* how the mean and the extra variance enter the likelihood */
enum {
  CCGP_MEAN_PROFILE_BETA = 0,  /* logpost: beta = 1'R^-1 y / 1'R^-1 1  (HX:458-460)        */
  CCGP_MEAN_ZERO_PLUS_TAU2 = 1 /* cond.like: mean 0, Sigma + tau^2 11'    (HX:567-570)        */
};

/* which script's log-prior ccgp_logpost adds */
enum {
  CCGP_PRIOR_INVGAMMA = 0, /* HX:462 / ADV:467, pars (a1,b1,a2,b2)                          */
  CCGP_PRIOR_GV = 1,       /* GV:450                                                        */
  CCGP_PRIOR_ISO = 2,      /* ISO:453 = BSQ:450 = D1:636                                    */
  CCGP_PRIOR_ANI = 3       /* ANI:462 (4 transformed parameters, anisotropic kernel)        */
};

/* ---- lifetime --------------------------------------------------------------------- */
int ccgp_create(int device, ccgp_handle** out);
int ccgp_destroy(ccgp_handle* h);
const char* ccgp_last_error(const ccgp_handle* h);
const char* ccgp_version(void);
/* run on a caller-owned hipStream_t.  NULL does NOT mean the legacy default stream: it selects the library's own stream,
 * created non-blocking, which does not order with the legacy default stream (nor with any other); a caller whose default
 * stream reports a null pointer passes a stream it created.  The call only switches: it neither waits for the work already
 * enqueued on the previous stream nor makes the new stream wait for it.  A caller who changes streams with work in flight
 * must order the two streams themself (an event, or ccgp_synchronize before the switch). */
int ccgp_set_stream(ccgp_handle* h, void* hip_stream);
/* correlation family of every component GP for the calls that follow (default Gaussian).
 * CCGP_KERNEL_GAUSS : R_c[i,j] = exp(-sum_k theta_ck (x_ik - x_jk)^2)     corr.matrix HX:328-337, ANI:351-360
 * CCGP_KERNEL_MATERN: the 1-D scripts' Matern.corr.func(nu, h, theta) D1:348-351,
 *                     R_c[i,j] = z^nu K_nu(z) / (Gamma(nu) 2^(nu-1)),  z = 2 sqrt(nu) |x_i - x_j| / theta_c;
 *                     d must be 1 and a draw is (w_1..w_K, theta_1..theta_K); 1 < nu <= 10, the range the quadrature is validated on (D1:1080 uses 5).
 * Replaces corr.matrix(nu, X, theta) D1:368-374, corr.vec D1:383-389 and everything built on them
 * (Mixed.corr.matrix D1:575-584, logpost D1:609-641, predict.post D1:794-812) through the same entry
 * points as the Gaussian family; the analytic gradient is Gaussian-only.
 * CCGP_KERNEL_MATERN_SPLINE: the two-family 1-D script (1D Combined GP Two Families Public.R = D1F), K = 2:
 *                     component 1 Matern(nu, theta_1) as above, component 2 the non-negative cubic spline
 *                     spline.corr.func(theta_2, h) D1F:346-357.  corr.matrix.combined D1F:453-462 is
 *                     ccgp_mixed_corr_matrix; corr.vec.combined D1F:470-480 is ccgp_mixed_corr_cross and -- as
 *                     written there, the division by p^2 + (1-p)^2 sits after the return -- is NOT normalised;
 *                     predict.post D1F:737-754 (ccgp_predict_batch) uses that same vector. */
enum { CCGP_KERNEL_GAUSS = 0, CCGP_KERNEL_MATERN = 1, CCGP_KERNEL_MATERN_SPLINE = 2 };
int ccgp_set_kernel(ccgp_handle* h, int family, double nu);
/* cap on device scratch used per launch group; larger batches are processed in chunks.  Default: three
 * quarters of the device's memory (216 of 288 GB on MI355X), and never more than is free at call time. */
int ccgp_set_workspace_limit(ccgp_handle* h, size_t bytes);
/* measurement switches (A/B runs under rocprof; results do not depend on them).  Option numbers 0, 1 and 6 were
 * CCGP_OPT_UPDATE_STRIPS, CCGP_OPT_SMALL_LDS and CCGP_OPT_FUSED_COV of rounds 1 - 4 (removed in round 5: no caller outside
 * tests; the fused covariance generation measured 0.3 % and is kept as profiles/r05/fused_cov_removed.diff) and are refused.
 *   CCGP_OPT_FUSE_DIAG      1 (default) = the update launch's diagonal-tile workgroup also factorises and inverts
 *                           the diagonal block; 0 = a separate diag_kernel launch per block column
 *   CCGP_OPT_TAIL_STRIPS    1 (default) = the tiles of an update launch's last, partial step of 256 workgroups run
 *                           as four quarter-width or two half-width strips each, whichever fills the step; 2 = half-width
 *                           strips only (rounds 2 - 3); 0 = every tile whole (same bits all three)
 *   CCGP_OPT_WIDE_OFFSETS   0 (default) = the update loops address their panels through 32-bit buffer offsets wherever a
 *                           panel spans less than 4 GiB; 1 = always the 64-bit-pointer loops that larger matrices
 *                           fall back to (same bits: the tests hold one against the other)
 *   CCGP_OPT_SMALL_GRID16   0 (default) = 64 < n <= 104 runs ONE wave per matrix on the 8 x 8 thread grid (up to 13 x 13
 *                           blocks per thread); 1 = the 16 x 16 grid (one workgroup per matrix) of rounds 1 - 3 (same bits)
 *   CCGP_OPT_PREDICT_FACTOR 1 (default) = prediction tables at n <= 104 (K <= 3) factorise each draw ONCE, keep the factor in HBM
 *                           and solve for the test sites with one lane per site; 0 = the extra-row scheme of rounds 2 - 4 (the
 *                           test sites ride through the elimination in chunks of 30 / 62, one factorisation per chunk): same
 *                           bits, the tests hold one against the other
 *   CCGP_OPT_SCHED          the blocked Cholesky sweep of a chunk (n > 128): 0 = one launch per phase and block column
 *                           (rounds 1 - 4); 1 = ONE persistent launch whose workgroups take diagonal / update / panel-solve
 *                           tiles from dependency-driven queues, two workgroups per CU; 2 = the same with one workgroup per CU;
 *                           3 (default) = 2 for chunks of 32 ... 128 matrices with n >= 2048, where it measures ahead, else 0.
 *                           Same tile code and summation order: same bits.
 *   CCGP_OPT_SCHED_POLICY   bit mask, default 11.  bit 0: a CU's second workgroup only takes a tile while ready tiles are waiting
 *                           (0 = always); bit 1: tiles of a matrix stay on one XCD and synchronise through its L2 (L1
 *                           invalidate + store completion); 0 = agent-scope release / acquire fences, which write back and
 *                           invalidate that L2 per tile (same bits, 40 % slower: DESIGN.md K3); bit 2: keep the per-workgroup
 *                           time account that ccgp_last_sched_profile reads; bit 3: a workgroup goes on with the first task its
 *                           own arrivals made ready instead of queueing it; bit 4 (tests only): drop the announcements of
 *                           matrix 0's second block column, so that the sweep cannot finish -- it must then abort after
 *                           CCGP_SCHED_TIMEOUT_MS (environment, default 30000) and fail every evaluation of the chunk, not hang
 *   CCGP_OPT_FUSED_SOLVE    the launch-per-phase sweep from block column 1 on: 0 = an update and a panel-solve (trsm) launch per
 *                           block column; 1 (default) = a diagonal launch (one workgroup per matrix: diagonal tile, block
 *                           factorisation, right-hand-side rows solved) and a tile launch whose workgroups update a tile AND
 *                           solve it against the inverted diagonal block in place, so that the updated tile never goes to
 *                           memory and there is no trsm launch -- taken when the chunk holds a multiple of 256 matrices
 *                           (whole steps of the chip), there are no extra tile rows (likelihood and factor jobs), CCGP_OPT_FUSE_DIAG is
 *                           1 and 32-bit panel offsets fit; 2 = the same route whatever the number of matrices.  Block column
 *                           0 and everything else keep the update / trsm launches.  Same summation order: same bits.  Both
 *                           launches are timed under CCGP_T_UPDATE; CCGP_T_TRSM is then block column 0 alone.
 *   CCGP_OPT_FAMILY_FUSED   NOT a same-bits switch.  0 (default) = CCGP_KERNEL_MATERN and CCGP_KERNEL_MATERN_SPLINE exist on the
 *                           blocked sweep only, and the chain and search entry points refuse them; 1 = at d = 1, 1 <= n <= 32
 *                           (K <= 8; K = 2 for the two-family kernel) the register-resident evaluator generates the family's
 *                           matrix itself -- the entries cov_kernel forms, from the direct difference x_i - x_j -- and serves
 *                           ccgp_loglik_batch(_dev) in both mean modes, the value-only ccgp_logpost and ccgp_logpost_batch,
 *                           ccgp_grid_marginal, ccgp_loglik_batch_sets, ccgp_logpost_sets, ccgp_chain_logpost_sets (one launch
 *                           for all sets instead of a sweep per set), ccgp_metro_segments_sets and ccgp_laplace_search_sets
 *                           (CCGP_OK instead of CCGP_EUNSUPPORTED: a chain or a search runs to its end inside one launch).  The
 *                           elimination is another one than the sweep's, so the values agree with the option off to rounding,
 *                           not in their bits; a pivot at or below the tolerance gives the 1-based pivot index and NaN as on
 *                           the Gaussian route.  Everything else keeps its route and its refusals whatever the option says:
 *                           prediction and kept factors, ccgp_logpost with R.Inv, the gradient, ccgp_profile_batch(_sets),
 *                           leave-one-out, the device fits, kriging, designs, CGP, and every n > 32.  No effect under
 *                           CCGP_KERNEL_GAUSS.  (Prediction and leave-one-out have an option of their own, below.)
 *   CCGP_OPT_FAMILY_FUSED_PREDICT  NOT a same-bits switch, and independent of CCGP_OPT_FAMILY_FUSED.  0 (default) = prediction
 *                           and leave-one-out of the two 1-D families run on the blocked sweep; 1 = inside the domain of
 *                           CCGP_OPT_FAMILY_FUSED (d = 1, n <= 32; K = 2 for the two-family kernel) the register-resident
 *                           evaluator serves ccgp_predict_batch(_dev), ccgp_predict_summary(_dev) and ccgp_krige_predict_batch
 *                           in its three variance forms at K <= 3 by the kept-factor scheme -- one factorisation per draw, the
 *                           test sites' correlation vectors from the direct difference x_t - x_i (under the two-family kernel
 *                           NOT divided by sum w^2, as corr.vec.combined is written), one lane per site -- and
 *                           ccgp_loo_batch and ccgp_loo_summary at n >= 2 from one factorisation per draw.  A family has no
 *                           extra-row scheme: with CCGP_OPT_PREDICT_FACTOR = 0, or where the kept factor's scratch cannot be
 *                           had, a prediction stays on the sweep with the sweep's bits.  Values agree with the option off to
 *                           rounding; a site's column does not depend on the other sites, a draw's row not on the other
 *                           draws; a failed pivot gives the 1-based index and NaN rows as on the Gaussian route.  Nothing else
 *                           moves: ccgp_factor_batch and factor sets, R.Inv, the gradient, the profiled mode, the device fits,
 *                           n > 32 and K > 3 keep their routes.  No effect under CCGP_KERNEL_GAUSS.
 *   CCGP_OPT_FAMILY_FUSED_GRAD  NOT a same-bits switch, and independent of CCGP_OPT_FAMILY_FUSED and
 *                           CCGP_OPT_FAMILY_FUSED_PREDICT.  0 (default) = the analytic gradient is refused under the two 1-D
 *                           families (CCGP_EUNSUPPORTED) and their profiled mode runs on the blocked sweep; 1 = inside the
 *                           domain of CCGP_OPT_FAMILY_FUSED (d = 1, n <= 32; K = 2 for the two-family kernel) the
 *                           register-resident evaluator serves ccgp_loglik_grad_batch, ccgp_profile_batch with and without
 *                           out_grad and ccgp_profile_batch_sets (with out_grad: one launch for all sets; without: set by set
 *                           through the fused single call).  The theta columns are + sigma2 w_q^2 sum_ab M_ab d R_q,ab / d
 *                           theta_q with the family's own derivative (Matern: z^(nu+1) K_(nu-1)(z) / (Gamma(nu) 2^(nu-1)
 *                           theta), spline: -u f'(u) / theta), the entries ccgp_family_corr_dtheta returns.  A row of the
 *                           sets call has the bits of the single-set call on its set; failures as on the Gaussian route
 *                           (1-based pivot index and a NaN row, gradient included; Q == 0: +Inf, NaN gradient, status 0).
 *                           Outside the domain (n = 33, d = 2, K = 3 under the two-family kernel) the gradient stays refused
 *                           before anything is copied or launched.  Nothing else moves: the device fits, the _dev variants,
 *                           R.Inv and ccgp_reserve keep their routes.  No effect under CCGP_KERNEL_GAUSS. */
enum { CCGP_OPT_FUSE_DIAG = 2, CCGP_OPT_TAIL_STRIPS = 3, CCGP_OPT_WIDE_OFFSETS = 4, CCGP_OPT_SMALL_GRID16 = 5,
       CCGP_OPT_SCHED = 7, CCGP_OPT_SCHED_POLICY = 8, CCGP_OPT_PREDICT_FACTOR = 9, CCGP_OPT_FUSED_SOLVE = 10,
       CCGP_OPT_FAMILY_FUSED = 11, CCGP_OPT_FAMILY_FUSED_PREDICT = 12, CCGP_OPT_FAMILY_FUSED_GRAD = 13 };
int ccgp_set_option(ccgp_handle* h, int option, int value);
/* pre-size scratch so that later _dev calls of this shape (or of fewer draws B or test sites m), under the kernel family,
 * options and workspace limit in force now, never allocate, synchronise or create a stream or an event.  Covers: the
 * blocked sweep's workspace of ccgp_loglik_batch_dev; with m > 0 also that of a prediction on the sweep, the kept-factor
 * prediction's scratch together with its second stream and fork / join events (CCGP_OPT_PREDICT_FACTOR), and the tables
 * ccgp_predict_summary_dev keeps between its launches; the staging of the host-pointer likelihood and prediction.  Not
 * covered: the events of ccgp_enable_timing (created on first use).  May itself allocate and synchronise. */
int ccgp_reserve(ccgp_handle* h, int n, int d, int K, int B, int m);
int ccgp_synchronize(ccgp_handle* h);

/* ---- a1/a2/a3: covariance kernels ---------------------------------------------------
 * corr.matrix(X, theta) HX:328-337 / ANI:351-360, corr.matrix.ISO HX:347-356 (caller
 * replicates theta d times); corr.vec / corr.vec.ISO HX:367-375, ANI:369-377 are the
 * m = 1 case of ccgp_corr_cross.  out_R is n x n, out is m x n (row t = r(x_t)). */
int ccgp_corr_matrix(ccgp_handle* h, const double* X, int n, int d, const double* theta,
                     double* out_R);
int ccgp_corr_cross(ccgp_handle* h, const double* Xnew, int m, const double* X, int n, int d,
                    const double* theta, double* out);

/* build-defined extension: d R_q / d theta_q of component q (0-based) under the 1-D family in force (d = 1: X holds n
 * coordinates), entry by entry -- the derivative the gradient under CCGP_OPT_FAMILY_FUSED_GRAD sums, out of the C ABI as the
 * values are out of ccgp_corr_matrix.  params is ONE row (2 K doubles: weights, then thetas); out is n x n, symmetric,
 * its diagonal exactly 0; a NaN coordinate gives a NaN row and column.  Any n; needs no option.  Host pointers; blocks.
 * CCGP_EUNSUPPORTED under CCGP_KERNEL_GAUSS. */
int ccgp_family_corr_dtheta(ccgp_handle* h, const double* X, int n, int K, const double* params /* one row */, int q,
                            double* out /* n x n */);

/* ---- a4/a5: convex-combination mix ---------------------------------------------------
 * Mixed.corr.matrix HX:408-415, ANI:399-406, ADV:414-421; Mixed.corr.vec HX:425-431,
 * ANI:416-422.  params is ONE row (P doubles). */
int ccgp_mixed_corr_matrix(ccgp_handle* h, const double* X, int n, int d, int K,
                           const double* params, double* out_R);
int ccgp_mixed_corr_cross(ccgp_handle* h, const double* Xnew, int m, const double* X, int n,
                          int d, int K, const double* params, double* out);

/* ---- a6/a7: beta.MLE HX:384-388, sigma2.MLE HX:394-399 (explicit R.Inv given) -------- */
int ccgp_beta_mle(ccgp_handle* h, const double* R_inv, const double* y, int n, double* out_beta);
int ccgp_sigma2_mle(ccgp_handle* h, const double* R_inv, const double* y, int n, double beta,
                    double* out_sigma2);

/* ---- a8/a9/a12: batched log-likelihood ----------------------------------------------
 * For each of B draws: build the mixed covariance, factorise, solve, return
 *   mode 0: dmnorm(y, beta_hat, sigma2*sum(w^2)*R_mixed, log)   (HX:454-460), out_beta
 *   mode 1: dmnorm(y, 0, sigma2*sum(w^2)*R_mixed + tau2 11', log) (HX:567-570), beta = 0
 * out_beta / status may be NULL. */
int ccgp_loglik_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                      const double* params, int B, double sigma2, int mean_mode, double tau2,
                      double* out_loglik, double* out_beta, int* status);
int ccgp_loglik_batch_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
                          const double* dparams, int B, double sigma2, int mean_mode, double tau2,
                          double* d_loglik, double* d_beta, int* d_status);

/* build-defined extension (the reference has no analytic gradient; LearnBayes::laplace
 * differences numerically, HX:493): d loglik(mode 0, beta profiled) / d params[b, j],
 * out_grad is B x P column-major.  Any n: n <= 128 in LDS; larger n carries the identity as
 * extra tile rows of the blocked sweep and contracts R^-1 tiles with the kernel derivatives.
 * Gaussian family; CCGP_KERNEL_MATERN and CCGP_KERNEL_MATERN_SPLINE at d = 1, n <= 32 under CCGP_OPT_FAMILY_FUSED_GRAD
 * (theta columns with respect to the family's theta); CCGP_EUNSUPPORTED otherwise, before anything is copied. */
int ccgp_loglik_grad_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                           const double* params, int B, double sigma2, double* out_loglik,
                           double* out_beta, double* out_grad, int* status);

/* ---- ordinary-kriging MLE: the likelihood with sigma2 concentrated out ------------------
 * What the scripts take from an ordinary-kriging fit: sigma2.MLE (D1:411-415) inside log.like / log.likeli
 * (D1:424-444), and `ord$sig2` of mlegp (HX:759-760).  For draw b with M = sum_c w_c^2 R_c(theta_c):
 *   beta   = 1'M^-1 y / 1'M^-1 1,   Q = (y - beta 1)'M^-1 (y - beta 1),   sigma2 = Q / n,
 *   loglik = -(n log 2 pi + n log sigma2 + log det M + n) / 2
 * (the 1-D scripts' log.likeli is log det M + n log sigma2 = -2 loglik - n log 2 pi - n), from ONE factorisation per
 * draw: sigma2 is formed on the device in the pass that forms Q.  out_grad (B x P column-major, may be NULL):
 * d loglik / d params[b, j] -- the gradient of the mode-0 likelihood at (beta, sigma2) of the draw (envelope theorem).
 * Host pointers; blocks.  Every family of ccgp_set_kernel without out_grad; with it the Gaussian family, and the two
 * 1-D families at d = 1, n <= 32 under CCGP_OPT_FAMILY_FUSED_GRAD (which also moves their value-only call from the sweep
 * to the register-resident evaluator) -- CCGP_EUNSUPPORTED otherwise, and for d + K beyond the blocked contraction's
 * LDS, as ccgp_loglik_grad_batch.
 * A failed factorisation: status[b] = 1-based pivot index, NaN in loglik, sigma2, beta and the gradient row; returns
 * the number of failed draws.  Q == 0 (y exactly constant): sigma2 = 0, loglik = +Inf, gradient row NaN, status 0.
 * out_beta / out_grad / status may be NULL. */
int ccgp_profile_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                       const double* params, int B, double* out_loglik, double* out_sigma2,
                       double* out_beta, double* out_grad /* B x P column-major, may be NULL */,
                       int* status);

/* ---- the CGP comparator of compare.GP: CGP GV:58-236, predict.CGP GV:245-317 ------------------
 * (the same two functions in every script; compare.GP calls them at GV:654-660, HX:713-725.)  A parameter row is
 * (lambda, theta[d], alpha[d], bw) on the scale of X as given: G = exp(-D(theta)), L = exp(-D(alpha)), Gbw = exp(-D(bw theta)),
 * D(r)_ij = sum_k r_k (x_ik - x_jk)^2.  One evaluation is the reference's fixed loop (GV:108-129): s = 1; four times
 *   Q = G + lambda diag(sqrt s) L diag(sqrt s), beta = 1'Q^-1 y / 1'Q^-1 1, temp = Q^-1 (y - beta 1), e = y - beta - G temp,
 *   s = (Gbw e^2) / (Gbw 1), sf = mean(s), s /= sf;
 * then a fifth Q: beta, temp, tau2 = (y - beta 1)'temp / n, val = log det Q + n log tau2 (var.MLE.DK's value, without the
 * 1e6 of GV:130-131: a non-finite val with status 0 -- sf = 0 for exactly interpolated data -- stays as it is).
 * ccgp_cgp_state_batch replaces B calls of var.MLE.DK (GV:102-133) and, with skip, the jackknife loop's body (GV:168-197):
 * skip[b] >= 0 runs evaluation b on the n - 1 other points and out_loo[b] is predict.CGP's value for the held-out point
 * (v from the fourth pass's e^2 and sf, q = g + lambda sqrt(v) sqrt(s) * l, beta + q'temp); NaN where skip[b] is -1.
 * params is B x (2 d + 2) column-major.  n <= 128 and d small enough for the design to lie in LDS beside the working matrix
 * (d <= 21 at n = 128), else CCGP_EUNSUPPORTED before anything is launched.  A pivot <= n eps in any of the five
 * factorisations (the rule of the mode-0 likelihood: the reference calls solve(Q)) gives status[b] = that pivot's 1-based
 * index and NaN in every output of evaluation b; returns the number of failed evaluations.  An evaluation depends on its
 * own row only: not on B, its position, or where the workspace limit cuts the batch.  skip, out_beta, out_tau2, out_loo and
 * status may be NULL.
 * ccgp_cgp_predict replaces the final state (GV:200-221) and predict.CGP with PI = TRUE (GV:287-307) for ONE row: the state
 * stays on the device as its factor, Q^-1 1 and temp, and each test site takes its q'Q^-1 q from a forward substitution
 * through that factor.  out is m x 6 column-major: Yp gp lp v Y_low Y_up; out_state (3 n + 3, may be NULL) receives
 * s[n] (the diagonal of Sig_matrix), res2[n], temp[n], sf, beta, tau2.  m may be 0 (state only).  A failed state: *status
 * = the pivot's index, NaN everywhere, return value 1.
 * Host pointers; both block.  Not in this version: _dev variants, ccgp_reserve coverage, a ccgp_multi wrapper, an R shim. */
int ccgp_cgp_state_batch(ccgp_handle* h, const double* X, int n, int d, const double* y,
                         const double* params /* B x (2d+2) */, int B, const int* skip /* B or NULL */,
                         double* out_val, double* out_beta, double* out_tau2, double* out_loo /* NULL ok */,
                         int* status);
int ccgp_cgp_predict(ccgp_handle* h, const double* X, int n, int d, const double* y,
                     const double* params /* one row */, const double* Xtest, int m, double* out /* m x 6 */,
                     double* out_state /* 3n+3, NULL ok */, int* status);

/* ---- a8 (+a13): logpost(D.train, theta, y, sigma2[, pars]) -> list(val, beta, R.Inv) --
 * theta_t = (psi1, psi2, phi[, zeta]) on the transformed scale; prior_pars =
 * (a1,b1,a2,b2) for CCGP_PRIOR_INVGAMMA, ignored otherwise.  out_loglik (the bare
 * dmnorm term; ADV:470 returns its exp) and out_Rinv (n x n, solve(R) of HX:454; any n) may
 * be NULL. *status as in the batch call. */
int ccgp_logpost(ccgp_handle* h, const double* X, int n, int d, const double* y, double sigma2,
                 int prior_id, const double* theta_t, const double* prior_pars, double* out_val,
                 double* out_beta, double* out_loglik, double* out_Rinv, int* status);
/* logpost of B transformed parameter vectors in one call -- the candidates of a speculative block of Metro (HX:505-512: the
 * random numbers of an iteration do not depend on accept / reject, so the 2^m - 1 candidates the chain can reach over the next
 * m iterations are known up front; r/ccgp_shim.c: ccgp_R_metro_steps), or a population of starting points.  theta_t is B x q
 * column-major, q = 3 (4 for CCGP_PRIOR_ANI).  val / beta / loglik per row exactly as ccgp_logpost returns them (same device
 * evaluator, same host arithmetic for Jacobian and prior: same bits); NaN and status != 0 where the factorisation fails.
 * Replaces B calls of logpost HX:441-466 (GV:429-454, ISO:433-457, ADV:447-471, ANI:433-467, D1:609-641, D1F:576-602). */
int ccgp_logpost_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, double sigma2, int prior_id,
                       const double* theta_t, int B, const double* prior_pars, double* out_val, double* out_beta,
                       double* out_loglik, int* status);

/* ---- many training sets of one shape in one call: the lockstep fit of a simulation study (GV:689-708 declares nine sets) --
 * Xs holds C designs (blocks of n x d, column-major each), ys their C responses (blocks of n), sigma2 their C variances; row b
 * of params (B x P column-major, as in ccgp_loglik_batch) is evaluated on set set[b] in 0 .. C-1.
 *   Bits.  Row b has exactly the bits ccgp_loglik_batch / ccgp_logpost_batch returns for it on set set[b] alone: they do not
 *     depend on C, B, the row's position, the order of `set`, or where the workspace limit cuts the call.
 *   Failure.  status[b] is the 1-based pivot and the row's outputs are NaN; the other rows are untouched; the return value is
 *     the number of failed rows.
 *   Arguments.  C < 1, B < 1, a set[b] outside 0 .. C-1 or a NULL required pointer (everything but out_beta, out_loglik of
 *     ccgp_logpost_sets, status, and prior_pars where the prior ignores it) return CCGP_EINVAL before anything is copied or
 *     launched.  A set no row refers to is legal.
 *   Shapes.  Every shape and kernel family the single-set call serves: Gaussian sets of n <= 128 whose instance fits run as
 *     ONE launch; otherwise the rows are grouped by set and each group goes through the single-set call.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging.  ccgp_logpost_sets: K = 2, theta_t is B x q as in
 * ccgp_logpost_batch, Jacobian and prior by the same host code. */
int ccgp_loglik_batch_sets(ccgp_handle* h, const double* Xs /* C blocks n x d, column-major each */, int n, int d,
                           const double* ys /* C blocks of n */, const double* sigma2 /* C */, int C, int K,
                           const double* params /* B x P column-major */, const int* set /* B, 0 .. C-1 */, int B,
                           int mean_mode, double tau2, double* out_loglik, double* out_beta, int* status);
int ccgp_logpost_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                      int prior_id, const double* theta_t /* B x q */, const int* set, int B,
                      const double* prior_pars, double* out_val, double* out_beta, double* out_loglik, int* status);

/* ---- Metropolis chains on the device: many proposals per launch (Metro, HX:483-540) ------------------------------------------
 * The random numbers of a proposal do not depend on the chain's state: the candidate is theta + e_t and the rule is
 * isfinite(l_cand) && l_cand - l > log u_t.  ccgp_metro_segments_sets takes A chains, chain a on training set set[a], each
 * with its start state (theta0 A x q column-major as theta_t; l0; beta0, may be NULL: NaN) and a block of pre-drawn
 * increments steps[a][t][j] and log-uniforms logu[a][t] (leading dimension T), and walks chain a through its proposals
 * t = 0, 1, .. on the device until it has accepted stop_acc[a] draws in this call or used n_prop[a] <= T proposals.  One
 * workgroup per chain; no chain waits for another.
 *   Values.  The likelihood of a proposal has the bits ccgp_loglik_batch_sets gives that parameter row.  Jacobian, prior and
 *     the parameter row come from a restatement of ccgp_logpost's host arithmetic whose exp and log are built from exactly
 *     rounded operations, so that host and device agree bit for bit: ccgp_chain_terms is that arithmetic on the host (rows
 *     B x P column-major as ccgp_loglik_batch takes them; needs no handle), ccgp_chain_logpost_sets the whole evaluation
 *     (arguments, checks and routes of ccgp_logpost_sets) -- the chain's host twin.  A chain driven proposal by proposal
 *     through ccgp_chain_logpost_sets makes the same decisions and leaves the same bits.  val is NaN (one quiet NaN) where
 *     the factorisation fails or a term is NaN.
 *   Outputs per chain.  out_used[a], out_accepted[a]; the accepted draws in order, out_draws[(a M + k) q + j] with their
 *     values out_draw_val[a M + k] and betas out_draw_beta[a M + k], k < out_accepted[a] <= stop_acc[a] <= M (entries beyond
 *     are NaN); the final state out_theta (A x q column-major), out_l, out_beta (may be NULL).  The trace (all four or none,
 *     [a T + t]): val, beta, pivot status and accept flag of every proposal used; NaN / -1 beyond.
 *   Bits.  A chain depends on its own inputs only: not on A, its position, the other chains' sets, what the handle ran before,
 *     or how its proposals are cut into calls (the state a call leaves is the next call's start).
 *   Failure.  A failed factorisation is a rejected proposal (status = 1-based pivot in the trace, val and beta NaN); the chain
 *     goes on.  The return value is the number of such proposals over all chains.
 *   Arguments.  CCGP_EINVAL before anything is copied or launched, outputs untouched: bad shapes, a NULL required pointer,
 *     an unknown prior (prior_pars as ccgp_logpost_batch), C < 1, A < 0, T < 1, M < 1, set[a] outside 0 .. C-1, n_prop[a]
 *     outside 0 .. T, stop_acc[a] outside 0 .. M, a partial trace.  CCGP_EUNSUPPORTED, outputs untouched, where the sets
 *     likelihood has no one-launch route: n > 128, the Matern and spline families (served at d = 1, n <= 32 under
 *     CCGP_OPT_FAMILY_FUSED), a shape whose instance does not fit.
 *     A == 0 returns CCGP_OK.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging. */
int ccgp_chain_terms(int prior_id, int d, const double* theta_t /* B x q */, int B, const double* prior_pars,
                     double* out_rows /* B x (2 + 2 d) column-major */, double* out_ljac, double* out_lprior);
int ccgp_chain_logpost_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                            int prior_id, const double* theta_t /* B x q */, const int* set, int B,
                            const double* prior_pars, double* out_val, double* out_beta, double* out_loglik, int* status);
int ccgp_metro_segments_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                             int prior_id, const double* prior_pars, int A, const int* set /* A */,
                             const double* theta0 /* A x q */, const double* l0 /* A */, const double* beta0 /* A or NULL */,
                             int T, const double* steps /* A x T x q */, const double* logu /* A x T */,
                             const int* n_prop /* A */, const int* stop_acc /* A */, int M, int* out_used,
                             int* out_accepted, double* out_draws /* A x M x q */, double* out_draw_val /* A x M */,
                             double* out_draw_beta /* A x M */, double* out_theta /* A x q */, double* out_l,
                             double* out_beta, double* trace_val /* A x T */, double* trace_beta, int* trace_status,
                             int* trace_accept);

/* ---- the comparator fits over many training sets of one shape: what compare.GP's table holds beside the Combined GP -------
 * The sets form of ccgp_profile_batch (the ordinary-kriging MLE behind sigma2 and the single-GP columns) and of
 * ccgp_cgp_state_batch (CGP's candidates, refinement points and jackknife), so that a study's comparator fits run in lockstep
 * across its sets as its chains do.  Xs, ys, set as in ccgp_loglik_batch_sets; params, the outputs and their NULLs as in the
 * single-set call.
 *   Bits.  Row b has exactly the bits ccgp_profile_batch / ccgp_cgp_state_batch returns for it on set set[b] alone -- for the
 *     CGP call including its skip[b]: they do not depend on C, B, the row's position, the order of `set`, or where the
 *     workspace limit or the 65535-workgroup grid cuts the call.
 *   Failure.  status[b] is the 1-based pivot and the row's outputs are NaN, the whole gradient row included; the other rows are
 *     untouched; the return value is the number of failed rows.  Q == 0 as in ccgp_profile_batch: sigma2 = 0, loglik = +Inf,
 *     gradient row NaN, status 0.
 *   Arguments.  C < 1, a set[b] outside 0 .. C-1, a NULL required pointer (everything but out_beta, out_grad, status; for the
 *     CGP call everything but skip, out_beta, out_tau2, out_loo, status) or a skip[b] that ccgp_cgp_state_batch refuses return
 *     CCGP_EINVAL before anything is copied or launched, outputs untouched.  B == 0 returns CCGP_OK.  A set no row refers to
 *     is legal.  CCGP_EUNSUPPORTED exactly where the single-set call says it.
 *   Routes.  ccgp_profile_batch_sets with out_grad, Gaussian family, n <= 128 where the register-resident gradient instance
 *     fits (where ccgp_profile_batch's gradient runs in LDS as one workgroup per row): ONE launch per chunk for all rows.
 *     So for the two 1-D families at d = 1, n <= 32 under CCGP_OPT_FAMILY_FUSED_GRAD; without that option their gradient is
 *     refused as in ccgp_profile_batch.
 *     Every other shape and family the single-set call serves (n > 128, the in-LDS fallback, Matern and spline value-only):
 *     the rows are grouped by set and each group goes through ccgp_profile_batch.  The value-only form (out_grad == NULL)
 *     takes that grouped route at EVERY shape: a fit calls it once, and one-launch instances for it would be 42 more kernels
 *     (both grids, every block count, general and full) in the file whose compile time is already the build's longest; the
 *     bits contract is the same either way.  ccgp_cgp_state_batch_sets: one launch per chunk for every supported shape.
 * Host pointers only, blocking; the sets go up once per call, not once per chunk; ccgp_reserve does not cover the staging.
 * Not in this version: _dev variants, a ccgp_multi wrapper, an R shim. */
int ccgp_profile_batch_sets(ccgp_handle* h, const double* Xs /* C blocks n x d, column-major each */, int n, int d,
                            const double* ys /* C blocks of n */, int C, int K, const double* params /* B x P */,
                            const int* set /* B, 0 .. C-1 */, int B, double* out_loglik, double* out_sigma2,
                            double* out_beta /* NULL ok */, double* out_grad /* B x P column-major, NULL ok */,
                            int* status /* NULL ok */);
int ccgp_cgp_state_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C,
                              const double* params /* B x (2d+2) */, const int* set, int B, const int* skip /* B or NULL */,
                              double* out_val, double* out_beta, double* out_tau2, double* out_loo, int* status);

/* ---- the Combined GP's and the single GP's prediction over many training sets of one shape ----------------------------------
 * The sets forms of ccgp_predict_batch, ccgp_krige_predict_batch and ccgp_predict_summary: row b of params is a draw (a fitted
 * model) of training set set[b] and is predicted at that set's own test sites, so that the prediction stage of a study is one
 * call per model and shape instead of one per set.  Xs, ys, sigma2 (one per set), set as in ccgp_loglik_batch_sets; Xtests
 * holds C blocks of m x d column-major, m common to the sets of a call; params, sigma2_row, var_form, probs and the NULLs of
 * the outputs as in the single-set call.  out_mean / out_var: B x m column-major, [b + t B].  ccgp_predict_summary_sets: ys_at
 * (may be NULL) holds C blocks of m; out holds C blocks of m x (4 + n_probs) column-major, block c summarising the rows with
 * set[b] == c and status 0 in increasing b; a set with no such row is NaN throughout.
 *   Bits.  Row b (for the summary: set c's block) has exactly the bits the single-set entry point returns on that set alone
 *     with its rows in their order: they do not depend on C, B, the row's position, the order of `set`, the workspace limit
 *     or what the handle ran before.
 *   Failure.  As in the single-set calls: status[b] is the 1-based pivot and row b is NaN; a failed row is left out of its
 *     set's summary; other rows and other sets are untouched; the return value is the number of failed rows.
 *   Arguments.  C < 1, B < 1, m < 1, a set[b] outside 0 .. C-1, a NULL required pointer, a var_form or a sigma2_row that
 *     ccgp_krige_predict_batch refuses, or probs that ccgp_predict_summary refuses return CCGP_EINVAL before anything is copied
 *     or launched, outputs untouched.  A set no row refers to is legal.
 *   Routes.  ONE set of launches per chunk of rows, for the rows of all sets, exactly where the single-set call takes the
 *     kept-factor scheme: Gaussian family, n <= 104 and K <= 3 with the carves that fit (the sets instance keeps a design per
 *     matrix on the 8 x 8 grid), CCGP_OPT_PREDICT_FACTOR on and the scratch to be had.  The rows are grouped by set and go up
 *     with every set's design, responses and test sites in one span; a factor-keeping sets instance of the small-n evaluator,
 *     the correlation kernel with a set per row and the site kernel serve a chunk -- as many rows as the kept-factor scratch
 *     holds under the workspace limit, at least 64; a cut may fall inside a set --; the summary then runs its (site, set)
 *     grids on the whole tables, which never leave the device; one span comes down.
 *     Everything else -- 105 <= n <= 128, K > 3, n > 128, the option off, the Matern and spline families with or without
 *     option 12 -- is grouped by set: the single-set launches run set after set on resident inputs with no host copy between
 *     them, whatever route they take.  The kept-factor and extra-row schemes have the same bits, so the contract does not
 *     depend on the route.  All inputs and tables of a call are staged at once: the workspace limit governs the kept-factor
 *     scratch, not the staging.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging.  Not in this version: _dev variants, ccgp_multi
 * wrappers, an R shim. */
int ccgp_predict_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2 /* C */,
                            int C, int K, const double* params /* B x P */, const int* set, int B,
                            const double* Xtests /* C blocks m x d */, int m, double* out_mean, double* out_var /* B x m */,
                            double* out_beta /* NULL ok */, int* status /* NULL ok */);
int ccgp_krige_predict_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int K,
                                  const double* params, const int* set, int B,
                                  const double* sigma2_row /* B; NULL ok for CCGP_VAR_UNBIASED */, int var_form,
                                  const double* Xtests, int m, double* out_mean, double* out_var, double* out_beta,
                                  double* out_q, int* status);
int ccgp_predict_summary_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2 /* C */,
                              int C, int K, const double* params, const int* set, int B, const double* Xtests, int m,
                              const double* probs, int n_probs, const double* ys_at /* C blocks of m, NULL ok */,
                              double* out /* C blocks of m x (4 + n_probs) */, double* out_beta /* B */, int* status /* B */);

/* ---- the CGP comparator's prediction over many training sets of one shape: the CGP columns of a study's tables in one call ----
 * The sets form of ccgp_cgp_predict: row b of params is a fitted model of training set set[b] and is predicted at that set's
 * own test sites.  Xs, ys, set as in ccgp_loglik_batch_sets; Xtests holds C blocks of m x d column-major, m common to the
 * sets of a call (m may be 0: states only).  out: B blocks of m x 6 column-major, block b as ccgp_cgp_predict's out;
 * out_state (may be NULL): B blocks of 3 n + 3 as ccgp_cgp_predict's out_state; status (may be NULL): B.
 *   Bits.  Block b of out and of out_state has exactly the bits ccgp_cgp_predict returns for that row on set set[b] alone
 *     with that set's test sites: they do not depend on C, B, the row's position, the order of `set`, where the workspace
 *     limit or the 65535-workgroup grid cuts the call, or what the handle ran before.
 *   Failure.  As in ccgp_cgp_predict, per row: status[b] is the 1-based pivot, blocks b of out and out_state are NaN; the
 *     other rows are untouched; the return value is the number of failed rows.
 *   Arguments.  C < 1, B < 0, m < 0, a set[b] outside 0 .. C-1 or a NULL required pointer (everything but out_state and
 *     status; Xtests and out only where m > 0) return CCGP_EINVAL before anything is copied or launched, outputs untouched.
 *     B == 0 returns CCGP_OK.  A set no row refers to is legal.  CCGP_EUNSUPPORTED exactly where ccgp_cgp_predict says it.
 *   Route.  One state launch (every row keeps its factor, Q^-1 1 and temp on the device) and one site launch (row x site) per
 *     chunk, for every supported shape; a chunk is as many rows as the workspace limit allows (n^2 + 7 n + 6 m + 2 d + 16
 *     doubles each).
 * Host pointers only, blocking; the sets and their test sites go up once per call, not once per chunk; ccgp_reserve does not
 * cover the staging.  Not in this version: a _dev variant, a ccgp_multi wrapper, an R shim. */
int ccgp_cgp_predict_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C,
                          const double* params /* B x (2d+2) */, const int* set, int B,
                          const double* Xtests /* C blocks m x d */, int m /* may be 0 */, double* out /* B blocks of m x 6 */,
                          double* out_state /* B blocks of 3n+3, NULL ok */, int* status /* B, NULL ok */);

/* ---- the ordinary-kriging fits on the device: every start in one launch (mlegp(...)$sig2, HX:759-760) ----------------------------
 * The quasi-Newton iteration of a start (box-constrained L-BFGS, memory 5, projected Armijo search: design._Start of the
 * Python package) restated from exactly rounded operations (csrc/fit_logic.h), so that host and device step a start to the
 * same bits.  One start's state is a flat array of W = ccgp_fit_state_doubles(d) = 16 + 16 d doubles:
 *   [0] d  [1] code  [2] f  [3] t  [4] backtracks  [5] iterations  [6] first  [7] pairs kept  [8] maxit  [9] factr  [10] pgtol
 *   [11] max_backtracks  [12] evaluations fed  [13 .. 15] 0, then x | g | p | trial | lo | hi (d each) and the five (s, y)
 *   pairs, s_0 .. s_4 | y_0 .. y_4, oldest first.
 *   code: 0 running, 1 converged by relative reduction, 2 converged by projected gradient, 3 maxit, 4 line-search failure,
 *   5 the start itself cannot be evaluated.  While the code is 0, `trial` is the next point to evaluate.
 * ccgp_fit_begin fills a state from a start x0 (clipped into [lo, hi]) and the options (R's optim defaults are maxit = 100,
 * factr = 1e7, pgtol = 0; max_backtracks = 30); ccgp_fit_feed hands it the value f and gradient g (d values) at `trial`, ok != 0
 * where the evaluator reported no failure, and returns the new code.  Host only, no handle; CCGP_EINVAL for d outside 1 .. 64, a
 * NULL pointer, maxit < 0, max_backtracks < 0, or (feed) a state whose recorded d is not d.
 * The objective.  x = log theta; theta_k = exp(x_k) by the portable exp of the device chains (ccgp_chain_terms), the parameter
 * row is (1, theta), f = -loglik and g_k = -(d loglik / d theta_k) theta_k.  ccgp_profile_fit_eval_sets is that evaluation of
 * B points (logtheta, out_g, out_theta: B x d column-major) on the host side of ccgp_profile_batch_sets: it forms the rows,
 * calls ccgp_profile_batch_sets with that call's arguments, checks and routes -- so it serves every shape and family that call
 * serves, value-only (out_g == NULL) included -- and transforms the results.  A failed row has f = NaN (the one quiet NaN), a
 * NaN gradient row and its 1-based pivot in status; the return value is the number of failed rows.  NULL ok: out_g, out_theta,
 * out_sigma2, out_beta, status.
 * ccgp_profile_fit_sets runs A starts, start a on training set set[a] (Xs, ys, C as in ccgp_profile_batch_sets, K = 1), on the
 * device: one workgroup carries one start from its state through up to max_evals[a] evaluations -- theta from `trial`, the
 * profiled likelihood and its gradient from one factorisation, the step of ccgp_fit_feed -- and writes the state back, so the
 * next call continues it.  out_evals[a] is the number of evaluations made.  The trace (both or neither, [a T + t]): f and the
 * pivot status of evaluation t of this call; NaN / -1 beyond out_evals[a].
 *   Bits.  Every evaluation inside a fit has the bits ccgp_profile_batch_sets gives that row on that set.  A start driven
 *     evaluation by evaluation through ccgp_profile_fit_eval_sets and ccgp_fit_feed leaves the same state and trace, bit for bit.
 *   Independence.  A start depends on its own inputs only: not on A, its position, the other starts' sets, what the handle ran
 *     before, or how its evaluations are cut into calls by max_evals.
 *   Failure.  A failed factorisation is an infeasible trial: the line search backs off and the start goes on.  A start whose
 *     first point fails ends with code 5, its neighbours untouched.  The return value is the number of evaluations whose
 *     factorisation failed, over all starts.
 *   Arguments.  CCGP_EINVAL before anything is copied or launched, outputs untouched: bad shapes, C < 1, A < 0, T < 0, set[a]
 *     outside 0 .. C-1, max_evals[a] outside 0 .. min(T, 4096), a partial trace, a NULL required pointer (everything but the
 *     trace), a state whose recorded d is not d.  CCGP_EUNSUPPORTED, outputs untouched, where ccgp_profile_batch_sets has no
 *     one-launch gradient route or the start's words do not fit beside its carve: n > 128, the Matern and spline families.
 *     A == 0 returns CCGP_OK.  A start that is not running, or whose max_evals is 0, is returned as it came.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging.  Not in this version: _dev variants, a ccgp_multi
 * wrapper, an R shim. */
int ccgp_fit_state_doubles(int d);
int ccgp_fit_begin(double* state, int d, const double* x0, const double* lo, const double* hi, int maxit, double factr,
                   double pgtol, int max_backtracks);
int ccgp_fit_feed(double* state, int d, double f, const double* g, int ok);
int ccgp_profile_fit_eval_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C,
                               const double* logtheta /* B x d */, const int* set, int B, double* out_f,
                               double* out_g /* B x d, NULL: value-only */, double* out_theta, double* out_sigma2,
                               double* out_beta, int* status);
int ccgp_profile_fit_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int A,
                          const int* set /* A */, double* state /* A x W, in and out */, const int* max_evals /* A */,
                          int* out_evals /* A */, double* trace_f, int* trace_status /* A x T, both or neither */, int T);

/* ---- the Laplace search on the device: every set's Nelder-Mead in one launch (LearnBayes::laplace, HX:493) -----------------------
 * The Nelder-Mead search of the Python package's fit.laplace_sets for one set (coefficients 1, 2, 1/2, 1/2; the initial simplex
 * x[k] -> (1.0 + 0.05) x[k], or 0.00025 where x[k] is zero; converged where every |x_v - x_0| <= xatol and every
 * |f_0 - f_v| <= fatol; a non-finite value counts as -1e300) restated from exactly rounded operations (csrc/nm_logic.h), so
 * that host and device step a search to the same bits, and advanced ONE evaluation at a time: reflection first, then the
 * expansion or the contraction the reflected value calls for, the shrink points only where the contraction fails.  One
 * search's state is a flat array of W = ccgp_nm_state_doubles(q) = q^2 + 5 q + 18 doubles:
 *   [0] q  [1] code  [2] phase  [3] vertex (of the initial-simplex and shrink phases)  [4] iterations
 *   [5] charged: the evaluations laplace_sets counts for this search (q + 1, + 4 per iteration, + q per shrink); the maxiter
 *       rule reads it  [6] fed: the evaluations actually made  [7] maxiter  [8] xatol  [9] fatol
 *   [10] expansions taken  [11] expansions refused  [12] plain reflections  [13] outside contractions taken
 *   [14] inside contractions taken  [15] shrinks
 *   then the simplex ((q + 1) x q, vertex-major, best first once sorted) | the negated values (q + 1) | xbar (q) | the
 *   reflected point (q) | its negated value (1) | trial (q).
 *   code: 0 running, 1 converged, 2 maxiter (iterations >= maxiter or charged >= maxiter, tested after the convergence test,
 *   once the initial simplex is sorted and after every iteration's sort).  phase: 0 initial simplex, 1 reflection, 2 expansion,
 *   3 outside contraction, 4 inside contraction, 5 shrink.  While the code is 0, `trial` is the next point to evaluate; the
 *   mode is simplex vertex 0 and its value minus negated value 0.
 * ccgp_nm_begin fills a state from a start x0 (laplace_sets uses xatol = 1e-6, fatol = 1e-9) with `trial` = x0;
 * ccgp_nm_feed hands it the log-posterior at `trial` and returns the new code.  Host only, no handle; CCGP_EINVAL for q outside
 * 1 .. 8, a NULL pointer, maxiter < 0, or (feed) a state whose recorded q is not q.
 * ccgp_laplace_search_sets runs A searches, search a on training set set[a] (Xs, ys, sigma2, C, prior_id, prior_pars as in
 * ccgp_chain_logpost_sets; q = 3, or 4 for CCGP_PRIOR_ANI), on the device: one workgroup carries one search from its state
 * through up to max_evals[a] evaluations -- the portable terms of `trial`, the likelihood, val = ll + ljac + lprior, the step of
 * ccgp_nm_feed -- and writes the state back, so the next call continues it.  out_evals[a] is the number of evaluations made.
 * The trace (both or neither, [a T + t]): val and the pivot status of evaluation t of this call; NaN / -1 beyond out_evals[a].
 *   Bits.  Every evaluation has the bits ccgp_chain_logpost_sets gives that point on that set.  A search driven evaluation by
 *     evaluation through ccgp_chain_logpost_sets and ccgp_nm_feed leaves the same state and trace, bit for bit.
 *   Independence.  A search depends on its own inputs only: not on A, its position, the other searches' sets, what the handle
 *     ran before, or how its evaluations are cut into calls by max_evals.
 *   Failure.  A failed factorisation is a non-finite value (NaN in the trace, its 1-based pivot in the status): the search
 *     goes on.  The return value is the number of evaluations whose factorisation failed, over all searches.
 *   Arguments.  CCGP_EINVAL before anything is copied or launched, outputs untouched: bad shapes, an unknown prior (prior_pars
 *     as ccgp_logpost_batch), C < 1, A < 0, T < 0, set[a] outside 0 .. C-1, max_evals[a] outside 0 .. min(T, 4096), a partial
 *     trace, a NULL required pointer (everything but the trace and prior_pars), a state whose recorded q is not the prior's.
 *     CCGP_EUNSUPPORTED, outputs untouched, where ccgp_metro_segments_sets has no route or the search's words do not fit
 *     behind its carve: n > 128, the Matern and spline families (served at d = 1, n <= 32 under CCGP_OPT_FAMILY_FUSED).
 *     A == 0 returns CCGP_OK.  A search that is not running, or
 *     whose max_evals is 0, is returned as it came.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging.  Not in this version: the Hessian points inside the
 * launch, _dev variants, a ccgp_multi wrapper, an R shim. */
int ccgp_nm_state_doubles(int q);
int ccgp_nm_begin(double* state, int q, const double* x0, double xatol, double fatol, int maxiter);
int ccgp_nm_feed(double* state, int q, double val);
int ccgp_laplace_search_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                             int prior_id, const double* prior_pars, int A, const int* set /* A */,
                             double* state /* A x W, in and out */, const int* max_evals /* A */, int* out_evals /* A */,
                             double* trace_val, int* trace_status /* A x T, both or neither */, int T);

/* ---- a9: likeli.hyperpars HX:549-575 / choose.hyperpars HX:584-595, ADV:552-599 -------
 * hyper is G x 4 (alpha1 beta1 alpha2 beta2).  For each row: N base-2 Halton quantiles
 * u_j, p = u_j, theta1 = qigamma(u_j, a1, b1), theta2 = qigamma(u_j, a2, b2), mode-1
 * likelihood with tau2 = tau^2, mean of exp() over j (accumulated as log-sum-exp).
 * out[g] = log(mean) if take_log (HX:591) else mean (ADV:595); *out_argmax is the
 * 0-based which.max row.  aniso_lambda < 0: isotropic kernel (HX/ADV); >= 0: the
 * anisotropic kernel of ANI:399-406 with d = 2, (theta1,theta2) per dimension and that
 * fixed lambda (BASELINE config 3).  out_logs (G x N, may be NULL) receives every
 * conditional log-likelihood. */
int ccgp_grid_marginal(ccgp_handle* h, const double* X, int n, int d, const double* y,
                       double sigma2, const double* hyper, int G, int N, double tau, int take_log,
                       double aniso_lambda, double* out, int* out_argmax, double* out_logs);
/* the quadrature nodes the call above uses, exposed for the R surface / tests */
int ccgp_halton_base2(int N, double* out);
int ccgp_qigamma(const double* p, int N, double alpha, double beta, double* out);

/* ---- a10/a11: factors HX:604-613, predict.post HX:655-673 / ANI:604-623 --------------
 * ccgp_predict_batch recomputes, per draw, what Metro caches (R.Inv, beta; HX:515-525)
 * and returns the S x m tables mean[s + t*S], var[s + t*S] that prediction() averages
 * (HX:688-693).  out_beta (S) and status (S) may be NULL.  Any n: n <= 128 runs the
 * register-resident evaluator, larger n (or a shape its LDS carve cannot hold) appends the
 * m cross-correlation rows to the blocked sweep. */
int ccgp_predict_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                       const double* params, int S, const double* Xtest, int m, double sigma2,
                       double* out_mean, double* out_var, double* out_beta, int* status);
int ccgp_predict_batch_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
                           const double* dparams, int S, const double* dXtest, int m,
                           double sigma2, double* d_mean, double* d_var, double* d_beta,
                           int* d_status);

/* ---- the ordinary-kriging ("single") comparator of compare.GP: its prediction -------------------
 * compare.GP puts a single GP beside the Combined GP and the CGP.  Row b is one fitted model: its parameter row has the
 * layout ccgp_predict_batch takes, R_b is the normalised mixed matrix that call uses (HX:408-415), and the row has its
 * own sigma2_b.  With q = r'R^-1 r, u = 1 - 1'R^-1 r, s11 = 1'R^-1 1, beta_b = 1'R^-1 y / s11 and
 * Q_b = (y - beta_b 1)'R_b^-1 (y - beta_b 1):
 *   mean = beta_b + r'R^-1 (y - beta_b 1)              the expression, and the bits, of ccgp_predict_batch
 *   CCGP_VAR_ORDINARY  var = sigma2_b (1 - q + u^2 / s11)        predict.post (HX:669, D1:490)
 *   CCGP_VAR_PLUGIN    var = sigma2_b (1 - q)                    mlegp's se.fit^2 (predict.gp(se.fit = TRUE): GV:662-666,
 *                                                                ANI:679-683, ISO:665-669, ADV:733-737, BSQ:664-668)
 *   CCGP_VAR_UNBIASED  var = Q_b / (n - 1) (1 - q + u^2 / s11)   the 1-D scripts (D1:504-516; CIs.single D1F:851-889);
 *                                                                takes no sigma2
 * ccgp_profile_batch works on the unnormalised M = sum w^2 R, so sigma2_b = sigma2_hat_M sum w^2 and
 * Q_b = n sigma2_hat_M sum w^2; for a single GP (K = 1, w = 1) they are the same numbers.  out_q is formed with the
 * expression and summation order of that call's sigma2 on the same route.
 * out_mean / out_var: B x m column-major as ccgp_predict_batch; out_beta, out_q, status (B each) may be NULL.
 * CCGP_EINVAL before anything is launched, outputs untouched: var_form outside 0..2; UNBIASED with n < 2; ORDINARY or
 * PLUGIN with sigma2 NULL or any sigma2_b not finite or negative.  A failed factorisation is reported as
 * ccgp_predict_batch reports it: status[b] = 1-based pivot index, NaN in row b of both tables, out_beta[b] and out_q[b];
 * returns the number of failed rows.  A row depends on its own parameters, sigma2_b and Q_b only: not on B, its position,
 * or where the workspace limit or a route's chunking cuts the call.  The route is ccgp_predict_batch's
 * (CCGP_OPT_PREDICT_FACTOR included); every family of ccgp_set_kernel (other than Gaussian: the blocked sweep).
 * Host pointers; blocks.  Not in this version: a _dev variant, ccgp_reserve coverage, a ccgp_multi wrapper, a
 * factor-set variant, an R shim. */
enum { CCGP_VAR_ORDINARY = 0, CCGP_VAR_PLUGIN = 1, CCGP_VAR_UNBIASED = 2 };
int ccgp_krige_predict_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                             const double* params, int B,
                             const double* sigma2 /* B values; ignored (may be NULL) for UNBIASED */,
                             int var_form, const double* Xtest, int m,
                             double* out_mean, double* out_var /* B x m column-major, as ccgp_predict_batch */,
                             double* out_beta /* B, NULL ok */, double* out_q /* B: Q_b, NULL ok */,
                             int* status /* B, NULL ok */);

/* ---- leave-one-out cross-validation of the Combined GP (Dubrule 1983) --------------------------------
 * What n calls of ccgp_predict_batch -- each on the n - 1 other points and the one held-out site -- return, from ONE
 * factorisation per draw.  For draw b with parameters fixed, R the normalised mixed matrix ccgp_predict_batch uses:
 *   v1 = R^-1 1,  v2 = 1'v1,  beta = v1'y / v2,  a = R^-1 (y - beta 1),  Q = (y - beta 1)'a
 *   g_i = (R^-1)_ii,   c_i = g_i - v1_i^2 / v2
 *   mean[b,i] = y_i - a_i / c_i
 *   var[b,i]  = sigma2_b / c_i                        CCGP_VAR_ORDINARY  (predict.post, HX:669)
 *             = sigma2_b / g_i                        CCGP_VAR_PLUGIN    (mlegp's se.fit^2)
 *             = (Q - a_i^2 / c_i) / (n - 2) / c_i     CCGP_VAR_UNBIASED  (D1:504-516 on n - 1 points); takes no sigma2
 * mean[b,i] and the ORDINARY var[b,i] are predict.post(x_i, D[-i,], ...) (HX:655-673) with factors() recomputed on the
 * n - 1 other points and beta re-estimated there; out_beta[b] and out_q[b] are the FULL-data beta and Q above.
 * out_mean / out_var: B x n column-major (element (b, i) at [b + i*B]); out_beta, out_q, status (B each) may be NULL.
 * CCGP_EINVAL before anything is launched, outputs untouched: var_form outside 0..2; n < 2, or n < 3 with UNBIASED;
 * ORDINARY or PLUGIN with sigma2 NULL or any sigma2_b not finite or negative.  B == 0 returns CCGP_OK.  A failed
 * factorisation (the pivot rule of the mode-0 likelihood): status[b] = 1-based pivot index, NaN in row b of both tables,
 * out_beta[b] and out_q[b]; returns the number of failed rows.  A row depends on its own parameters and sigma2_b only: not
 * on B, its position, or where the workspace limit cuts the call.
 * Route: Gaussian family where the register-resident inverse instance fits (n <= 128, small d, K): one launch, one
 * workgroup per draw, an O(n^2) epilogue behind the factorisation (CCGP_T_FUSED).  Everything else -- larger n, and every
 * other family of ccgp_set_kernel -- carries the identity as extra tile rows of the blocked sweep and reads L^-1 once,
 * O(n^2) per draw, with no R^-1 tile product (the epilogue is timed under CCGP_T_SOLVE).
 * Under CCGP_KERNEL_MATERN_SPLINE the result is this closed form on the NORMALISED R.  The script's predict.post uses the
 * un-normalised corr.vec.combined there (D1F:470-480), so the closed form is NOT what ccgp_predict_batch returns on the
 * reduced sets for that family; for the other two families it is.
 * ccgp_loo_summary runs the same evaluation (CCGP_VAR_ORDINARY, one sigma2) into device tables and summarises them as
 * ccgp_predict_summary does with the training points as sites and y_at = y: out is n x (4 + n_probs) column-major, column 3
 * is the PIT value F(y_i) of the leave-one-out posterior predictive; failed draws are left out and counted as there.
 * Host pointers; both block.  Not in this version: _dev variants, ccgp_reserve coverage, a ccgp_multi wrapper, an R shim. */
int ccgp_loo_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                   const double* params, int B,
                   const double* sigma2 /* B values; ignored, may be NULL, for UNBIASED */,
                   int var_form, double* out_mean, double* out_var /* B x n column-major: [b + i*B] */,
                   double* out_beta /* B, NULL ok */, double* out_q /* B: Q_b, NULL ok */, int* status /* B, NULL ok */);
int ccgp_loo_summary(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                     const double* params, int S, double sigma2, const double* probs, int n_probs,
                     double* out /* n x (4 + n_probs), the columns of ccgp_predict_summary with y_at = y */,
                     double* out_beta, int* status);

/* ---- prediction(): the per-site summaries of those tables (HX:686-703 / GV:620-638) -------------
 * Every script ends in compare.GP -> prediction(): per test site the mean of the S per-draw means, a
 * prediction interval and Quant.Combined, which the reference estimates from ONE normal variate per draw.
 * The posterior predictive at a site is known exactly -- the equal-weight mixture of the S' normals
 * N(mean_s, var_s) of the draws with status 0 -- so the summaries are computed from it, on the device,
 * where the tables already are, and only m x (4 + n_probs) doubles come back:
 *   sigma_s  = sqrt(max(var_s, 0));  F(q) = 1/S' sum_s Phi((q - mean_s) / sigma_s)  (sigma_s = 0: a step at mean_s)
 *   column 0   y_hat    = 1/S' sum mean_s
 *   column 1   pred_var = 1/S' sum sigma_s^2 + 1/S' sum (mean_s - y_hat)^2
 *   column 2   quant    = 1 - F(y_hat)      (the expectation of mean(y.hat <= posterior.predictive))
 *   column 3   cdf_at   = F(y_at[t])        (NaN when y_at is NULL)
 *   column 4+j q_j      = inf{q : F(q) >= probs[j]},  j < n_probs <= CCGP_SUMMARY_MAX_PROBS
 * out is m x (4 + n_probs) column-major.  Every probs[j] lies strictly inside (0, 1), else CCGP_EINVAL.  A site
 * with S' = 0 is NaN throughout.  Failed draws are left out and reported through status as ccgp_predict_batch
 * reports them; the return value is their count.  y_at (m), out_beta (S) and status (S) may be NULL.  A site's row
 * depends on its own column of the tables only: not on m, the other sites, or the entry point. */
enum { CCGP_SUMMARY_MAX_PROBS = 8 };
int ccgp_predict_summary(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                         const double* params, int S, const double* Xtest, int m, double sigma2,
                         const double* probs, int n_probs, const double* y_at, double* out,
                         double* out_beta, int* status);
/* the same on device pointers (HX:686-703), asynchronous on the handle's stream like ccgp_predict_batch_dev (returns
 * CCGP_OK; the failed draws are in d_status).  probs stays a HOST array: its values travel as kernel arguments. */
int ccgp_predict_summary_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
                             const double* dparams, int S, const double* dXtest, int m, double sigma2,
                             const double* probs, int n_probs, const double* d_y_at, double* d_out,
                             double* d_beta, int* d_status);
/* ---- device-resident factor set ------------------------------------------------
 * Metro caches R.Inv and beta of every accepted draw (HX:515-525), factors.frame flattens them into a
 * (5 + 2n + n^2)-column data-frame row (HX:625-644) and predict.post re-parses that row for every test
 * site (HX:655-665).  Here the per-draw cache stays on the device as the Cholesky factor the sweep left
 * behind (lower tiles, inverted diagonal blocks, L^-1 y, L^-1 1, beta, 1'R^-1 1): ccgp_factor_batch
 * factorises S draws ONCE, ccgp_predict_from_factorset then serves any number of test sets at the cost
 * of their forward substitutions only (O(m n^2) per draw instead of O(n^3)); results are bit-identical to
 * ccgp_predict_batch.  For n <= 128 the set keeps the draws and the resident inputs only -- the fused
 * evaluator regenerates a factor in registers faster than it could be read back from HBM.
 * All S factors must fit on the device together (142 MB each at n = 4096); CCGP_ENOMEM otherwise.
 * out_loglik / out_beta / status (S each) may be NULL.  The converter that materialises the reference's
 * wide frame for drop-in callers is rsurface.factors_frame_from_draws. */
typedef struct ccgp_factorset ccgp_factorset;
int ccgp_factor_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                      const double* params, int S, double sigma2, ccgp_factorset** out,
                      double* out_loglik, double* out_beta, int* status);
/* out_mean / out_var: S x m column-major, as ccgp_predict_batch */
int ccgp_predict_from_factorset(ccgp_handle* h, const ccgp_factorset* fs, const double* Xtest, int m,
                                double* out_mean, double* out_var);
/* the summaries of ccgp_predict_summary (HX:686-703 / GV:620-638) from kept factors: same kernel, same bits; returns
 * the number of draws of the set that failed to factorise */
int ccgp_summary_from_factorset(ccgp_handle* h, const ccgp_factorset* fs, const double* Xtest, int m,
                                const double* probs, int n_probs, const double* y_at, double* out);
size_t ccgp_factorset_bytes(const ccgp_factorset* fs);
int ccgp_factorset_free(ccgp_handle* h, ccgp_factorset* fs);

/* literal factors(): out = (mean.factor[n], var.factor1[n], var.factor2).  R_inv is taken as the caller gives it, symmetric
 * or not (R's solve() output is symmetric only up to rounding): var.factor1 = apply(R.Inv, 2, sum) are COLUMN sums (HX:609),
 * mean.factor = R.Inv %*% (y - beta) row products (HX:608); ccgp_beta_mle forms (1' R.Inv) y / sum(R.Inv) (HX:387) likewise. */
int ccgp_factors(ccgp_handle* h, const double* R_inv, double beta, const double* y, int n,
                 double* out);
/* literal predict.post arithmetic with caller-supplied cached terms (HX:667-670);
 * r is m x n as produced by ccgp_mixed_corr_cross; out_mean/out_var length m. */
int ccgp_predict_from_factors(ccgp_handle* h, const double* r, int m, int n, double beta,
                              const double* mean_factor, const double* var_factor1,
                              double var_factor2, const double* R_inv, double sigma2,
                              double* out_mean, double* out_var);

/* predict.post(x.new, D.train, pars, sigma2) HX:655-673 as the scripts call it -- once per (draw, test site),
 * HX:688 -- in ONE device round trip: r = Mixed.corr.vec(x_t, D.train, ...) (HX:665, the kernel of
 * ccgp_mixed_corr_cross) for the m rows of Xnew, then the arithmetic of HX:667-670 with the caller's cached
 * terms (the frame row's beta, mean.factor, var.factor1, var.factor2, R.Inv: HX:659-663).  Same bits as
 * ccgp_mixed_corr_cross followed by ccgp_predict_from_factors; X, x.new, the parameter row and the n^2 + 2n cached
 * doubles cross PCIe in one pinned copy, (mean, var) come back in one. */
int ccgp_predict_post(ccgp_handle* h, const double* Xnew, int m, const double* X, int n, int d, int K,
                      const double* params_row, double beta, const double* mean_factor,
                      const double* var_factor1, double var_factor2, const double* R_inv, double sigma2,
                      double* out_mean, double* out_var);

/* ---- entropy criteria of the batch-sequential design script ---------------------------
 * Entropy(D, p, theta1, theta2) = -det(R.mixed(D))  (Batch Sequential ME Design.R:856-861) and
 * Augmented.Mixed.Entropy = -det(R.new - R.cross R.old^-1 R.cross') (same file :869-877), which by
 * the Schur complement equals -det(R.mixed(D.old U D.new)) / det(R.mixed(D.old)): both are log
 * determinants of the mixed correlation matrix of a CANDIDATE DESIGN.  Xs holds B designs of
 * n x d (column-major each, design b at Xs + b*n*d) that share ONE parameter row.  Up to 128 points (the reference's
 * candidate sets are a few dozen) all B designs are evaluated in one launch; larger designs run the blocked sweep one
 * design at a time. */
int ccgp_mixed_logdet_designs(ccgp_handle* h, const double* Xs, int n, int d, int B, int K,
                              const double* params, double* out_logdet, int* status);
/* The design search around those criteria (Entropy.optim / Batch.Entropy.optim, Batch Sequential ME Design.R:886-948;
 * the criteria themselves :856-877): log det R.mixed(D) as ccgp_mixed_logdet_designs computes it AND its gradient with
 * respect to the design,
 *   d log det R / d x_ik = -4 sum_{j != i} (R^-1)_ij (x_ik - x_jk) sum_q (w_q^2 / sum_r w_r^2) theta_qk exp(-theta_q'(x_i - x_j)^2),
 * for the rows i >= n_fixed.  Rows below n_fixed are the fixed batch D.old: they enter R and get no gradient, so with
 * n_fixed = n.old the gradient is that of the Schur criterion log det R(D.old U D.new) - log det R(D.old) (:869-877) too.
 * Xs, n, d, B, K and params as for ccgp_mixed_logdet_designs; out_logdet[B]; out_grad holds B blocks of (n - n_fixed) x d,
 * column-major each (design b at out_grad + b*(n - n_fixed)*d).  A design whose elimination meets a pivot <= 0 or not
 * finite (two coincident rows) gets status[b] != 0 and NaN log det and gradient; the others are unaffected.  One launch,
 * one workgroup per design, n <= 128 (CCGP_EUNSUPPORTED where the design does not fit); Gaussian family only;
 * CCGP_EINVAL for n_fixed outside [0, n).  Returns the number of failed designs. */
int ccgp_mixed_logdet_grad_designs(ccgp_handle* h, const double* Xs, int n, int d, int B, int K,
                                   const double* params, int n_fixed, double* out_logdet, double* out_grad,
                                   int* status);

/* ---- the maximum-entropy design search on the device: every start in one launch (Entropy.optim / Batch.Entropy.optim, -------------
 * Batch Sequential ME Design.R:886-948).  A start's variables are the free rows of its design in row-major order: nv =
 * (n - n_fixed) d, variable v = i d + k is free row i, dimension k.  The iterate IS the design -- nothing is transformed --, the
 * objective is f = -(log det R - ld_offset) (ld_offset = log det R(D.old) for the batch form, 0 otherwise) and g_v = -(d log det
 * R / d x_v), each one exactly rounded operation on what ccgp_mixed_logdet_grad_designs returns.  The state of a start is
 * ccgp_fit_begin's with d = nv (W = ccgp_fit_state_doubles(nv)); ccgp_fit_feed steps it on the host.  All starts share D_old
 * (n_fixed x d column-major, NULL iff n_fixed == 0) and one parameter row (K + K d values).
 * ccgp_design_fit_eval is the evaluation of B points (x, out_g: B blocks of nv in variable order) on the host side of
 * ccgp_mixed_logdet_grad_designs: it forms the B designs (D_old on top of block b's rows), calls ccgp_mixed_logdet_grad_designs
 * with that call's checks and routes -- so it serves every shape that call serves, nv > 64 included -- and transforms the
 * results.  ccgp_design_fit runs A starts on the device: one workgroup carries one start from its state through up to
 * max_evals[a] evaluations -- the design from `trial`, log det and its gradient from one factorisation, the step of
 * ccgp_fit_feed -- and writes the state back, so the next call continues it.  out_evals[a] is the number of evaluations made.
 * The trace (both or neither, [a T + t]): f and the pivot status of evaluation t of this call; NaN / -1 beyond out_evals[a].
 *   Bits.  Every evaluation inside ccgp_design_fit has the bits ccgp_mixed_logdet_grad_designs gives that design with that
 *     n_fixed.  A start driven evaluation by evaluation through ccgp_design_fit_eval and ccgp_fit_feed leaves the same state and
 *     trace, bit for bit.
 *   Independence.  A start depends on its own state and the shared inputs only: not on A, its position, what the handle ran
 *     before, or how its evaluations are cut into calls by max_evals.
 *   Failure.  A failed elimination (coincident rows) is an infeasible trial: f is the one quiet NaN, the gradient row is NaN,
 *     status is the 1-based pivot, and the line search backs off.  A start whose first point fails ends with code 5, its
 *     neighbours untouched.  The return value is the number of failed evaluations (ccgp_design_fit: over all starts).
 *   Arguments.  CCGP_EINVAL before anything is copied or launched, outputs and ccgp_workspace_bytes unchanged: bad shapes,
 *     n_fixed outside [0, n), D_old NULL with n_fixed > 0, A < 0 (B < 0), T < 0, max_evals[a] outside 0 .. min(T, 4096), a
 *     partial trace, a NULL required pointer (everything but D_old at n_fixed == 0, the trace and ccgp_design_fit_eval's
 *     status), a state whose recorded d is not nv.  CCGP_EUNSUPPORTED, outputs untouched: ccgp_design_fit for a family other
 *     than the Gaussian, n > 128, nv > 64 (the stepper's state ends there) or a design-gradient instance whose carve does not
 *     fit with the start's words behind it; ccgp_design_fit_eval where ccgp_mixed_logdet_grad_designs refuses.  A == 0 (B == 0)
 *     returns CCGP_OK.  A start that is not running, or whose max_evals is 0, is returned as it came.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging.  Not in this version: nv > 64, per-start parameter rows
 * or D_old, _dev variants, a ccgp_multi wrapper, an R shim. */
int ccgp_design_fit_eval(ccgp_handle* h, const double* D_old /* n_fixed x d column-major, NULL iff n_fixed == 0 */,
                         int n_fixed, int n, int d, int K, const double* params /* one row */, double ld_offset,
                         const double* x /* B blocks of nv, variable order */, int B,
                         double* out_f, double* out_g /* B blocks of nv */, int* status /* NULL ok */);
int ccgp_design_fit(ccgp_handle* h, const double* D_old, int n_fixed, int n, int d, int K, const double* params,
                    double ld_offset, int A, double* state /* A x W(nv), in and out */, const int* max_evals,
                    int* out_evals, double* trace_f, int* trace_status /* A x T, both or neither */, int T);

/* ---- the CGP refinement on the device: evaluate and step launches, no host trips (CGP's optim calls, GV:152-154) ------------------
 * A start's variables are w = (lambda, theta_1 .. theta_d, kappa, bw), P = d + 3, in its box [lo, hi]; the gradient is by central
 * differences of step `step` clipped at the box: up_j = min(w_j + step, hi_j), dn_j = max(w_j - step, lo_j).  One evaluation is
 * R = ccgp_cgp_fit_rows(d) = 1 + 2 P rows of ccgp_cgp_state_batch_sets: row 0 the centre, row 1 + 2 j variable j at up_j, row
 * 2 + 2 j at dn_j, each as the device row (v_0, v_1 .. v_d, v_k + v_{d+1}, v_{d+2}).  F = val where val is finite, else 1e6
 * (GV:130-131); f = F_0, g_j = (F_{1+2j} - F_{2+2j}) / (up_j - dn_j), status = the centre row's.  Every operation between the
 * stepper and the evaluator is exactly rounded (csrc/cgp_fit_logic.h), so host and device form the same rows and gradients.
 * The state of a start is ccgp_fit_begin's with d = P (W = ccgp_fit_state_doubles(P)); lo and hi are read from it.
 * ccgp_cgp_fit_eval_sets is the evaluation of B points (w, lo, hi, out_g: B x P column-major) on the host side of
 * ccgp_cgp_state_batch_sets: it forms the B R rows, calls ccgp_cgp_state_batch_sets with that call's checks, routes and
 * chunking, and transforms the results.  ccgp_cgp_fit_sets runs A starts, start a on training set set[a], on the device: it
 * stages the sets and states once, writes the first rows, and queues rounds of two launches on the handle's stream -- the gated
 * evaluation of every running start's R rows, then one wave per start that forms the gradient, takes the step of ccgp_fit_feed
 * and writes the start's next rows or closes its gate -- `look` rounds back to back before the host reads the A gate words,
 * until no gate is open.  It writes the states back, so the next call continues them.  out_evals[a] is the number of
 * evaluations made.  The trace (both or neither, [a T + t]): f and the centre row's pivot status of evaluation t of this call;
 * NaN / -1 beyond out_evals[a].
 *   Bits.  Every row evaluated inside ccgp_cgp_fit_sets has the bits ccgp_cgp_state_batch_sets gives it on its set.  A start
 *     driven evaluation by evaluation through ccgp_cgp_fit_eval_sets and ccgp_fit_feed leaves the same state and trace, bit for
 *     bit.
 *   Independence.  A start depends on its own state, its set and `step` only: not on A, its position, the other starts' sets,
 *     `look`, how its evaluations are cut into calls by max_evals, or what the handle's buffers held before.
 *   Failure.  A failed centre row is an infeasible trial: the line search backs off and the start goes on; a failed differenced
 *     row shows through the 1e6 only.  A start whose first point fails ends with code 5, its neighbours untouched.  The return
 *     value is the number of evaluations whose centre row failed, over all starts (all points).
 *   Arguments.  CCGP_EINVAL before anything is copied or launched, outputs and ccgp_workspace_bytes unchanged: bad shapes,
 *     C < 1, A < 0 (B < 0), T < 0, look outside 1 .. 64, step not finite or <= 0, set[a] outside 0 .. C-1, max_evals[a] outside
 *     0 .. min(T, 4096), a partial trace, a NULL required pointer (everything but the trace and ccgp_cgp_fit_eval_sets' status),
 *     a state whose recorded d is not P.  CCGP_EUNSUPPORTED, outputs untouched: where ccgp_cgp_state_batch_sets refuses; and for
 *     ccgp_cgp_fit_sets alone more than 64 variables (the stepper's state ends there), A R > 65535, or rows, results and states
 *     that do not fit under the workspace limit in one piece -- the twin serves these, its call chunks.  A == 0 (B == 0) returns
 *     CCGP_OK.  A start that is not running, or whose max_evals is 0, is returned as it came.
 * Host pointers only, blocking; ccgp_reserve does not cover the staging.  Not in this version: an analytic gradient, _dev
 * variants, a ccgp_multi wrapper, an R shim. */
int ccgp_cgp_fit_rows(int d);
int ccgp_cgp_fit_eval_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C,
                           const double* w /* B x P */, const double* lo, const double* hi /* B x P */, double step,
                           const int* set /* B */, int B, double* out_f, double* out_g /* B x P */, int* status /* NULL ok */);
int ccgp_cgp_fit_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int A, const int* set /* A */,
                      double* state /* A x W(P), in and out */, double step, const int* max_evals /* A */, int look,
                      int* out_evals /* A */, double* trace_f, int* trace_status /* A x T, both or neither */, int T);

/* ---- several GPUs behind ONE host process (csrc/multi.cpp) ------------------------------
 * The drop-in host is R: one single-threaded process.  A ccgp_multi owns one handle per device; the three
 * batched entry points below take the same arguments as their single-device forms, cut the batch into
 * contiguous shards (the grid by grid ROW, so that a row's mean over its Halton nodes stays on one device,
 * HX:574), run the shards concurrently and deliver every result in the caller's host buffers at the
 * shard's offset -- plain device-to-host copies: the consumer (which.max, HX:593-594) is the host, so an
 * all-gather into every GPU's memory would be a copy nobody reads.  Results are bit-identical to the
 * single-device call whatever the number of shards (every evaluation is computed by its own workgroups).
 * devices = NULL means 0 .. n_devices-1; a device may be listed more than once (shards then share it).
 * Return values as for the single-device calls (sum over shards of the failed evaluations; the first
 * negative shard return otherwise, message in ccgp_multi_last_error). */
typedef struct ccgp_multi ccgp_multi;
int ccgp_multi_create(int n_devices, const int* devices, ccgp_multi** out);
int ccgp_multi_destroy(ccgp_multi* m);
int ccgp_multi_count(const ccgp_multi* m);
ccgp_handle* ccgp_multi_handle(ccgp_multi* m, int i); /* per-shard handle: workspace limit, options */
const char* ccgp_multi_last_error(const ccgp_multi* m);
int ccgp_multi_set_kernel(ccgp_multi* m, int family, double nu);
int ccgp_multi_loglik_batch(ccgp_multi* m, const double* X, int n, int d, const double* y, int K,
                            const double* params, int B, double sigma2, int mean_mode, double tau2,
                            double* out_loglik, double* out_beta, int* status);
int ccgp_multi_grid_marginal(ccgp_multi* m, const double* X, int n, int d, const double* y, double sigma2,
                             const double* hyper, int G, int N, double tau, int take_log,
                             double aniso_lambda, double* out, int* out_argmax, double* out_logs);
int ccgp_multi_predict_batch(ccgp_multi* m, const double* X, int n, int d, const double* y, int K,
                             const double* params, int S, const double* Xtest, int mt, double sigma2,
                             double* out_mean, double* out_var, double* out_beta, int* status);

/* ---- measurement hooks (bench.py / rocprof; not part of the R surface) ---------------
 * Time, with HIP events on the handle's stream, every launch group of the most recent
 * *_dev call: ids below.  Returns milliseconds summed over launches and the count. */
enum {
  CCGP_T_COV = 0,      /* covariance / mix build            */
  CCGP_T_UPDATE = 1,   /* blocked Cholesky panel update (MFMA) */
  CCGP_T_DIAG = 2,     /* diagonal-block factor + inverse   */
  CCGP_T_TRSM = 3,     /* panel triangular solve (MFMA)     */
  CCGP_T_SOLVE = 4,    /* forward solves + reductions       */
  CCGP_T_FUSED = 5,    /* small-n fused evaluators (n <= 128) */
  CCGP_T_SWEEP = 6,    /* blocked Cholesky sweep as one scheduled launch (update + diag + trsm tiles) */
  CCGP_T_COUNT = 7
};
/* on = 0: off; 1: every id; otherwise a mask with bit (1 + id) set for each id to time */
int ccgp_enable_timing(ccgp_handle* h, int on);
int ccgp_get_timing(ccgp_handle* h, int id, double* out_ms, int* out_launches);
/* With CCGP_OPT_SCHED_POLICY bit 2 set, the scheduled sweep keeps a time account per workgroup (8 words each, ticks of 10 ns:
 * waiting for a task, in diagonal / update / panel-solve tiles, applying arrivals; then tasks run, XCD served, 1 if second on
 * its CU).  Copies the account of the LAST scheduled sweep (synchronises the stream). */
int ccgp_last_sched_profile(ccgp_handle* h, unsigned long long* out, int max_workgroups, int* out_workgroups);
/* Bytes of device scratch the handle holds now: the workspace (sweep matrices, kept factors) and the staging buffer.
 * Both grow only; a figure that changed across a call means the call allocated.  Does not synchronise.  Either may be NULL. */
int ccgp_workspace_bytes(const ccgp_handle* h, size_t* ws_bytes, size_t* stage_bytes);
/* Tests only: make what a call finds in the handle's scratch a chosen value instead of whatever an earlier call (or a fresh
 * allocation, usually zero pages) left there.  byte in 0 .. 255: fills the device workspace and the device staging buffer
 * with that byte on the handle's stream and the pinned host buffer after a stream synchronise, forgets the scheduler's
 * time account (it lies in that memory), and from now on fills every buffer the handle allocates -- a regrown workspace,
 * staging or pinned buffer, the memory of a factor set -- right after the allocation.  byte = -1 (the default) turns the
 * fill on allocation off; anything else is CCGP_EINVAL.  No result may depend on the byte.  May synchronise. */
int ccgp_debug_fill_scratch(ccgp_handle* h, int byte);

#ifdef __cplusplus
}
#endif
#endif /* CCGP_H */
