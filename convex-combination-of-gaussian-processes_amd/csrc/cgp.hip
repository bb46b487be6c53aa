// The composite GP of Ba & Joseph, the third model of compare.GP's table: the state that CGP's objective var.MLE.DK
// (GV:102-133), its jackknife (GV:167-198) and its final fit (GV:200-221) all run, and predict.CGP (GV:287-307) from a kept
// state.  n <= 128, Gaussian correlations only (the reference has no other CGP).
//
// cgp_state_kernel: one workgroup per evaluation (parameter row, optional held-out row).  The design (without the held-out
// row) is copied to LDS once; per pass
//
//      Q = G(theta) + lambda diag(sqrt s) L(alpha) diag(sqrt s)
//
// is built in the lower triangle of an LDS matrix with y' and 1' as extra rows and factorised in place as L' D L'^T exactly
// as small.hip does (one barrier per column; the extra rows come out forward-substituted).  Then, by wave 0,
// beta = 1'Q^-1 y / 1'Q^-1 1 as D-weighted dot products of those rows and temp = Q^-1 (y - beta 1) by a column-oriented back
// substitution held in registers (lane l owns entries l and l + 64; a step is one broadcast and two LDS reads); then, by all
// waves, e = y - beta - G temp and s = (Gbw e^2) / (Gbw 1), one wave per row.  Four such passes and a fifth factorisation:
// the loop count is fixed, nothing in the input keeps a workgroup running.
//
// Where G, L and Gbw live: at n = 128 the working matrix takes 134 of the 160 KB, so three more n x n matrices cannot stay
// resident and the handle's workspace would put 3 n^2 doubles per evaluation and pass through HBM.  But the factorisation
// never touches the strict UPPER triangle of the working matrix: G is written there by the first pass's fill (entry (i, j),
// i > j, at row j of column i) and read back by the four later fills and by every G temp product, at no exp at all.  L is
// needed by the fill only and is recomputed there from the LDS copy of X (n^2 / 2 exps a pass); Gbw is needed by the
// reweighting only and is recomputed there (n^2 exps a pass).  The leading dimension is odd, so the row-wise reads of the
// upper triangle and of the back substitution spread over the LDS banks.
//
// Bound: neither HBM nor MFMA -- five n-step dependent chains (a barrier per column) plus five n-step broadcast chains in one
// wave, over LDS-resident data; HBM traffic is X, y and the parameter row in and four doubles out.
//
// cgp_predict_kernel: one wave per test site against the state a `keep` evaluation left in HBM (the normalised factor, Q^-1 1,
// temp, s, e^2 and five scalars).  q'Q^-1 q comes from a forward substitution of q through the kept factor, columns streamed
// from L2 one step ahead, never from an inverse.
//
// Over many training sets of one shape (ccgp_cgp_predict_sets): cgp_state_kernel<sets, keep> leaves the state of EVERY row,
// each on its own set, and cgp_predict_kernel<sets> serves rows x sites from them, each row at its own set's test sites.  Both
// are template instances beside the single-set ones and run the single-set code behind their loads: a row has the bits of
// ccgp_cgp_predict on its set alone.
#include <type_traits>

#include "ccgp_internal.h"
#include "cgp_fit_logic.h"

namespace ccgp {

namespace {

struct CgpStateArgs {
  const double* X;        // n x d column-major
  const double* y;
  int n, d;
  const double* params;   // nb x (2 d + 2) column-major, leading dimension ldp: lambda | theta[d] | alpha[d] | bw
  int ldp;
  const int* skip;        // nb held-out rows (-1: none) or nullptr
  double *val, *beta, *tau2, *loo;   // nb each; loo may be nullptr
  int* status;
  double* keep;           // CgpKeep(n) of evaluation 0, or nullptr
  const int* set;         // SETS: evaluation b belongs to training set set[b]: X + set[b] n d, y + set[b] n
  const int* gate;        // GATED: evaluation b runs only where gate[b / gate_rows] != 0
  int gate_rows;
};

__device__ inline double cgp_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// every exponential of this file: exp(-dist) with the range select (ccgp_internal.h exp_poly_ranged), exactly 0 beyond exp's range
__device__ __forceinline__ double cgp_exp(double dist) { return exp_poly_ranged(dist); }

// sum_k rate_k (a_k - b_k)^2 from the direct differences, as Stand_PSI forms it (GV:96-99): exactly 0 for coincident points
__device__ __forceinline__ double cgp_dist(const double* xs, int ldx, int i, int j, const double* rate, int d) {
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double df = xs[k * ldx + i] - xs[k * ldx + j];
    s = fma(df * df, rate[k], s);
  }
  return s;
}
__device__ __forceinline__ double cgp_dist_to(const double* xs, int ldx, int j, const double* x0, const double* rate, int d) {
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double df = xs[k * ldx + j] - x0[k];
    s = fma(df * df, rate[k], s);
  }
  return s;
}

// SETS: many training sets of one shape in one launch (ccgp_cgp_state_batch_sets): the evaluation's design and responses come
// from its set, everything after the loads is the single-set instance's code, hence its bits.  A template parameter, not a
// branch, for the reason small_reg.hip gives for PROF and SETS: the single-set instance compiles from unchanged code.  The
// sets form of the fits keeps no state (`keep` does not exist there).
// KEEP: the sets form of the prediction (ccgp_cgp_predict_sets): EVERY evaluation leaves its CgpKeep(n) block, evaluation b at
// keep + b CgpKeep(n).total, for cgp_predict_kernel<sets> behind it in the stream.  A third switch for the same reason: what it
// adds (Q^-1 1 in the last back substitution, the epilogue) is the single-set instance's code for its evaluation 0.
// GATED: the evaluations of the refinement on the device (ccgp_cgp_fit_sets): gate_rows consecutive evaluations belong to one
// start, and a workgroup whose start has stopped leaves at once -- before any LDS write or barrier, the whole workgroup on one
// word.  A workgroup that stays runs the sets instance's code.  A second switch for the same reason as the first.
template <bool SETS, bool GATED = false, bool KEEP = false>
__global__ __launch_bounds__(256) void cgp_state_kernel(CgpStateArgs a) {
  static_assert(!KEEP || (SETS && !GATED), "the keeping sets instance is the plain sets instance plus the kept state");
  // the instances that can leave a state.  They form Q^-1 1 in EVERY evaluation once `keep` is set, although the single-set
  // instance keeps evaluation 0 only: the u chain shares nothing with the others, so no bit depends on it
  constexpr bool kKeeps = !SETS || KEEP;
  if constexpr (GATED) {
    if (a.gate[blockIdx.x / a.gate_rows] == 0) return;   // uniform: every thread reads the same word
  }
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int n0 = a.n, d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const CgpCarve cv(n0, d);
  const int ld = cv.ld;
  double *A = smem + cv.A, *xs = smem + cv.xs, *yv = smem + cv.yv, *s = smem + cv.s, *rs = smem + cv.rs, *sn = smem + cv.sn,
         *e2 = smem + cv.e2, *tv = smem + cv.tv, *uv = smem + cv.uv, *x0 = smem + cv.x0, *th = smem + cv.th, *al = smem + cv.al,
         *tb = smem + cv.tb, *red = smem + cv.red;

  const double *X = a.X, *y = a.y;
  if constexpr (SETS) {
    const int st = __builtin_amdgcn_readfirstlane(a.set[b]);   // wave-uniform: the addresses stay in scalar registers
    X += (size_t)st * n0 * d;
    y += (size_t)st * n0;
  }
  int skip = a.skip ? a.skip[b] : -1;
  if (skip < 0 || skip >= n0) skip = -1;
  const int n = skip >= 0 ? n0 - 1 : n0;            // points of this evaluation
  const int Rt = n + 2;
  const double lam = a.params[b];
  const double bw = a.params[b + (size_t)(1 + 2 * d) * a.ldp];
  for (int k = tid; k < d; k += 256) {
    const double t = a.params[b + (size_t)(1 + k) * a.ldp];
    th[k] = t;
    tb[k] = t * bw;
    al[k] = a.params[b + (size_t)(1 + d + k) * a.ldp];
    x0[k] = skip >= 0 ? X[(size_t)k * n0 + skip] : 0.0;
  }
  for (int e = tid; e < n * d; e += 256) {
    const int k = e / n, i = e % n;
    xs[k * n0 + i] = X[(size_t)k * n0 + i + (skip >= 0 && i >= skip ? 1 : 0)];
  }
  for (int i = tid; i < n; i += 256) {
    yv[i] = y[i + (skip >= 0 && i >= skip ? 1 : 0)];
    s[i] = 1.0;
    rs[i] = 1.0;
  }
  __syncthreads();

  const double tol = pivot_tolerance(0, n);   // the reference calls solve(Q): base R's rule, as the mode-0 likelihood
  int bad = 0;
  double beta = 0.0, sf = 0.0;
  for (int rep = 0; rep < 5; ++rep) {
    // ---- fill: column j, rows j..n+1; G goes to / comes from the strict upper triangle ---------------------------------
    for (int j = wave; j < n; j += 4) {
      const double rsj = rs[j];
      for (int i = j + lane; i < Rt; i += 64) {
        double v;
        if (i == j) {
          v = fma(lam, rs[i] * rsj, 1.0);
        } else if (i < n) {
          double g;
          if (rep == 0) {
            g = cgp_exp(cgp_dist(xs, n0, i, j, th, d));
            A[j + (size_t)i * ld] = g;
          } else {
            g = A[j + (size_t)i * ld];
          }
          const double l = cgp_exp(cgp_dist(xs, n0, i, j, al, d));
          v = fma(lam, (rs[i] * l) * rsj, g);
        } else {
          v = i == n ? yv[j] : 1.0;
        }
        A[i + (size_t)j * ld] = v;
      }
    }
    // ---- Q = L' D L'^T, one barrier per column (small.hip) --------------------------------------------------------------
    for (int k = 0; k < n; ++k) {
      __syncthreads();
      const double piv = A[k + (size_t)k * ld];
      if (!(piv > tol)) { bad = k + 1; break; }   // uniform: every thread reads the same word
      const double rinv = 1.0 / piv;
      const double* colk = A + (size_t)k * ld;
      for (int j = k + 1 + wave; j < n; j += 4) {
        const double ljk = colk[j] * rinv;
        double* colj = A + (size_t)j * ld;
        for (int i = j + lane; i < Rt; i += 64) colj[i] = fma(-colk[i], ljk, colj[i]);
      }
    }
    __syncthreads();
    if (bad) break;   // uniform

    // ---- wave 0: beta, temp (and on the last pass the quadratic form, log det and Q^-1 1) --------------------------------
    if (wave == 0) {
      const int i0 = lane, i1 = lane + 64;
      const double d0 = i0 < n ? A[i0 + (size_t)i0 * ld] : 1.0, d1 = i1 < n ? A[i1 + (size_t)i1 * ld] : 1.0;
      const double zy0 = i0 < n ? A[n + (size_t)i0 * ld] : 0.0, zy1 = i1 < n ? A[n + (size_t)i1 * ld] : 0.0;
      const double z10 = i0 < n ? A[n + 1 + (size_t)i0 * ld] : 0.0, z11 = i1 < n ? A[n + 1 + (size_t)i1 * ld] : 0.0;
      const double rd0 = 1.0 / d0, rd1 = 1.0 / d1;
      const double s11 = cgp_wave_sum(fma(z11 * z11, rd1, z10 * z10 * rd0));
      const double s1y = cgp_wave_sum(fma(z11 * zy1, rd1, z10 * zy0 * rd0));
      beta = s1y / s11;
      const double r0 = zy0 - beta * z10, r1 = zy1 - beta * z11;
      const bool last = rep == 4;
      if (last) {
        const double quad = cgp_wave_sum(fma(r1 * r1, rd1, r0 * r0 * rd0));
        const double logdet = cgp_wave_sum((i0 < n ? log(d0) : 0.0) + (i1 < n ? log(d1) : 0.0));
        if (lane == 0) { red[2] = quad / n; red[3] = logdet; red[4] = s11; }
      }
      // L'^T x = D^-1 z, column-oriented: x_k is final once every k' > k has been applied; then row k of L' (entries
      // A[k + i ld] / d_i, i < k) carries it into the entries above
      double t0 = r0 * rd0, t1 = r1 * rd1;          // temp
      double u0 = z10 * rd0, u1 = z11 * rd1;        // Q^-1 1 (kept state only)
      const bool want_u = kKeeps && last && a.keep != nullptr;
      for (int k = n - 1; k > 0; --k) {
        const double xk = __shfl(k < 64 ? t0 : t1, k & 63, 64);
        const double c0 = i0 < k ? A[k + (size_t)i0 * ld] * rd0 : 0.0;
        const double c1 = i1 < k ? A[k + (size_t)i1 * ld] * rd1 : 0.0;
        t0 = fma(-c0, xk, t0);
        t1 = fma(-c1, xk, t1);
        if (want_u) {
          const double uk = __shfl(k < 64 ? u0 : u1, k & 63, 64);
          u0 = fma(-c0, uk, u0);
          u1 = fma(-c1, uk, u1);
        }
      }
      if (i0 < n) { tv[i0] = t0; uv[i0] = u0; }
      if (i1 < n) { tv[i1] = t1; uv[i1] = u1; }
      if (lane == 0) red[0] = beta;
    }
    __syncthreads();
    beta = red[0];
    if (rep == 4) break;

    // ---- e = y - beta - G temp, one wave per row -------------------------------------------------------------------------
    for (int i = wave; i < n; i += 4) {
      double acc = 0.0;
      for (int j = lane; j < n; j += 64) {
        const double g = j == i ? 1.0 : (j > i ? A[i + (size_t)j * ld] : A[j + (size_t)i * ld]);
        acc = fma(g, tv[j], acc);
      }
      acc = cgp_wave_sum(acc);
      if (lane == 0) {
        const double e = (yv[i] - beta) - acc;
        e2[i] = e * e;
      }
    }
    __syncthreads();
    // ---- s = (Gbw e^2) / (Gbw 1), Gbw recomputed --------------------------------------------------------------------------
    for (int i = wave; i < n; i += 4) {
      double num = 0.0, den = 0.0;
      for (int j = lane; j < n; j += 64) {
        const double gb = cgp_exp(cgp_dist(xs, n0, i, j, tb, d));
        num = fma(gb, e2[j], num);
        den += gb;
      }
      num = cgp_wave_sum(num);
      den = cgp_wave_sum(den);
      if (lane == 0) sn[i] = num / den;
    }
    __syncthreads();
    {
      double t = 0.0;
      for (int j = lane; j < n; j += 64) t += sn[j];   // every wave forms the same sum in the same order
      sf = cgp_wave_sum(t) / n;
      for (int i = tid; i < n; i += 256) {
        const double si = sn[i] / sf;
        s[i] = si;
        rs[i] = sqrt(si);
      }
    }
    __syncthreads();
  }

  // ---- results --------------------------------------------------------------------------------------------------------------
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const double tau2 = bad ? kNaN : red[2];
  if (wave == 0) {
    double loo = kNaN;
    if (!bad && skip >= 0 && a.loo) {
      // predict.CGP's arithmetic for the held-out point (GV:191-197): e^2 and sf are the fourth pass's, s the final one
      double num = 0.0, den = 0.0;
      for (int j = lane; j < n; j += 64) {
        const double gb = cgp_exp(cgp_dist_to(xs, n0, j, x0, tb, d));
        num = fma(gb, e2[j], num);
        den += gb;
      }
      num = cgp_wave_sum(num);
      den = cgp_wave_sum(den);
      const double v = (num / den) / sf;
      const double lsv = lam * sqrt(v);
      double acc = 0.0;
      for (int j = lane; j < n; j += 64) {
        const double g = cgp_exp(cgp_dist_to(xs, n0, j, x0, th, d));
        const double l = cgp_exp(cgp_dist_to(xs, n0, j, x0, al, d));
        acc = fma(fma(lsv * rs[j], l, g), tv[j], acc);
      }
      loo = beta + cgp_wave_sum(acc);
    }
    if (lane == 0) {
      a.val[b] = bad ? kNaN : red[3] + n * log(tau2);
      a.beta[b] = bad ? kNaN : beta;
      a.tau2[b] = tau2;
      if (a.loo) a.loo[b] = loo;
      a.status[b] = bad;
    }
  }
  if (kKeeps && a.keep && (KEEP || b == 0) && !bad) {
    const CgpKeep kp(n);
    double* K = a.keep + (KEEP ? (size_t)b * kp.total : 0);
    for (int e = tid; e < n * n; e += 256) {
      const int i = e % n, k = e / n;
      double v = 0.0;
      if (i == k) v = A[k + (size_t)k * ld];
      else if (i > k) v = A[i + (size_t)k * ld] / A[k + (size_t)k * ld];
      K[kp.F + e] = v;
    }
    for (int i = tid; i < n; i += 256) {
      K[kp.u + i] = uv[i];
      K[kp.temp + i] = tv[i];
      K[kp.s + i] = s[i];
      K[kp.res2 + i] = e2[i];
    }
    if (tid == 0) {
      K[kp.sc + 0] = sf;
      K[kp.sc + 1] = beta;
      K[kp.sc + 2] = tau2;
      K[kp.sc + 3] = red[4];   // 1'Q^-1 1
    }
  }
}

struct CgpPredictArgs {
  const double* X;        // n x d
  int n, d;
  const double* row;      // the parameter row, contiguous (2 d + 2)
  const double* Xtest;    // m x d column-major
  int m;
  const double* keep;     // CgpKeep(n)
  const int* status;      // of the kept state
  double* out;            // m x 6 column-major: Yp gp lp v Y_low Y_up
};

// the sets form (ccgp_cgp_predict_sets): row r = blockIdx.y of the call has its own kept state (keep + r CgpKeep(n).total),
// parameter row (row + r, leading dimension ldp), status word and output block (out + r 6 m), and reads the design and the
// test sites of its set: X and Xtest are then the C blocks of all sets
struct CgpPredictSetsArgs : CgpPredictArgs {
  const int* set;         // rows
  int ldp;
};

// one wave per site; lane l owns design points l and l + 64.  SETS is a template parameter, not a branch, as in
// cgp_state_kernel: the single-set instance compiles from unchanged code, and the sets instance narrows its arguments to its
// row and then runs that code, hence its bits.
template <bool SETS>
__global__ __launch_bounds__(256) void cgp_predict_kernel(std::conditional_t<SETS, CgpPredictSetsArgs, CgpPredictArgs> a) {
  if constexpr (SETS) {
    const int r = blockIdx.y;
    const int st = __builtin_amdgcn_readfirstlane(a.set[r]);   // wave-uniform: the addresses stay in scalar registers
    a.X += (size_t)st * a.n * a.d;
    a.Xtest += (size_t)st * a.m * a.d;
    a.row += r;
    a.keep += (size_t)r * CgpKeep(a.n).total;
    a.status += r;
    a.out += (size_t)r * a.m * 6;
  }
  size_t ldp = 1;   // entry j of the parameter row is row[j ldp]: contiguous, or a row of the column-major table
  if constexpr (SETS) ldp = (size_t)a.ldp;
  const int n = a.n, d = a.d, m = a.m;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= m) return;   // whole waves leave; no barrier below
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  if (a.status[0] != 0) {
    if (lane < 6) a.out[t + (size_t)lane * m] = kNaN;
    return;
  }
  const CgpKeep kp(n);
  const double* K = a.keep;
  const double* F = K + kp.F;
  const double lam = a.row[0], bw = a.row[(1 + 2 * d) * ldp];
  const int i0 = lane, i1 = lane + 64;
  const bool h0 = i0 < n, h1 = i1 < n;
  double dt0 = 0.0, dt1 = 0.0, da0 = 0.0, da1 = 0.0;
  for (int k = 0; k < d; ++k) {
    const double xt = a.Xtest[t + (size_t)k * m], thk = a.row[(1 + k) * ldp], alk = a.row[(1 + d + k) * ldp];
    if (h0) { const double df = a.X[i0 + (size_t)k * n] - xt; dt0 = fma(df * df, thk, dt0); da0 = fma(df * df, alk, da0); }
    if (h1) { const double df = a.X[i1 + (size_t)k * n] - xt; dt1 = fma(df * df, thk, dt1); da1 = fma(df * df, alk, da1); }
  }
  // g, gbw, l against the n design points (GV:288-292)
  const double g0 = h0 ? cgp_exp(dt0) : 0.0, g1 = h1 ? cgp_exp(dt1) : 0.0;
  const double b0 = h0 ? cgp_exp(dt0 * bw) : 0.0, b1 = h1 ? cgp_exp(dt1 * bw) : 0.0;
  const double l0 = h0 ? cgp_exp(da0) : 0.0, l1 = h1 ? cgp_exp(da1) : 0.0;
  const double e20 = h0 ? K[kp.res2 + i0] : 0.0, e21 = h1 ? K[kp.res2 + i1] : 0.0;
  const double tp0 = h0 ? K[kp.temp + i0] : 0.0, tp1 = h1 ? K[kp.temp + i1] : 0.0;
  const double rs0 = h0 ? sqrt(K[kp.s + i0]) : 0.0, rs1 = h1 ? sqrt(K[kp.s + i1]) : 0.0;
  const double uu0 = h0 ? K[kp.u + i0] : 0.0, uu1 = h1 ? K[kp.u + i1] : 0.0;
  const double sf = K[kp.sc + 0], beta = K[kp.sc + 1], tau2 = K[kp.sc + 2], s11 = K[kp.sc + 3];
  const double num = cgp_wave_sum(fma(b1, e21, b0 * e20)), den = cgp_wave_sum(b0 + b1);
  const double v = (num / den) / sf;                                   // GV:293
  const double lsv = lam * sqrt(v);
  const double ls0 = l0 * rs0, ls1 = l1 * rs1;
  double q0 = fma(lsv, ls0, g0), q1 = fma(lsv, ls1, g1);               // GV:294
  const double Yp = beta + cgp_wave_sum(fma(q1, tp1, q0 * tp0));       // GV:295
  const double gp = beta + cgp_wave_sum(fma(g1, tp1, g0 * tp0));       // GV:296
  const double lp = lsv * cgp_wave_sum(fma(ls1, tp1, ls0 * tp0));      // GV:298
  const double qu = cgp_wave_sum(fma(q1, uu1, q0 * uu0));              // q'Q^-1 1
  // q'Q^-1 q = sum_k z_k^2 / d_k with z = L'^-1 q: forward substitution, the next column of the factor in flight
  const double dd0 = h0 ? F[i0 + (size_t)i0 * n] : 1.0, dd1 = h1 ? F[i1 + (size_t)i1 * n] : 1.0;
  double qq = 0.0;
  double c0 = (h0 && i0 > 0) ? F[i0] : 0.0, c1 = h1 ? F[i1] : 0.0;     // column 0
  for (int k = 0; k < n; ++k) {
    double nc0 = 0.0, nc1 = 0.0;
    if (k + 1 < n) {
      if (h0 && i0 > k + 1) nc0 = F[i0 + (size_t)(k + 1) * n];
      if (h1 && i1 > k + 1) nc1 = F[i1 + (size_t)(k + 1) * n];
    }
    const double zk = __shfl(k < 64 ? q0 : q1, k & 63, 64);
    const double dk = __shfl(k < 64 ? dd0 : dd1, k & 63, 64);
    qq = fma(zk * zk, 1.0 / dk, qq);
    q0 = fma(-c0, zk, q0);   // c is 0 at and above the diagonal: entries already final stay as they are
    q1 = fma(-c1, zk, q1);
    c0 = nc0;
    c1 = nc1;
  }
  const double w = 1.0 - qu;
  double ppp = ((1.0 + lam * v) - qq) + w * w / s11;                   // GV:299
  if (ppp < 0.0) ppp = 0.0;                                            // GV:303
  const double half = 1.96 * sqrt(tau2 * ppp);                         // GV:304-306
  if (lane == 0) {
    a.out[t] = Yp;
    a.out[t + (size_t)1 * m] = gp;
    a.out[t + (size_t)2 * m] = lp;
    a.out[t + (size_t)3 * m] = v;
    a.out[t + (size_t)4 * m] = Yp - half;
    a.out[t + (size_t)5 * m] = Yp + half;
  }
}

// The step of the refinement on the device (ccgp_cgp_fit_sets): one wave per start, behind the gated evaluation of the start's
// R = 1 + 2 P rows in the same stream.  The state comes to LDS; lane j < P forms g_j from the values of rows 1 + 2 j and
// 2 + 2 j (cgp_fit_logic.h) and leaves it in LDS; lane 0 runs fit_feed on the state with f = F_0 and the centre row's status
// and appends both to the trace; the state goes back.  Where the start is still running and has evaluations left, the lanes
// write its next R parameter rows (and the rows' set); otherwise its gate closes and neither kernel touches the start again.
// init: no evaluation has been made yet -- the counters are zeroed and the first rows written.  No path waits on another
// workgroup: the order of evaluation and step is the stream's.
__global__ __launch_bounds__(64) void cgp_fit_step_kernel(CgpFitIO io, int d, int init) {
  extern __shared__ __attribute__((aligned(16))) double fsm[];
  const int a = blockIdx.x, lane = threadIdx.x;
  if (!init && io.gate[a] == 0) return;   // uniform
  const int P = cgp_fit_vars(d), R = cgp_fit_rows(d), NC = cgp_fit_cols(d), W = io.W;
  double* sg = io.state + (size_t)a * W;
  double *st = fsm, *g = fsm + W, *cnt = fsm + W + P;
  for (int e = lane; e < W; e += 64) st[e] = sg[e];
  __syncthreads();
  const size_t b0 = (size_t)a * R;
  const double *w = fit_trial(st, P), *lo = fit_lo(st, P), *hi = fit_hi(st, P);
  if (!init) {
    for (int j = lane; j < P; j += 64)
      g[j] = cgp_fit_grad(io.val[b0 + 1 + 2 * j], io.val[b0 + 2 + 2 * j], w[j], io.step, lo[j], hi[j]);
    __syncthreads();
    if (lane == 0) {
      const double f = cgp_fit_value(io.val[b0]);
      const int bad = io.status[b0];
      const int t = io.evals[a];   // < max_evals[a] <= T: the gate was open
      if (io.tr_f) {
        const size_t at = (size_t)a * io.T + t;
        io.tr_f[at] = f;
        io.tr_status[at] = bad;
      }
      fit_feed(st, f, g, bad == 0);
      io.evals[a] = t + 1;
      io.nfail[a] += bad != 0;
      cnt[0] = (double)(t + 1);
    }
    __syncthreads();
    for (int e = lane; e < W; e += 64) sg[e] = st[e];
  } else if (lane == 0) {
    io.evals[a] = 0;
    io.nfail[a] = 0;
  }
  const int made = init ? 0 : (int)cnt[0];
  const bool go = st[kFitCode] == (double)kFitRunning && made < io.max_evals[a];   // uniform
  if (go) {
    const int st_a = io.set[a];
    for (int e = lane; e < R * NC; e += 64) {
      const int r = e % R, c = e / R;
      io.rows[b0 + r + (size_t)c * io.ldp] = cgp_fit_row_entry(w, lo, hi, io.step, d, r, c);
    }
    for (int r = lane; r < R; r += 64) io.row_set[b0 + r] = st_a;
  }
  if (lane == 0) io.gate[a] = go ? 1 : 0;
}

}  // namespace

void launch_cgp_state(hipStream_t st, const double* X, int n, int d, const double* y, const double* params, int ldp, int nb,
                      const int* skip, double* val, double* beta, double* tau2, double* loo, int* status, double* keep) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] { raise_lds_limit((const void*)cgp_state_kernel<false>, "cgp_state_kernel"); });
  CgpStateArgs a{};
  a.X = X; a.y = y; a.n = n; a.d = d; a.params = params; a.ldp = ldp; a.skip = skip;
  a.val = val; a.beta = beta; a.tau2 = tau2; a.loo = loo; a.status = status; a.keep = keep;
  hipLaunchKernelGGL(cgp_state_kernel<false>, dim3(nb), dim3(256), sizeof(double) * CgpCarve(n, d).total, st, a);
}

void launch_cgp_state_sets(hipStream_t st, const double* Xs, int n, int d, const double* ys, const int* set,
                           const double* params, int ldp, int nb, const int* skip, double* val, double* beta, double* tau2,
                           double* loo, int* status) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask, [] { raise_lds_limit((const void*)cgp_state_kernel<true>, "cgp_state_kernel<sets>"); });
  CgpStateArgs a{};
  a.X = Xs; a.y = ys; a.n = n; a.d = d; a.params = params; a.ldp = ldp; a.skip = skip; a.set = set;
  a.val = val; a.beta = beta; a.tau2 = tau2; a.loo = loo; a.status = status;
  hipLaunchKernelGGL(cgp_state_kernel<true>, dim3(nb), dim3(256), sizeof(double) * CgpCarve(n, d).total, st, a);
}

void launch_cgp_state_sets_keep(hipStream_t st, const double* Xs, int n, int d, const double* ys, const int* set,
                                const double* params, int ldp, int nb, double* val, double* beta, double* tau2, int* status,
                                double* keep) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask,
                  [] { raise_lds_limit((const void*)cgp_state_kernel<true, false, true>, "cgp_state_kernel<sets, keep>"); });
  CgpStateArgs a{};
  a.X = Xs; a.y = ys; a.n = n; a.d = d; a.params = params; a.ldp = ldp; a.set = set;
  a.val = val; a.beta = beta; a.tau2 = tau2; a.status = status; a.keep = keep;
  hipLaunchKernelGGL((cgp_state_kernel<true, false, true>), dim3(nb), dim3(256), sizeof(double) * CgpCarve(n, d).total, st, a);
}

void launch_cgp_state_gated(hipStream_t st, const double* Xs, int n, int d, const double* ys, const CgpFitIO& io, int A) {
  static unsigned long long attr_mask = 0;
  once_per_device(attr_mask,
                  [] { raise_lds_limit((const void*)cgp_state_kernel<true, true>, "cgp_state_kernel<sets, gated>"); });
  CgpStateArgs a{};
  a.X = Xs; a.y = ys; a.n = n; a.d = d; a.params = io.rows; a.ldp = io.ldp; a.set = io.row_set;
  a.val = io.val; a.beta = io.beta; a.tau2 = io.tau2; a.status = io.status;
  a.gate = io.gate; a.gate_rows = cgp_fit_rows(d);
  hipLaunchKernelGGL((cgp_state_kernel<true, true>), dim3(A * cgp_fit_rows(d)), dim3(256),
                     sizeof(double) * CgpCarve(n, d).total, st, a);
}

void launch_cgp_fit_step(hipStream_t st, int d, int A, const CgpFitIO& io, bool init) {
  const size_t lds = sizeof(double) * ((size_t)io.W + cgp_fit_vars(d) + 1);
  hipLaunchKernelGGL(cgp_fit_step_kernel, dim3(A), dim3(64), lds, st, io, d, init ? 1 : 0);
}

void launch_cgp_predict(hipStream_t st, const double* X, int n, int d, const double* row, const double* Xtest, int m,
                        const double* keep, const int* status, double* out) {
  CgpPredictArgs a{X, n, d, row, Xtest, m, keep, status, out};
  hipLaunchKernelGGL(cgp_predict_kernel<false>, dim3((m + 3) / 4), dim3(256), 0, st, a);
}

void launch_cgp_predict_sets(hipStream_t st, const double* Xs, int n, int d, const int* set, const double* params, int ldp,
                             int nb, const double* Xtests, int m, const double* keep, const int* status, double* out) {
  CgpPredictSetsArgs a{{Xs, n, d, params, Xtests, m, keep, status, out}, set, ldp};
  hipLaunchKernelGGL(cgp_predict_kernel<true>, dim3((m + 3) / 4, nb), dim3(256), 0, st, a);
}

}  // namespace ccgp
