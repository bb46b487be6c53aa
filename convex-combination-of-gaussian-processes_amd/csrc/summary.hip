// Posterior-predictive summaries of prediction() (HX:686-703, GV:620-638) on the S x m tables that the prediction left in
// device memory.  Per test site the predictive is the equal-weight mixture of the S' normals N(mean_s, var_s) of the
// draws that factorised (status == 0):
//   F(q)     = 1/S' sum_s Phi((q - mu_s) / sigma_s),  sigma_s = sqrt(max(var_s, 0)); sigma_s = 0 is a step at mu_s
//   y_hat    = 1/S' sum mu_s                     pred_var = 1/S' sum sigma_s^2 + 1/S' sum (mu_s - y_hat)^2  (two passes)
//   quant    = 1 - F(y_hat)                      cdf_at   = F(y_at)
//   q_j      = inf{q : F(q) >= probs[j]}
// One workgroup per site.  Every sum runs in one fixed order -- thread tid takes the valid draws tid, tid + 256, ...,
// then a shuffle tree per wave, then the four waves left to right -- so a site's numbers depend on nothing but its own
// column of the tables.  Both tails go through erfc: levels <= 1/2 are solved on F, levels > 1/2 on 1 - F.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "ccgp_internal.h"

namespace ccgp {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kInvSqrt2Pi = 0.39894228040143267794;
// the first bracket is [min(mu - c sigma), max(mu + c sigma)]: Phi(-8) = 6.2e-16, so for levels further than kTailSafe
// from 0 and 1 both ends hold without being evaluated
constexpr double kBracketSigmas = 8.0;
constexpr double kTailSafe = 1e-15;
// bound of the root search.  Log-Newton needs 6 - 10 evaluations; pure bisection of a step CDF ~60; the bound only
// guarantees that no data can keep a workgroup spinning
constexpr int kSummaryMaxIter = 128;
constexpr double kFarZ = 64.0;   // stands for (q - mu) / 0: erfc(kFarZ / sqrt 2) == 0 and erfc(-kFarZ / sqrt 2) == 2 exactly

// the indices of the draws with status == 0, in order, and their number: ONE workgroup, so the order is the draws' own.
// A failed draw thereby leaves every sum exactly as if the call had not contained it.
// SETS (ccgp_predict_summary_sets): one workgroup per training set (blockIdx.x); the rows of set c are the nb[c] consecutive
// rows from off[c] of tables whose rows are grouped by set, its indices (relative to off[c]) go to idx + off[c] and its
// number to count[c].  A template parameter, not a branch: the single-set instance compiles from unchanged code.
struct SetRows {
  const int *off, *nb;   // per set: first row and number of rows
};
template <bool SETS>
__global__ __launch_bounds__(kThreads) void summary_valid_kernel(const int* status, int S, int* idx, int* count, SetRows sr) {
  if constexpr (SETS) {
    const int c = blockIdx.x, o = sr.off[c];
    status += o; idx += o; count += c;
    S = sr.nb[c];
  }
  __shared__ int wave_n[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int s0 = 0; s0 < S; s0 += kThreads) {
    const int s = s0 + tid;
    const bool ok = s < S && status[s] == 0;
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_n[w];
    if (ok) idx[off + __popcll(mask & ((1ull << lane) - 1ull))] = s;
    for (int w = 0; w < kWaves; ++w) base += wave_n[w];
    __syncthreads();
  }
  if (tid == 0) *count = base;
}

struct SummaryArgs {
  const double* mean;   // S x m column-major: a site's S values are contiguous
  const double* var;
  const int* idx;       // the valid draws (summary_valid_kernel)
  const int* count;
  const double* y_at;   // m, or nullptr
  double* out;          // m x (4 + n_probs) column-major
  int S, m, n_probs;
  double probs[CCGP_SUMMARY_MAX_PROBS];
};
// the sets form: a grid of (site, set).  mean / var are B x m with the rows grouped by set (S is their leading dimension B),
// idx / count as summary_valid_kernel<true> leaves them, y_at C blocks of m (or nullptr), out C blocks of m x (4 + n_probs).
// want_staged: this launch serves the sets whose rows fit the staged route (nb <= kSummaryLdsDraws) or those that do not --
// a set takes the route the single-set call takes for its rows; a workgroup of another set's kind leaves at once.
struct SummarySetsArgs : SummaryArgs {
  SetRows sr;
};

struct SumOp { __device__ static double f(double a, double b) { return a + b; } };
struct MinOp { __device__ static double f(double a, double b) { return fmin(a, b); } };
struct MaxOp { __device__ static double f(double a, double b) { return fmax(a, b); } };

// block_sum (blocked.hip) for N values at once: one pair of barriers for all of them; every thread gets the totals
template <class Op, int N>
__device__ inline void block_reduce(double (&v)[N], double* red, int tid) {
#pragma unroll
  for (int i = 0; i < N; ++i)
    for (int off = 32; off > 0; off >>= 1) v[i] = Op::f(v[i], __shfl_down(v[i], off, 64));
  __syncthreads();
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[(tid >> 6) * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = Op::f(Op::f(Op::f(red[i], red[N + i]), red[2 * N + i]), red[3 * N + i]);
}

// one site's draws: staged as (mu, 1 / sigma) in LDS, or streamed from the site's column of the tables
template <bool STAGED>
struct Draws {
  const double *mcol, *vcol;
  const int* idx;
  const double *smu, *sis;
  __device__ static double inv_sigma(double v) { return v > 0.0 ? 1.0 / sqrt(v) : INFINITY; }
  __device__ void get(int k, double& mu, double& is) const {
    if (STAGED) {
      mu = smu[k];
      is = sis[k];
    } else {
      const int s = idx[k];
      mu = mcol[s];
      is = inv_sigma(vcol[s]);
    }
  }
};

// tail[j] = 1/S' sum_s 1/2 erfc(sgn[j] z_sj / sqrt 2) (sgn -1: F, +1: 1 - F) and dens[j] = the mixture density, at q[j]
template <int N, bool STAGED>
__device__ inline void mix_eval(const Draws<STAGED>& dr, int Sv, const double (&q)[N], const double (&sgn)[N],
                                double (&tail)[N], double (&dens)[N], double* red, int tid) {
  double acc[2 * N];
#pragma unroll
  for (int j = 0; j < 2 * N; ++j) acc[j] = 0.0;
  for (int k = tid; k < Sv; k += kThreads) {
    double mu, is;
    dr.get(k, mu, is);
    const bool point = is == INFINITY;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double z = point ? (q[j] >= mu ? kFarZ : -kFarZ) : (q[j] - mu) * is;
      acc[j] += 0.5 * erfc(sgn[j] * z * kInvSqrt2);
      acc[N + j] += point ? 0.0 : is * exp(-0.5 * z * z);
    }
  }
  block_reduce<SumOp>(acc, red, tid);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    tail[j] = acc[j] / Sv;
    dens[j] = acc[N + j] * kInvSqrt2Pi / Sv;
  }
}

// Root search of one level.  h(x) = F(x) - p (or (1 - p) - (1 - F(x)) on the upper tail) is non-decreasing; lo and hi
// hold h(lo) < 0 <= h(hi) once verified, and the answer is hi.
struct Root {
  double lo, hi, x, tgt, sgn, step, wref, floor_;
  double flo, fhi;                 // the tails evaluated at lo and hi (NaN where the end holds by the Phi(-8) argument)
  double bx, btail, bdens, berr;   // the evaluated point whose tail is closest to the target: Newton starts there
  int lo_ok, hi_ok, which, since, done, babove;   // which: what x is -- 0 an interior point, 1 the lower end, 2 the upper end
};

__device__ inline double ulpish(double a) { return fabs(a) * 0x1p-53; }   // in [ulp / 2, ulp)

__device__ inline void root_next(Root& r) {
  if (!r.lo_ok) { r.x = r.lo; r.which = 1; return; }
  if (!r.hi_ok) { r.x = r.hi; r.which = 2; return; }
  r.which = 0;
  const double width = r.hi - r.lo;
  const double tol = 2.0 * ulpish(fmax(fabs(r.lo), fabs(r.hi))) + r.floor_;
  // done: the bracket is under four ulp wide, or the tail no longer changes across it beyond its own rounding (a root
  // much closer to zero than sigma: the bracket cannot reach ulp(q), and F says nothing below eps F)
  if (!(width > 2.0 * tol) || fabs(r.fhi - r.flo) <= 4.0 * DBL_EPSILON * r.tgt) { r.done = 1; return; }
  double xn = NAN;
  if (r.berr < INFINITY) {
    // Newton on log(tail): the tails of a normal mixture are close to exp(-quadratic), where a step on the tail itself
    // crawls from the steep side and overshoots by orders of magnitude from the flat side
    double d = r.sgn * r.btail * log(r.btail / r.tgt) / r.bdens;
    // converged from one side: step across the root, by what the bracket's tolerance and the tail's rounding resolve,
    // to close the bracket
    const double dmin = tol + 2.0 * DBL_EPSILON * r.btail / r.bdens;
    if (fabs(d) < dmin) d = r.babove ? -dmin : dmin;
    xn = r.bx + d;
  }
  bool bisect = !(xn > r.lo && xn < r.hi);
  if (++r.since >= 4) {   // Newton steps that do not halve the bracket in four evaluations yield to bisection
    if (width > 0.5 * r.wref) bisect = true;
    r.wref = width;
    r.since = 0;
  }
  if (bisect) xn = r.lo + 0.5 * width;
  if (!(xn > r.lo && xn < r.hi)) { r.done = 1; return; }
  r.x = xn;
}

__device__ inline void root_update(Root& r, double tail, double dens) {
  if (r.done) return;
  // tail is F(x) on the lower tail (sgn -1) and 1 - F(x) on the upper: F(x) >= p  <=>  sgn (tgt - tail) >= 0
  const bool above = r.sgn * (r.tgt - tail) >= 0.0;
  if (r.which == 1) {
    if (!above) { r.lo_ok = 1; r.flo = tail; }
    else { r.hi = r.x; r.fhi = tail; r.hi_ok = 1; r.lo = r.x - r.step; r.step *= 4.0; }
  } else if (r.which == 2) {
    if (above) { r.hi_ok = 1; r.fhi = tail; }
    else { r.lo = r.x; r.flo = tail; r.lo_ok = 1; r.hi = r.x + r.step; r.step *= 4.0; }
  } else if (above) {
    r.hi = r.x; r.fhi = tail;
  } else {
    r.lo = r.x; r.flo = tail;
  }
  const double err = fabs(log(tail / r.tgt));
  if (err < r.berr) { r.bx = r.x; r.btail = tail; r.bdens = dens; r.berr = err; r.babove = above; }
  root_next(r);
}

template <int NL, bool STAGED, bool SETS = false>
__global__ __launch_bounds__(kThreads) void predict_summary_kernel(std::conditional_t<SETS, SummarySetsArgs, SummaryArgs> g) {
  __shared__ double smu[STAGED ? kSummaryLdsDraws : 1];
  __shared__ double sis[STAGED ? kSummaryLdsDraws : 1];
  __shared__ double red[kWaves * 2 * (NL > 2 ? NL : 2)];
  if constexpr (SETS) {
    const int c = blockIdx.y, nb = g.sr.nb[c], o = g.sr.off[c];
    if (nb == 0 || (nb <= kSummaryLdsDraws) != STAGED) return;   // uniform over the workgroup, before any barrier
    g.mean += o; g.var += o; g.idx += o; g.count += c;
    if (g.y_at) g.y_at += (size_t)c * g.m;
    g.out += (size_t)c * g.m * (4 + g.n_probs);
  }
  const int t = blockIdx.x, tid = threadIdx.x;
  const int Sv = *g.count, ncol = 4 + g.n_probs;
  if (Sv == 0) {
    for (int c = tid; c < ncol; c += kThreads) g.out[t + (size_t)c * g.m] = NAN;
    return;
  }
  Draws<STAGED> dr{g.mean + (size_t)t * g.S, g.var + (size_t)t * g.S, g.idx, smu, sis};

  // pass 1: the sums of mu and sigma^2, the first bracket; the staged route fills LDS on the way
  double sums[2] = {0.0, 0.0}, mins[2] = {INFINITY, INFINITY}, maxs[1] = {-INFINITY};
  for (int k = tid; k < Sv; k += kThreads) {
    const int s = g.idx[k];
    const double mu = dr.mcol[s], v = fmax(dr.vcol[s], 0.0), sd = sqrt(v);
    if (STAGED) {
      smu[k] = mu;
      sis[k] = Draws<STAGED>::inv_sigma(dr.vcol[s]);
    }
    sums[0] += mu;
    sums[1] += v;
    mins[0] = fmin(mins[0], mu - kBracketSigmas * sd);
    mins[1] = fmin(mins[1], mu);
    maxs[0] = fmax(maxs[0], mu + kBracketSigmas * sd);
  }
  block_reduce<SumOp>(sums, red, tid);
  block_reduce<MinOp>(mins, red, tid);
  block_reduce<MaxOp>(maxs, red, tid);   // its barriers also publish smu / sis
  const double y_hat = sums[0] / Sv;

  // pass 2: the spread of the means about y_hat
  double dev2[1] = {0.0};
  for (int k = tid; k < Sv; k += kThreads) {
    double mu, is;
    dr.get(k, mu, is);
    const double e = mu - y_hat;
    dev2[0] += e * e;
  }
  block_reduce<SumOp>(dev2, red, tid);
  const double pred_var = sums[1] / Sv + dev2[0] / Sv;

  // quant = 1 - F(y_hat), cdf_at = F(y_at)
  double q2[2] = {y_hat, g.y_at ? g.y_at[t] : y_hat}, s2[2] = {1.0, -1.0}, t2[2], d2[2];
  mix_eval<2, STAGED>(dr, Sv, q2, s2, t2, d2, red, tid);
  if (tid == 0) {
    g.out[t] = y_hat;
    g.out[t + (size_t)g.m] = pred_var;
    g.out[t + (size_t)2 * g.m] = t2[0];
    g.out[t + (size_t)3 * g.m] = g.y_at ? t2[1] : NAN;
  }
  if (g.n_probs == 0) return;

  // the quantiles: all levels iterate together, one pass over the draws per iteration
  const double lo0 = mins[0], hi0 = maxs[0], span = hi0 - lo0;
  Root r[NL];
  double q[NL], sg[NL], tl[NL], dn[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const double p = g.probs[j < g.n_probs ? j : 0];   // a level past n_probs repeats level 0 and is not written
    const bool upper = p > 0.5;
    Root& a = r[j];
    a.lo = lo0; a.hi = hi0; a.flo = a.fhi = NAN;
    a.tgt = upper ? 1.0 - p : p;
    a.sgn = upper ? 1.0 : -1.0;
    a.step = fmax(fmax(span, fmax(fabs(lo0), fabs(hi0)) * 0x1p-30), 1e-300);
    a.floor_ = span * 0x1p-75;
    a.wref = span; a.since = 0; a.done = 0; a.which = 0; a.x = lo0;
    // F(lo0) <= Phi(-8) unless a zero-sigma draw sits at lo0 itself; 1 - F(hi0) <= Phi(-8) always
    a.lo_ok = lo0 < mins[1] && (upper || p > kTailSafe);
    a.hi_ok = !upper || a.tgt > kTailSafe;
    a.bx = a.btail = a.bdens = 0.0; a.berr = INFINITY; a.babove = 0;
    root_next(a);
  }
  for (int it = 0; it < kSummaryMaxIter; ++it) {
    int all_done = 1;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      all_done &= r[j].done;
      q[j] = r[j].x;
      sg[j] = r[j].sgn;
    }
    if (all_done) break;
    mix_eval<NL, STAGED>(dr, Sv, q, sg, tl, dn, red, tid);
#pragma unroll
    for (int j = 0; j < NL; ++j) root_update(r[j], tl[j], dn[j]);
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < NL; ++j)
      if (j < g.n_probs) g.out[t + (size_t)(4 + j) * g.m] = r[j].hi;
  }
}

template <int NL>
void launch_nl(hipStream_t s, const SummaryArgs& g, bool staged) {
  if (staged) hipLaunchKernelGGL((predict_summary_kernel<NL, true>), dim3(g.m), dim3(kThreads), 0, s, g);
  else hipLaunchKernelGGL((predict_summary_kernel<NL, false>), dim3(g.m), dim3(kThreads), 0, s, g);
}

}  // namespace

void launch_predict_summary(hipStream_t s, const double* d_mean, const double* d_var, const int* d_status, int S, int m,
                            const double* probs, int n_probs, const double* d_y_at, int* d_idx, int* d_count,
                            double* d_out) {
  hipLaunchKernelGGL(summary_valid_kernel<false>, dim3(1), dim3(kThreads), 0, s, d_status, S, d_idx, d_count, SetRows{});
  SummaryArgs g{};
  g.mean = d_mean; g.var = d_var; g.idx = d_idx; g.count = d_count; g.y_at = d_y_at; g.out = d_out;
  g.S = S; g.m = m; g.n_probs = n_probs;
  for (int j = 0; j < n_probs; ++j) g.probs[j] = probs[j];
  const bool staged = S <= kSummaryLdsDraws;
  // the level loop is unrolled for 1, 2, 4 or 8 levels: the erfc chains of a draw's levels interleave
  if (n_probs <= 1) launch_nl<1>(s, g, staged);
  else if (n_probs <= 2) launch_nl<2>(s, g, staged);
  else if (n_probs <= 4) launch_nl<4>(s, g, staged);
  else launch_nl<8>(s, g, staged);
}

namespace {
template <int NL>
void launch_nl_sets(hipStream_t s, const SummarySetsArgs& g, int C, bool staged) {
  if (staged) hipLaunchKernelGGL((predict_summary_kernel<NL, true, true>), dim3(g.m, C), dim3(kThreads), 0, s, g);
  else hipLaunchKernelGGL((predict_summary_kernel<NL, false, true>), dim3(g.m, C), dim3(kThreads), 0, s, g);
}
}  // namespace

// the sets form: C sets in one grid.  d_mean / d_var: B x m column-major, rows grouped by set; d_off / d_nb (C ints each):
// a set's first row and its rows; d_idx (B ints) and d_count (C ints) are scratch; d_y_at: C blocks of m or nullptr; d_out:
// C blocks of m x (4 + n_probs), the block of a set without rows is not written.  any_staged / any_streamed: whether some set
// has at most / more than kSummaryLdsDraws rows (the host knows): one launch per kind that occurs.
void launch_predict_summary_sets(hipStream_t s, const double* d_mean, const double* d_var, const int* d_status, int B, int m,
                                 int C, const int* d_off, const int* d_nb, bool any_staged, bool any_streamed,
                                 const double* probs, int n_probs, const double* d_y_at, int* d_idx, int* d_count,
                                 double* d_out) {
  const SetRows sr{d_off, d_nb};
  hipLaunchKernelGGL(summary_valid_kernel<true>, dim3(C), dim3(kThreads), 0, s, d_status, 0, d_idx, d_count, sr);
  SummarySetsArgs g{};
  g.mean = d_mean; g.var = d_var; g.idx = d_idx; g.count = d_count; g.y_at = d_y_at; g.out = d_out;
  g.S = B; g.m = m; g.n_probs = n_probs; g.sr = sr;
  for (int j = 0; j < n_probs; ++j) g.probs[j] = probs[j];
  for (int kind = 0; kind < 2; ++kind) {
    const bool staged = kind == 0;
    if (!(staged ? any_staged : any_streamed)) continue;
    if (n_probs <= 1) launch_nl_sets<1>(s, g, C, staged);
    else if (n_probs <= 2) launch_nl_sets<2>(s, g, C, staged);
    else if (n_probs <= 4) launch_nl_sets<4>(s, g, C, staged);
    else launch_nl_sets<8>(s, g, C, staged);
  }
}

}  // namespace ccgp
