// The Nelder-Mead search of fit.laplace_sets (fit.py) for ONE set, restated so that the host and the device compute THE SAME
// BITS: the Laplace search that runs inside small_reg_kernel<.., CHAIN, .., NM> steps its simplex in the kernel, and its host
// twin (ccgp_nm_begin, ccgp_nm_feed) must reproduce every trial point, every decision and the stop.  Operation for operation
// what laplace_sets does, with numpy's order of operations:
//   the initial simplex of the search laplace runs (vertex k + 1: x[k] = (1.0 + 0.05) x[k], or 0.00025 where x[k] is zero);
//   xbar = the column sums of the p best vertices, left to right from vertex 0 (numpy's axis-0 reduction of a p x p block adds
//   row after row; tests/test_nm_logic_host.py holds numpy to it), then / p;
//   the trial points 2 xbar - w, 3 xbar - 2 w, 1.5 xbar - 0.5 w, 0.5 xbar + 0.5 w (every product rounded, then the sum);
//   the shrink x0 + 0.5 (x - x0); a stable sort of the vertices by value; a non-finite value stored as 1e300;
//   the stop tests after the initial simplex is sorted and after every iteration's sort: converged where every
//   |x_v - x_0| <= xatol and every |f_0 - f_v| <= fatol, else maxiter where iterations >= maxiter or charged >= maxiter.
// laplace_sets sends the four trial points of an iteration out at once, but its decisions read only the values a
// one-at-a-time search asks for: the reflection first, then the expansion (f_r < f_0), nothing (f_r < f_{p-1}), the outside
// contraction (f_r < f_p) or the inside contraction, and the p shrink points only where the contraction fails.  nm_feed
// advances by ONE evaluation and asks for exactly those; `charged` keeps laplace_sets' own count (p + 1, + 4 per iteration,
// + p per shrink), which its maxiter rule reads, `fed` the evaluations actually made.
// Only +, -, *, /, comparisons and selects are used, with contraction off inside every function (the pragma is
// function-local: a file-scope one would change the kernels of whatever includes this).  fp64 division is exactly rounded on
// the host and, under this project's flags, on the device (see chain_terms.h).
//   State.  One search is a flat array of nm_state_doubles(q) = q^2 + 5 q + 18 doubles:
//     [0] q  [1] code  [2] phase  [3] vertex (of the initial-simplex and shrink phases)  [4] iterations  [5] charged  [6] fed
//     [7] maxiter  [8] xatol  [9] fatol  [10] expansions taken  [11] expansions refused  [12] plain reflections
//     [13] outside contractions taken  [14] inside contractions taken  [15] shrinks
//     then simplex ((q + 1) x q, vertex-major, sorted best first) | negated values (q + 1) | xbar (q) | reflected point (q) |
//     its value (1) | trial (q)
//   code: kNmRunning, kNmConverged or kNmMaxiter.  While the code is kNmRunning, `trial` is the next point to evaluate.
// Plain C++ apart from the __host__ __device__ marks.
#pragma once

#include "chain_terms.h"

namespace ccgp {

enum { kNmRunning = 0, kNmConverged = 1, kNmMaxiter = 2 };
enum { kNmPhaseInit = 0, kNmPhaseReflect, kNmPhaseExpand, kNmPhaseOutside, kNmPhaseInside, kNmPhaseShrink };
enum { kNmQ = 0, kNmCode, kNmPhase, kNmVertex, kNmIterations, kNmCharged, kNmFed, kNmMaxiterOpt, kNmXatol, kNmFatol,
       kNmExpTaken, kNmExpRefused, kNmReflected, kNmOutside, kNmInside, kNmShrunk, kNmHeader = 16 };
constexpr int kNmMaxQ = 8;

CCGP_CHAIN_HD constexpr int nm_state_doubles(int q) { return kNmHeader + (q + 1) * q + (q + 1) + 3 * q + 1; }
CCGP_CHAIN_HD inline double* nm_sim(double* s, int q, int v) { return s + kNmHeader + v * q; }
CCGP_CHAIN_HD inline double* nm_fsim(double* s, int q) { return s + kNmHeader + (q + 1) * q; }
CCGP_CHAIN_HD inline double* nm_xbar(double* s, int q) { return nm_fsim(s, q) + (q + 1); }
CCGP_CHAIN_HD inline double* nm_xr(double* s, int q) { return nm_xbar(s, q) + q; }
CCGP_CHAIN_HD inline double* nm_fr(double* s, int q) { return nm_xr(s, q) + q; }
CCGP_CHAIN_HD inline double* nm_trial(double* s, int q) { return nm_fr(s, q) + 1; }

CCGP_CHAIN_HD inline bool nm_finite(double v) { return (chain_bits(v) & 0x7ff0000000000000ULL) != 0x7ff0000000000000ULL; }
// |v| <= tol as np.abs(v) <= tol decides it (a NaN says no)
CCGP_CHAIN_HD inline bool nm_within(double v, double tol) {
  const double m = v < 0.0 ? -v : v;
  return m <= tol;
}

// np.argsort(fsim, kind="stable") applied to both arrays: adjacent exchanges on a strict >, so equal values keep their order
CCGP_CHAIN_HD inline void nm_sort(double* st, int q) {
  double* f = nm_fsim(st, q);
  for (int i = 1; i <= q; ++i)
    for (int j = i - 1; j >= 0 && f[j] > f[j + 1]; --j) {
      const double t = f[j]; f[j] = f[j + 1]; f[j + 1] = t;
      double *a = nm_sim(st, q, j), *b = nm_sim(st, q, j + 1);
      for (int k = 0; k < q; ++k) { const double u = a[k]; a[k] = b[k]; b[k] = u; }
    }
}

// the stop tests on the sorted simplex, then -- where the search goes on -- xbar and the reflected point as the next trial
CCGP_CHAIN_HD inline void nm_next_iteration(double* st, int q) {
#pragma clang fp contract(off)
  const double *x0 = nm_sim(st, q, 0), *f = nm_fsim(st, q);
  bool conv = true;
  for (int v = 1; v <= q; ++v) {
    const double* xv = nm_sim(st, q, v);
    for (int k = 0; k < q; ++k) conv = nm_within(xv[k] - x0[k], st[kNmXatol]) && conv;
    conv = nm_within(f[0] - f[v], st[kNmFatol]) && conv;
  }
  if (conv) { st[kNmCode] = kNmConverged; return; }
  if (st[kNmIterations] >= st[kNmMaxiterOpt] || st[kNmCharged] >= st[kNmMaxiterOpt]) { st[kNmCode] = kNmMaxiter; return; }
  double *xbar = nm_xbar(st, q), *xr = nm_xr(st, q), *trial = nm_trial(st, q);
  const double* w = nm_sim(st, q, q);
  const double p = (double)q;
  for (int k = 0; k < q; ++k) {
    double s = x0[k];
    for (int v = 1; v < q; ++v) s = s + nm_sim(st, q, v)[k];
    xbar[k] = s / p;
    const double t = 2.0 * xbar[k];
    xr[k] = t - w[k];
    trial[k] = xr[k];
  }
  st[kNmPhase] = kNmPhaseReflect;
}

// the worst vertex becomes x with value fx; the iteration ends
CCGP_CHAIN_HD inline void nm_replace_worst(double* st, int q, const double* x, double fx) {
  double* w = nm_sim(st, q, q);
  for (int k = 0; k < q; ++k) w[k] = x[k];
  nm_fsim(st, q)[q] = fx;
  nm_sort(st, q);
  nm_next_iteration(st, q);
}

// the contraction failed: every vertex but the best moves half way to it, and their values are asked for one by one
CCGP_CHAIN_HD inline void nm_begin_shrink(double* st, int q) {
#pragma clang fp contract(off)
  const double* x0 = nm_sim(st, q, 0);
  for (int v = 1; v <= q; ++v) {
    double* xv = nm_sim(st, q, v);
    for (int k = 0; k < q; ++k) {
      const double h = 0.5 * (xv[k] - x0[k]);
      xv[k] = x0[k] + h;
    }
  }
  st[kNmShrunk] = st[kNmShrunk] + 1.0;
  st[kNmPhase] = kNmPhaseShrink;
  st[kNmVertex] = 1.0;
  double* trial = nm_trial(st, q);
  for (int k = 0; k < q; ++k) trial[k] = nm_sim(st, q, 1)[k];
}

CCGP_CHAIN_HD inline void nm_begin(double* st, int q, const double* x0, double xatol, double fatol, int maxiter) {
#pragma clang fp contract(off)
  for (int e = 0; e < nm_state_doubles(q); ++e) st[e] = 0.0;
  st[kNmQ] = q;
  st[kNmCode] = kNmRunning;
  st[kNmPhase] = kNmPhaseInit;
  st[kNmCharged] = q + 1;
  st[kNmMaxiterOpt] = maxiter;
  st[kNmXatol] = xatol;
  st[kNmFatol] = fatol;
  const double one = 1.0, step = 0.05;
  const double grow = one + step;
  for (int v = 0; v <= q; ++v) {
    double* xv = nm_sim(st, q, v);
    for (int k = 0; k < q; ++k) xv[k] = x0[k];
    if (v > 0) xv[v - 1] = x0[v - 1] != 0.0 ? grow * x0[v - 1] : 0.00025;
  }
  for (int k = 0; k < q; ++k) nm_trial(st, q)[k] = x0[k];
}

// the log-posterior val at `trial`: one step of the search
CCGP_CHAIN_HD inline void nm_feed(double* st, double val) {
#pragma clang fp contract(off)
  if (st[kNmCode] != (double)kNmRunning) return;
  const int q = (int)st[kNmQ];
  const double fx = nm_finite(val) ? -val : 1e300;
  double *f = nm_fsim(st, q), *trial = nm_trial(st, q);
  const double *xbar = nm_xbar(st, q), *w = nm_sim(st, q, q);
  st[kNmFed] = st[kNmFed] + 1.0;
  const int phase = (int)st[kNmPhase];
  if (phase == kNmPhaseInit || phase == kNmPhaseShrink) {
    const int v = (int)st[kNmVertex];
    f[v] = fx;
    if (v < q) {
      st[kNmVertex] = v + 1;
      for (int k = 0; k < q; ++k) trial[k] = nm_sim(st, q, v + 1)[k];
      return;
    }
    if (phase == kNmPhaseShrink) st[kNmCharged] = st[kNmCharged] + (double)q;
    nm_sort(st, q);
    nm_next_iteration(st, q);
    return;
  }
  if (phase == kNmPhaseReflect) {
    *nm_fr(st, q) = fx;
    st[kNmIterations] = st[kNmIterations] + 1.0;
    st[kNmCharged] = st[kNmCharged] + 4.0;
    if (fx < f[0]) {
      for (int k = 0; k < q; ++k) {
        const double a = 3.0 * xbar[k], b = 2.0 * w[k];
        trial[k] = a - b;
      }
      st[kNmPhase] = kNmPhaseExpand;
    } else if (fx < f[q - 1]) {
      st[kNmReflected] = st[kNmReflected] + 1.0;
      nm_replace_worst(st, q, nm_xr(st, q), fx);
    } else if (fx < f[q]) {
      for (int k = 0; k < q; ++k) {
        const double a = 1.5 * xbar[k], b = 0.5 * w[k];
        trial[k] = a - b;
      }
      st[kNmPhase] = kNmPhaseOutside;
    } else {
      for (int k = 0; k < q; ++k) {
        const double a = 0.5 * xbar[k], b = 0.5 * w[k];
        trial[k] = a + b;
      }
      st[kNmPhase] = kNmPhaseInside;
    }
    return;
  }
  const double fr = *nm_fr(st, q);
  if (phase == kNmPhaseExpand) {
    if (fx < fr) {
      st[kNmExpTaken] = st[kNmExpTaken] + 1.0;
      nm_replace_worst(st, q, trial, fx);
    } else {
      st[kNmExpRefused] = st[kNmExpRefused] + 1.0;
      nm_replace_worst(st, q, nm_xr(st, q), fr);
    }
  } else if (phase == kNmPhaseOutside) {
    if (fx <= fr) {
      st[kNmOutside] = st[kNmOutside] + 1.0;
      nm_replace_worst(st, q, trial, fx);
    } else {
      nm_begin_shrink(st, q);
    }
  } else {
    if (fx < f[q]) {
      st[kNmInside] = st[kNmInside] + 1.0;
      nm_replace_worst(st, q, trial, fx);
    } else {
      nm_begin_shrink(st, q);
    }
  }
}

}  // namespace ccgp
