// The box-constrained limited-memory quasi-Newton iteration of design._Start (design.py) restated so that the host and the
// device compute THE SAME BITS: the ordinary-kriging fit that runs inside small_reg_kernel<.., FIT> steps its start in the
// kernel, and its host twin (ccgp_fit_begin, ccgp_fit_feed) must reproduce every trial point, every accepted iterate and every
// stopping decision.  Operation for operation what _Start does: the active set, the two-loop recursion (memory 5) with its sy
// filter, the steepest-descent fallback with its memory reset, t = min(1, 1 / |p|) on a steepest step, the projected Armijo
// search (constant 1e-4), the safeguarded quadratic interpolation min(max(tq, 0.1 t), 0.5 t), halving after an infeasible
// trial, max_backtracks with one retry from an emptied memory, the acceptance test s.y > eps y.y and the three stopping rules.
// Only +, -, *, /, sqrt, comparisons and selects are used, with contraction off inside every function (the pragma is
// function-local: a file-scope one would change the kernels of whatever includes this).  fp64 division and square root are
// exactly rounded on the host and, under this project's flags, on the device: the Makefile compiles without -ffast-math,
// without -fno-honor-* and without -freciprocal-math; a build that relaxes either would break the host / device agreement,
// and tests/test_gpu_device_fits.py would show it.  min / max follow Python's (min(a, b) is b only where b < a), clip follows
// numpy's minimum(maximum(v, lo), hi) for the finite boxes a fit has.
//   Sums.  design._dot is np.add.reduce(a * b): every product rounded, then numpy's pairwise order, which for the lengths a
//   start has (d <= 64) is: below 8 terms, from +0.0 left to right; from 8 terms on, eight accumulators seeded with terms
//   0 .. 7, every further full block of eight added lane-wise, the accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
//   the remaining terms added left to right.  fit_sum is that order (tests/test_fit_logic_host.py holds numpy to it).
//   State.  One start is a flat array of fit_state_doubles(d) = 16 + 16 d doubles:
//     [0] d  [1] code  [2] f  [3] t  [4] backtracks  [5] iterations  [6] first (1.0 until the start itself is evaluated)
//     [7] pairs kept (0 .. 5)  [8] maxit  [9] factr  [10] pgtol  [11] max_backtracks  [12] evaluations fed  [13 .. 15] 0
//     then x | g | p | trial | lo | hi (d each) | s_0 .. s_4 | y_0 .. y_4 (d each, oldest pair first)
//   code: kFitRunning, or why the start stopped.  After fit_begin or fit_feed, `trial` is the next point to evaluate or the
//   code says stop.  Plain C++ apart from the __host__ __device__ marks.
// The objective of the ordinary-kriging fit, in the same portable arithmetic (fit._kriging_fit_sets.evaluate with numpy's exp
// replaced by chain_exp): theta_k = chain_exp(x_k), parameter row (1, theta), f = -ll, g_k = -(g_theta_k theta_k).
#pragma once

#include "chain_terms.h"

namespace ccgp {

enum { kFitRunning = 0, kFitConvReduction = 1, kFitConvProjGrad = 2, kFitMaxit = 3, kFitLineSearch = 4, kFitNotEvaluable = 5 };
enum { kFitD = 0, kFitCode, kFitF, kFitT, kFitBacktracks, kFitIterations, kFitFirst, kFitPairs, kFitMaxitOpt, kFitFactr,
       kFitPgtol, kFitMaxBt, kFitEvals, kFitHeader = 16 };
constexpr int kFitMemory = 5;

struct FitOpts {
  int maxit;
  double factr, pgtol;
  int max_backtracks;
};

CCGP_CHAIN_HD constexpr int fit_state_doubles(int d) { return kFitHeader + (6 + 2 * kFitMemory) * d; }
CCGP_CHAIN_HD inline double* fit_x(double* s, int d) { (void)d; return s + kFitHeader; }
CCGP_CHAIN_HD inline double* fit_g(double* s, int d) { return s + kFitHeader + d; }
CCGP_CHAIN_HD inline double* fit_p(double* s, int d) { return s + kFitHeader + 2 * d; }
CCGP_CHAIN_HD inline double* fit_trial(double* s, int d) { return s + kFitHeader + 3 * d; }
CCGP_CHAIN_HD inline double* fit_lo(double* s, int d) { return s + kFitHeader + 4 * d; }
CCGP_CHAIN_HD inline double* fit_hi(double* s, int d) { return s + kFitHeader + 5 * d; }
CCGP_CHAIN_HD inline double* fit_s(double* s, int d, int i) { return s + kFitHeader + (6 + i) * d; }
CCGP_CHAIN_HD inline double* fit_y(double* s, int d, int i) { return s + kFitHeader + (6 + kFitMemory + i) * d; }

CCGP_CHAIN_HD inline double fit_pymin(double a, double b) { return b < a ? b : a; }
CCGP_CHAIN_HD inline double fit_pymax(double a, double b) { return b > a ? b : a; }
CCGP_CHAIN_HD inline double fit_abs(double v) { return chain_from_bits(chain_bits(v) & 0x7fffffffffffffffULL); }
CCGP_CHAIN_HD inline bool fit_finite(double v) { return (chain_bits(v) & 0x7ff0000000000000ULL) != 0x7ff0000000000000ULL; }
CCGP_CHAIN_HD inline double fit_clip(double v, double lo, double hi) {
  const double m = v < lo ? lo : v;   // a NaN stays a NaN, as in numpy
  return m > hi ? hi : m;
}

// np.add.reduce over term(0) .. term(n - 1), n <= 128
template <class F>
CCGP_CHAIN_HD inline double fit_sum(int n, F term) {
#pragma clang fp contract(off)
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res = res + term(i);
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = term(j);
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + term(i + j);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res = res + term(i);
  return res;
}
CCGP_CHAIN_HD inline double fit_dot(int n, const double* a, const double* b) {
#pragma clang fp contract(off)
  return fit_sum(n, [=](int i) {
#pragma clang fp contract(off)
    return a[i] * b[i];
  });
}

// _Start._free: a variable at a bound whose gradient points out of the box is frozen
CCGP_CHAIN_HD inline bool fit_free(const double* x, const double* g, const double* lo, const double* hi, int k) {
  const bool at_lo = x[k] <= lo[k] && g[k] > 0.0, at_hi = x[k] >= hi[k] && g[k] < 0.0;
  return !(at_lo || at_hi);
}
// _Start._pg_norm
CCGP_CHAIN_HD inline double fit_pg_norm(int d, const double* x, const double* g, const double* lo, const double* hi) {
#pragma clang fp contract(off)
  double m = 0.0;
  for (int k = 0; k < d; ++k) {
    const double v = fit_abs(fit_clip(x[k] - g[k], lo[k], hi[k]) - x[k]);
    if (k == 0 || v > m || v != v) m = v;   // np.max: a NaN wins (none can occur for finite x and g)
  }
  return m;
}

// _Start._begin_iteration with _direction: p and the first trial of the iteration, or the code of a Kuhn-Tucker point
CCGP_CHAIN_HD inline void fit_begin_iteration(double* st) {
#pragma clang fp contract(off)
  const int d = (int)st[kFitD];
  double *x = fit_x(st, d), *g = fit_g(st, d), *p = fit_p(st, d), *trial = fit_trial(st, d);
  const double *lo = fit_lo(st, d), *hi = fit_hi(st, d);
  const double eps = chain_from_bits(0x3cb0000000000000ULL);   // 2^-52
  int cnt = (int)st[kFitPairs];
  // q lives in p; masked operands are +0.0 as np.where(free, ., 0.0) gives them
  for (int k = 0; k < d; ++k) p[k] = fit_free(x, g, lo, hi, k) ? g[k] : 0.0;
  int kept[kFitMemory], nk = 0;
  double alpha[kFitMemory], rho[kFitMemory];
  for (int i = cnt - 1; i >= 0; --i) {   // newest first
    const double *s = fit_s(st, d, i), *y = fit_y(st, d, i);
    auto sf = [=](int k) { return fit_free(x, g, lo, hi, k) ? s[k] : 0.0; };
    auto yf = [=](int k) { return fit_free(x, g, lo, hi, k) ? y[k] : 0.0; };
    const double sy = fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return sf(k) * yf(k);
    });
    const double yy = fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return yf(k) * yf(k);
    });
    if (sy <= eps * yy || sy <= 0.0) continue;
    const double r = 1.0 / sy;
    const double* q = p;
    const double a = r * fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return sf(k) * q[k];
    });
    for (int k = 0; k < d; ++k) {
      const double ay = a * yf(k);
      p[k] = p[k] - ay;
    }
    kept[nk] = i; alpha[nk] = a; rho[nk] = r;
    ++nk;
  }
  if (nk) {
    const double* y = fit_y(st, d, kept[0]);
    auto yf = [=](int k) { return fit_free(x, g, lo, hi, k) ? y[k] : 0.0; };
    const double yy = fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return yf(k) * yf(k);
    });
    const double scale = (1.0 / rho[0]) / yy;
    for (int k = 0; k < d; ++k) p[k] = p[k] * scale;
  }
  for (int j = nk - 1; j >= 0; --j) {   // oldest first
    const double *s = fit_s(st, d, kept[j]), *y = fit_y(st, d, kept[j]);
    const double* q = p;
    const double b = rho[j] * fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return (fit_free(x, g, lo, hi, k) ? y[k] : 0.0) * q[k];
    });
    const double ab = alpha[j] - b;
    for (int k = 0; k < d; ++k) {
      const double as = ab * (fit_free(x, g, lo, hi, k) ? s[k] : 0.0);
      p[k] = p[k] + as;
    }
  }
  for (int k = 0; k < d; ++k) p[k] = -p[k];
  const double gd = fit_dot(d, g, p);
  bool steepest = false;
  if (!nk || !(gd < 0.0)) {
    cnt = 0;
    st[kFitPairs] = 0.0;
    for (int k = 0; k < d; ++k) p[k] = -(fit_free(x, g, lo, hi, k) ? g[k] : 0.0);
    steepest = true;
  }
  const double pn = __builtin_sqrt(fit_dot(d, p, p));
  if (pn == 0.0) {   // every variable frozen or a zero gradient: a Kuhn-Tucker point
    st[kFitCode] = kFitConvProjGrad;
    return;
  }
  const double t = steepest ? fit_pymin(1.0, 1.0 / pn) : 1.0;
  st[kFitT] = t;
  st[kFitBacktracks] = 0.0;
  for (int k = 0; k < d; ++k) {
    const double tp = t * p[k];
    trial[k] = fit_clip(x[k] + tp, lo[k], hi[k]);
  }
}

// _Start.__init__: the first call evaluates the (clipped) start itself
CCGP_CHAIN_HD inline void fit_begin(double* st, int d, const double* x0, const double* lo, const double* hi, const FitOpts& o) {
  for (int e = 0; e < fit_state_doubles(d); ++e) st[e] = 0.0;
  st[kFitD] = d;
  st[kFitCode] = kFitRunning;
  st[kFitF] = chain_from_bits(0x7ff0000000000000ULL);
  st[kFitFirst] = 1.0;
  st[kFitMaxitOpt] = o.maxit;
  st[kFitFactr] = o.factr;
  st[kFitPgtol] = o.pgtol;
  st[kFitMaxBt] = o.max_backtracks;
  for (int k = 0; k < d; ++k) {
    fit_lo(st, d)[k] = lo[k];
    fit_hi(st, d)[k] = hi[k];
    const double v = fit_clip(x0[k], lo[k], hi[k]);
    fit_x(st, d)[k] = v;
    fit_trial(st, d)[k] = v;
  }
}

// _Start.feed: the value f and gradient gnew at `trial`; ok = the evaluator did not report a failure
CCGP_CHAIN_HD inline void fit_feed(double* st, double f, const double* gnew, bool ok) {
#pragma clang fp contract(off)
  if (st[kFitCode] != (double)kFitRunning) return;
  const int d = (int)st[kFitD];
  double *x = fit_x(st, d), *g = fit_g(st, d), *p = fit_p(st, d), *trial = fit_trial(st, d);
  const double *lo = fit_lo(st, d), *hi = fit_hi(st, d);
  const double eps = chain_from_bits(0x3cb0000000000000ULL);
  st[kFitEvals] = st[kFitEvals] + 1.0;
  ok = ok && fit_finite(f);
  for (int k = 0; ok && k < d; ++k) ok = fit_finite(gnew[k]);
  if (st[kFitFirst] != 0.0) {
    st[kFitFirst] = 0.0;
    if (!ok) { st[kFitCode] = kFitNotEvaluable; return; }
    st[kFitF] = f;
    for (int k = 0; k < d; ++k) g[k] = gnew[k];
    if (fit_pg_norm(d, x, g, lo, hi) <= st[kFitPgtol]) { st[kFitCode] = kFitConvProjGrad; return; }
    fit_begin_iteration(st);
    return;
  }
  const double f0 = st[kFitF];
  const double slope = fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
    return g[k] * (trial[k] - x[k]);
  });
  if (ok && f <= f0 + 1e-4 * fit_pymin(slope, 0.0)) {
    // _accept
    const double sy = fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return (trial[k] - x[k]) * (gnew[k] - g[k]);
    });
    const double yy = fit_sum(d, [=](int k) {
#pragma clang fp contract(off)
      return (gnew[k] - g[k]) * (gnew[k] - g[k]);
    });
    if (sy > eps * yy) {
      int cnt = (int)st[kFitPairs];
      if (cnt == kFitMemory) {   // the oldest pair leaves
        for (int i = 0; i + 1 < kFitMemory; ++i)
          for (int k = 0; k < d; ++k) {
            fit_s(st, d, i)[k] = fit_s(st, d, i + 1)[k];
            fit_y(st, d, i)[k] = fit_y(st, d, i + 1)[k];
          }
        cnt = kFitMemory - 1;
      }
      for (int k = 0; k < d; ++k) {
        fit_s(st, d, cnt)[k] = trial[k] - x[k];
        fit_y(st, d, cnt)[k] = gnew[k] - g[k];
      }
      st[kFitPairs] = cnt + 1;
    }
    for (int k = 0; k < d; ++k) { x[k] = trial[k]; g[k] = gnew[k]; }
    st[kFitF] = f;
    st[kFitIterations] = st[kFitIterations] + 1.0;
    const double scale = fit_pymax(fit_pymax(fit_abs(f0), fit_abs(f)), 1.0);
    if ((f0 - f) <= st[kFitFactr] * eps * scale) { st[kFitCode] = kFitConvReduction; return; }
    if (fit_pg_norm(d, x, g, lo, hi) <= st[kFitPgtol]) { st[kFitCode] = kFitConvProjGrad; return; }
    if (st[kFitIterations] >= st[kFitMaxitOpt]) { st[kFitCode] = kFitMaxit; return; }
    fit_begin_iteration(st);
    return;
  }
  // backtrack: safeguarded quadratic interpolation on an infeasible-free trial, halving otherwise
  st[kFitBacktracks] = st[kFitBacktracks] + 1.0;
  bool moved = false;
  for (int k = 0; k < d; ++k) moved = moved || (trial[k] - x[k]) != 0.0;
  if (st[kFitBacktracks] > st[kFitMaxBt] || !moved) {
    if (st[kFitPairs] != 0.0) {   // the quasi-Newton model misled the search: forget it and try steepest descent once more
      st[kFitPairs] = 0.0;
      fit_begin_iteration(st);
      return;
    }
    st[kFitCode] = kFitLineSearch;
    return;
  }
  double t = st[kFitT];
  if (ok) {
    const double dphi = slope / t;
    const double denom = 2.0 * ((f - f0) - dphi * t);
    const double tq = denom > 0.0 ? ((-dphi * t) * t) / denom : 0.5 * t;
    t = fit_pymin(fit_pymax(tq, 0.1 * t), 0.5 * t);
  } else {
    t = 0.5 * t;
  }
  st[kFitT] = t;
  for (int k = 0; k < d; ++k) {
    const double tp = t * p[k];
    trial[k] = fit_clip(x[k] + tp, lo[k], hi[k]);
  }
}

// ---- the objective of the ordinary-kriging fit in the portable arithmetic ---------------------------------------------------
CCGP_CHAIN_HD inline double fit_theta(double x, const double* thi, const double* tlo) { return chain_exp(x, thi, tlo); }
// f = -ll; a NaN likelihood (a failed factorisation) is the one quiet NaN on both sides
CCGP_CHAIN_HD inline double fit_value(double ll) {
  return ll == ll ? -ll : chain_from_bits(0x7ff8000000000000ULL);
}
// g_k = -(d ll / d theta_k  theta_k)
CCGP_CHAIN_HD inline double fit_grad(double g_theta, double theta) {
#pragma clang fp contract(off)
  const double v = -(g_theta * theta);
  return v == v ? v : chain_from_bits(0x7ff8000000000000ULL);
}

// ---- the objective of the maximum-entropy design search (rsurface.Entropy_optim / Batch_Entropy_optim) ----------------------
// The iterate is the design itself, so nothing is transformed: f = -(ld - ld_offset) (ld_offset = log det R(D.old) of the
// batch form, 0 otherwise) and g_v = -(d ld / d x_v), each one exactly rounded operation and a sign; a failed elimination's
// NaN is the one quiet NaN on both sides
CCGP_CHAIN_HD inline double design_fit_value(double ld, double ld_offset) {
#pragma clang fp contract(off)
  const double v = -(ld - ld_offset);
  return v == v ? v : chain_from_bits(0x7ff8000000000000ULL);
}
CCGP_CHAIN_HD inline double design_fit_grad(double g_x) {
  const double v = -g_x;
  return v == v ? v : chain_from_bits(0x7ff8000000000000ULL);
}

}  // namespace ccgp
