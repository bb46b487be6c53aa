// The objective of the CGP refinement (cgp._fit_sets.evaluate with cgp.rows_from_ww, GV:102-133 behind optim's central
// differences) restated so that the host and the device compute THE SAME BITS: the step kernel of ccgp_cgp_fit_sets forms a
// start's next parameter rows and its gradient on the device, and its host twin (ccgp_cgp_fit_eval_sets with ccgp_fit_feed)
// must reproduce every row and every gradient entry.  Nothing transcendental lies between the stepper (fit_logic.h) and the
// evaluator (cgp_state_kernel): a row is the iterate plus one addition, a gradient entry one subtraction and one division,
// each exactly rounded on both sides under the flags fit_logic.h names, with contraction off inside every function.
//   A start's variables are w = (lambda, theta_1 .. theta_d, kappa, bw), P = d + 3, in the box [lo, hi]; the difference step
//   is `step`.  up_j = min(w_j + step, hi_j), dn_j = max(w_j - step, lo_j), following numpy's minimum / maximum (the first
//   operand where it is smaller / larger or a NaN, else the second).
//   The R = 1 + 2 P points of one evaluation: row 0 is the centre w, row 1 + 2 j has variable j at up_j, row 2 + 2 j at dn_j.
//   The device row of a point v is (v_0, v_1 .. v_d, v_k + v_{d+1} for k = 1 .. d, v_{d+2}): 2 d + 2 columns.
//   F = val where val is finite, else 1e6 (cgp.NONFINITE, GV:130-131); f = F_0; g_j = (F_{1+2j} - F_{2+2j}) / (up_j - dn_j);
//   ok = (status of row 0 == 0): failures of differenced rows only show through the 1e6.
// Plain C++ apart from the __host__ __device__ marks.
#pragma once

#include "fit_logic.h"

namespace ccgp {

CCGP_CHAIN_HD constexpr int cgp_fit_vars(int d) { return d + 3; }
CCGP_CHAIN_HD constexpr int cgp_fit_rows(int d) { return 1 + 2 * (d + 3); }
CCGP_CHAIN_HD constexpr int cgp_fit_cols(int d) { return 2 * d + 2; }

CCGP_CHAIN_HD inline double cgp_fit_up(double w, double step, double hi) {
#pragma clang fp contract(off)
  const double a = w + step;
  return (a < hi || a != a) ? a : hi;
}
CCGP_CHAIN_HD inline double cgp_fit_dn(double w, double step, double lo) {
#pragma clang fp contract(off)
  const double a = w - step;
  return (a > lo || a != a) ? a : lo;
}

// variable j of the point in row r of the evaluation around w
CCGP_CHAIN_HD inline double cgp_fit_point(const double* w, const double* lo, const double* hi, double step, int r, int j) {
  if (r == 0 || (r - 1) / 2 != j) return w[j];
  return ((r - 1) & 1) == 0 ? cgp_fit_up(w[j], step, hi[j]) : cgp_fit_dn(w[j], step, lo[j]);
}

// column c (0 .. 2 d + 1) of the device row of that point: lambda | theta | alpha = theta + kappa | bw
CCGP_CHAIN_HD inline double cgp_fit_row_entry(const double* w, const double* lo, const double* hi, double step, int d, int r,
                                              int c) {
#pragma clang fp contract(off)
  if (c <= d) return cgp_fit_point(w, lo, hi, step, r, c);
  if (c == 2 * d + 1) return cgp_fit_point(w, lo, hi, step, r, d + 2);
  const double theta = cgp_fit_point(w, lo, hi, step, r, c - d), kappa = cgp_fit_point(w, lo, hi, step, r, d + 1);
  return theta + kappa;
}

CCGP_CHAIN_HD inline double cgp_fit_value(double val) { return fit_finite(val) ? val : 1e6; }

// g_j from the values of rows 1 + 2 j and 2 + 2 j
CCGP_CHAIN_HD inline double cgp_fit_grad(double val_up, double val_dn, double w, double step, double lo, double hi) {
#pragma clang fp contract(off)
  const double num = cgp_fit_value(val_up) - cgp_fit_value(val_dn);
  const double den = cgp_fit_up(w, step, hi) - cgp_fit_dn(w, step, lo);
  return num / den;
}

}  // namespace ccgp
