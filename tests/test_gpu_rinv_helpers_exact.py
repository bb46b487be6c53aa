"""The literal R.Inv helpers (rinv_terms_kernel and predict_factors_kernel of csrc/capi.hip: lane = row, four waves share the
columns, four lanes per column for the column sums) against an exact reference, output by output, out of the C ABI:
ccgp_beta_mle, ccgp_sigma2_mle, ccgp_factors, ccgp_predict_from_factors, ccgp_predict_post -- what the R drop-in calls.

Reference and bands: tests/gauss_exact.py (mpmath, exactly rounded dot products on the fp64 R.Inv, y, r, beta, mean.factor, v1
and v2 exactly as passed -- the helpers take any matrix, so no inverse is formed; with u = 2^-53, c_j = sum_i |A_ij|:
mean.factor_i (n/4 + 8) u sum_j |A_ij| (|y_j| + |beta|); colsum_j (n/4 + 6) u c_j; 1'Ay, sum(A) and e'Ae the same sums carried
through with n/4 + n/64 + 18 (20 for e'Ae); beta (D a0 + |beta| D a1) / |a1| + 2 u |beta|; the predictive mean its dot
product's (n/64 + 12) u sum |mean.factor_i r_i| + 2 u |beta|; the variance sigma2 (D q + 2 |u_t| D s1 / v2 + 4 u (1 + |q| +
u_t^2 / v2)), absolute, so the cancellation near a training point is judged against what the sums can carry).  Nothing in a
band comes from a device run; tests/test_gauss_corr_host.py runs the same cases on the kernels' arithmetic restated in numpy.

Cases: n in (1, 3, 4, 5, 63, 64, 65, 129, 257) -- 4-way column striding, 64-row passes, 4 lanes per column -- each with a
visibly asymmetric matrix and with the long-double inverse, rounded, of a Gaussian mixed matrix of cond1 ~ 1e8; m in (1, 5, 65)
sites, one ON a training point (the exact variance is ~ 0), one so far away that r = 0 (var = sigma2 (1 + 1 / v2)); one NaN in
y, then one in a row of r; and the literal chain at n = 14 (maximin) and n = 65 -- the device's Mixed.corr.matrix, a
long-double solve on the host, beta.MLE, factors, predict.post at 5 sites -- against oracle/mp_check.predict under the band of
tests/test_gpu_predict_exact.py.

Measured on an MI355X (test_zz_report_headroom prints it; largest |dev - ref| / band, limit 1):
    mean.factor 0.15, var.factor1 0.12, var.factor2 0.047, beta.MLE 0.021, sigma2.MLE 0.020, mean 0.098, var 0.36 (on a
    training point the band itself is at most 1e-3 sigma2, asserted); the chain 0.0022 (var), 0.00031 (mean), 8.1e-5 (beta).
The restatement of tests/test_gauss_corr_host.py gives 0.14 for the terms, 0.098 and 0.36 for mean and variance.  No output left
its band and no kernel was changed for this module.

Mutation check (not committed; see tests/test_gpu_gauss_corr_exact.py):
  `for (int j = wave + 4; ...)` in rinv_terms_kernel          18 tests here fail    both older helper tests fail too
  part[3] left out of predict_factors_kernel's combine       16 tests here fail    test_rinv_helpers_and_literal_predict_post fails too
  v1[lane] for v1[i] in predict_factors_kernel (a sixth)      8 tests here fail     all four older tests pass (their
                                                              predict.post stops at n = 64: one pass of rows)

Cost: the references take 3.5 s of host time (exactly rounded dot products over n^2 terms per site; m = 65 only up to n = 65, 5
sites at n = 129 and 257); test_zz_report_headroom asserts REFERENCE_SECONDS_MAX = 30.
"""
import time

import numpy as np
import pytest

import gauss_exact as gx

pytestmark = pytest.mark.gpu

MAX_RATIO = {}                      # output -> largest |dev - ref| / band seen
REFERENCE_SECONDS = [0.0]
REFERENCE_SECONDS_MAX = 30.0


def _timed(fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    REFERENCE_SECONDS[0] += time.perf_counter() - t0
    return out


def _note(name, worst):
    MAX_RATIO[name] = max(MAX_RATIO.get(name, 0.0), worst)


def check_vector(tag, name, dev, T, want_nan=None):
    """the shape, the NaN pattern, every entry inside its band"""
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == T.hi.shape, (tag, name, dev.shape)
    want_nan = np.zeros(dev.shape, dtype=bool) if want_nan is None else want_nan
    assert np.array_equal(np.isnan(dev), want_nan), (tag, name, np.nonzero(np.isnan(dev) != want_nan)[0][:6].tolist())
    worst, bad = gx.worst_ratio(np.where(want_nan, T.hi, dev), T)
    _note(name, worst)
    assert not bad, (tag, name, worst, len(bad), bad[:6])
    return worst


def check_scalar(tag, name, dev, ref):
    ratio = ref.ratio(dev)
    _note(name, ratio)
    assert ratio <= 1.0, (tag, name, dev, ref.hi, ref.band, ratio)
    return ratio


# ----------------------------------------------------------------------------- 1. beta.MLE, sigma2.MLE, factors
@pytest.mark.parametrize("key", gx.HELPER_KEYS, ids=lambda k: "%s-n%d" % k)
def test_rinv_terms_exact(handle, key):
    c = _timed(gx.helper_case, *key)
    ref = _timed(c.terms_reference)
    f = handle.factors(c.A, c.beta, c.y)
    assert f.shape == (2 * c.n + 1,)
    got = dict(mean_factor=check_vector(c.id, "mean.factor", f[:c.n], ref["mean_factor"]),
               colsum=check_vector(c.id, "var.factor1", f[c.n:2 * c.n], ref["colsum"]),
               v2=check_scalar(c.id, "var.factor2", f[2 * c.n], ref["v2"]),
               beta=check_scalar(c.id, "beta.MLE", handle.beta_mle(c.A, c.y), ref["beta_mle"]),
               sigma2=check_scalar(c.id, "sigma2.MLE", handle.sigma2_mle(c.A, c.y, c.beta), ref["sigma2"]))
    print("%-12s %s" % (c.id, "  ".join("%s %.3g" % kv for kv in got.items())))


# ----------------------------------------------------------------------------- 2. predict.post from the caller's terms
@pytest.mark.parametrize("key", gx.HELPER_KEYS, ids=lambda k: "%s-n%d" % k)
def test_predict_from_factors_exact(handle, key):
    c = _timed(gx.helper_case, *key)
    Tm, Tv = _timed(c.predict_reference)
    mean, var = handle.predict_from_factors(c.r, c.beta, c.mf, c.v1, c.v2, c.A, gx.HELPER_SIGMA2)
    got = (check_vector(c.id, "mean", mean, Tm), check_vector(c.id, "var", var, Tv))
    print("%-12s m = %-3d mean %.3g  var %.3g" % ((c.id, c.m) + got))
    if c.on is not None and c.n > 1:
        # ON a training point: the exact variance all but vanishes and the band is what the sums can carry
        assert abs(Tv.hi[c.on]) <= 1e-4 * gx.HELPER_SIGMA2 and Tv.band[c.on] <= 1e-3 * gx.HELPER_SIGMA2, (c.id, Tv.hi[c.on], Tv.band[c.on])
    if c.far is not None:
        assert (c.r[c.far] == 0.0).all() and mean[c.far] == c.beta
        want = gx.HELPER_SIGMA2 * (1.0 + 1.0 / c.v2)
        assert abs(var[c.far] - want) <= 4 * np.spacing(want), (c.id, var[c.far], want)


# ----------------------------------------------------------------------------- 3. NaN
def test_nan_in_y_and_in_a_row_of_r(handle):
    """One NaN in y: every mean.factor (each row's product reads it), beta.MLE and sigma2.MLE are NaN; the column sums and
    var.factor2, which never read y, stay inside their bands.  One NaN in a row of r: that site's mean and variance are NaN
    and nobody else's."""
    c = _timed(gx.helper_nan_case)
    ref = _timed(c.terms_reference)
    y = c.y.copy()
    y[gx.NAN_Y] = np.nan
    f = handle.factors(c.A, c.beta, y)
    assert np.isnan(f[:c.n]).all()
    check_vector(c.id, "var.factor1", f[c.n:2 * c.n], ref["colsum"])
    check_scalar(c.id, "var.factor2", f[2 * c.n], ref["v2"])
    assert np.isnan(handle.beta_mle(c.A, y)) and np.isnan(handle.sigma2_mle(c.A, y, c.beta))
    Tm, Tv = _timed(c.predict_reference)
    r = c.r.copy()
    r[gx.NAN_R] = np.nan
    mean, var = handle.predict_from_factors(r, c.beta, c.mf, c.v1, c.v2, c.A, gx.HELPER_SIGMA2)
    want = np.arange(c.m) == gx.NAN_R[0]
    check_vector(c.id, "mean", mean, Tm, want)
    check_vector(c.id, "var", var, Tv, want)


# ----------------------------------------------------------------------------- 4. the literal chain
@pytest.mark.parametrize("n", gx.CHAIN_N)
def test_literal_chain_against_the_exact_prediction(handle, n):
    """Mixed.corr.matrix on the device, solve(R) in long double on the host, then beta.MLE, factors and predict.post on the
    device: the whole literal route against a 50-digit prediction from X and y, under the band of the predict.post tables."""
    mean, var, beta = gx.run_chain(n, handle.mixed_corr_matrix, handle.beta_mle, handle.factors, handle.predict_post)
    want_mean, want_var, want_beta, band = _timed(gx.chain_reference, n)
    assert mean.shape == (gx.CHAIN_M,) and var.shape == (gx.CHAIN_M,)
    ratios = dict(mean=float((np.abs(mean - want_mean) / band["mean"]).max()), var=float((np.abs(var - want_var) / band["var"]).max()),
                  beta=abs(beta - want_beta) / band["beta"])
    print("chain n = %d: %s (x band)" % (n, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        _note("chain " + k, v)
    assert (np.abs(mean - want_mean) <= band["mean"]).all(), (n, mean, want_mean, band["mean"])
    assert (np.abs(var - want_var) <= band["var"]).all(), (n, var, want_var, band["var"])
    assert abs(beta - want_beta) <= band["beta"], (n, beta, want_beta, band["beta"])


def test_zz_report_headroom():
    """Largest |dev - ref| / band per output over the module, and the host time the references took."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-12s %.3g" % (k, MAX_RATIO[k]))
    print("references: %.1f s of host time" % REFERENCE_SECONDS[0])
    assert REFERENCE_SECONDS[0] <= REFERENCE_SECONDS_MAX
