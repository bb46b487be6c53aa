"""The yardstick of tests/test_gpu_loo.py, on the host (tests/loo_ref.py): the closed form IS predict.post on the n - 1 other
points, its bands hold a plain fp64 evaluation on every case the device file uses, and fit.leave_one_out's host arithmetic."""
import numpy as np
import pytest
from scipy.stats import t as student_t

import loo_ref as lr
from oracle import ccgp_oracle as orc

LD_EPS = float(np.finfo(np.longdouble).eps)
# the long-double unit of test 1: both sides are long-double evaluations with errors of about eps_ld cond1 of the sizes each
LD_C = 64.0


def _subset_tables(X, y, row, K, i, Rc=None):
    """Long-double predict.post at x_i from the n - 1 other points, everything recomputed there: (mean, unit = 1 - q + u^2 /
    s11, plug_unit = 1 - q, Q_{-i})."""
    n = X.shape[0]
    keep = np.arange(n) != i
    d = X.shape[1]
    sub = None if Rc is None else [M[np.ix_(keep, keep)] for M in Rc]
    f = orc.predict_factor(X[keep], y[keep], row, K, d, np.longdouble, Rc=sub)
    if Rc is None:
        p = orc.predict_parts(X[keep], y[keep], row, K, d, 1.0, X[i:i + 1], np.longdouble, factor=f)
    else:
        p = orc.predict_parts(X[keep], y[keep], row, K, d, 1.0, X[i:i + 1], np.longdouble, factor=f,
                              rc=[M[i, keep][None, :] for M in Rc], rho=0.0, rho_t=np.zeros(1))
    yc = f["y"] - f["beta"]
    return p["mean"][0], p["var"][0], np.longdouble(1) - p["ww"][0], yc @ f["g"]


def _closed_form_is_predict_post(X, y, row, K, Rc=None, rho=None):
    n = X.shape[0]
    ref = lr.reference(X, y, row, K, Rc=Rc, rho=rho)
    bnd = lr.bands(ref, unit=LD_C * LD_EPS * ref["cond1"])
    s2 = 0.7
    worst = {}
    for i in range(n):
        mean, unit, plug, Qi = _subset_tables(X, y, row, K, i, Rc)
        want = {lr.ORDINARY: s2 * unit, lr.PLUGIN: s2 * plug, lr.UNBIASED: Qi / np.longdouble(n - 2) * unit}
        e = abs(float(ref["mean"][i] - mean))
        assert e <= bnd["mean"][i], (i, "mean", e, bnd["mean"][i])
        worst["mean"] = max(worst.get("mean", 0.0), abs(float((ref["mean"][i] - mean) / mean)))
        for form in lr.FORMS:
            got = lr.variance(ref, form, s2)[i]
            band = lr.variance_band(ref, bnd, form, s2)[i]
            assert abs(float(got - want[form])) <= band, (i, lr.FORM_NAMES[form], float(got), float(want[form]), band)
            name = lr.FORM_NAMES[form]
            worst[name] = max(worst.get(name, 0.0), abs(float((got - want[form]) / want[form])))
    print("cond1 %.3g, largest relative difference closed form - subsets:" % ref["cond1"], worst)
    # long double against long double: far inside anything fp64 can see
    assert max(worst.values()) <= 1e-12


# ----------------------------------------------------------------------------- 1. the identities
def test_closed_form_is_predict_post_on_every_subset_gaussian():
    orc.require_extended_precision()
    X, y, P = lr.gauss_case(14, 3, 2)
    _closed_form_is_predict_post(X, y, P[0], 2)


def test_closed_form_is_predict_post_on_every_subset_matern():
    orc.require_extended_precision()
    import test_gpu_family_end_to_end as fe
    x, y, rows = lr.family_case(1, 14)
    gram = fe._component_tables(1, rows[0], x, x)
    _closed_form_is_predict_post(x[:, None], y, rows[0], 2, Rc=[T.longdouble() for T in gram], rho=0.0)


def test_fp64_identity_against_the_oracle():
    """The fp64 statement of the issue: the closed form in LAPACK arithmetic against oracle.predict_post_iso on subsets."""
    rng = np.random.default_rng(3)
    n, d = 14, 3
    X = rng.random((n, d))
    y = np.sin(3.0 * X).sum(axis=1)
    p, t1, t2, s2 = 0.7, 1.5, 9.0, 1.3
    row = orc.params_from_iso(p, t1, t2, d)
    cf = lr.fp64_evaluation(orc.mixed_corr_matrix_iso(X, p, t1, t2), y)
    for i in range(n):
        keep = np.arange(n) != i
        m, v = orc.predict_post_iso(X[i], X[keep], y[keep], p, t1, t2, s2)
        assert abs(cf["mean"][i] - m) <= 1e-10 * abs(m) and abs(lr.variance(cf, lr.ORDINARY, s2)[i] - v) <= 1e-10 * abs(v)
    assert row.shape == (2 + 2 * d,)


# ----------------------------------------------------------------------------- 2. the reference alone passes its bands
def _check_fp64(tag, ref, bnd, cf, sigma2):
    worst = {}
    checks = [("mean", np.abs(cf["mean"] - lr._f64(ref["mean"])), bnd["mean"]),
              ("beta", abs(cf["beta"] - float(ref["beta"])), bnd["beta"]), ("Q", abs(cf["Q"] - float(ref["Q"])), bnd["Q"])]
    for form in (lr.FORMS if ref["n"] >= 3 else (lr.ORDINARY, lr.PLUGIN)):      # UNBIASED divides by n - 2
        err = np.abs(lr.variance(cf, form, sigma2) - lr._f64(lr.variance(ref, form, sigma2)))
        checks.append((lr.FORM_NAMES[form], err, lr.variance_band(ref, bnd, form, sigma2)))
    for name, err, band in checks:
        worst[name] = float(np.max(err / band)) * lr.C
        assert np.all(err <= band), (tag, name, worst[name])
    print(tag, "cond1 %.3g rho %.3g:" % (ref["cond1"], ref["rho"]), " ".join("%s %.3g" % kv for kv in sorted(worst.items())),
          "(x band / C)")
    return worst


@pytest.mark.parametrize("n,d,K", lr.reg_shapes() + lr.BLOCKED_SHAPES)
def test_fp64_evaluation_sits_inside_every_band_gaussian(n, d, K):
    """Plain fp64 numpy (LAPACK's inverse of the expanded-form matrix) on every Gaussian case of the device file."""
    orc.require_extended_precision()
    _, y, _ = lr.gauss_case(n, d, K)
    for b in range(lr.B):
        ref, bnd = lr.gauss_reference(n, d, K, b)
        _check_fp64((n, d, K, b), ref, bnd, lr.fp64_evaluation(lr.gauss_fp64_matrix(n, d, K, b), y), lr.SIGMA2[b])


@pytest.mark.parametrize("family,n", lr.FAMILY_CASES)
def test_fp64_evaluation_sits_inside_every_band_families(family, n):
    """The same for the 1-D families: the exact entries rounded to fp64, LAPACK's inverse, the closed form."""
    orc.require_extended_precision()
    x, y, rows = lr.family_case(family, n)
    for b in range(len(rows)):
        ref, bnd, R64 = lr.family_reference(family, n, b)
        _check_fp64((family, n, b), ref, bnd, lr.fp64_evaluation(R64, y), 1.3)


# ----------------------------------------------------------------------------- 3. fit.leave_one_out's host arithmetic
class _StubHandle:
    """What fit.leave_one_out asks of a handle: loo_summary's dict and one loo_batch row, with recognisable numbers."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def loo_summary(self, X, y, K, params, sigma2, probs):
        self.calls.append(("summary", K, np.asarray(params).shape, float(sigma2), tuple(probs)))
        n = self.n
        q = np.column_stack([np.arange(n) - 1.0, np.arange(n) + 1.0])
        return dict(y_hat=np.arange(n) + 0.0, pred_var=np.full(n, 0.25), quant=np.full(n, 0.5), cdf_at=np.linspace(0.1, 0.9, n),
                    quantiles=q, beta=np.zeros(len(params)), status=np.zeros(len(params), dtype=np.int32), n_failed=0)

    def loo_batch(self, X, y, K, params, sigma2, form=0):
        self.calls.append(("batch", K, np.asarray(params).shape, None if sigma2 is None else tuple(np.ravel(sigma2)), form))
        n = self.n
        return (np.arange(n)[None] + 0.5, np.linspace(-1e-18, 4.0, n)[None], np.zeros(1), np.ones(1), np.zeros(1, dtype=np.int32))


def test_fit_leave_one_out_host_arithmetic():
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP
    n, d, alpha = 9, 2, 0.1
    rng = np.random.default_rng(5)
    D, y = rng.random((n, d)), rng.random(n)
    stub = _StubHandle(n)
    gp = CombinedGP("HX", handle=stub)
    draws = [(0.8, 0.3, 15.0), (0.6, 0.2, 9.0)]
    exact_keys = {"y_hat", "quant", "LL", "UL", "y_true"}
    table = fit.leave_one_out(gp, alpha, draws, D, 1.3, y)
    assert exact_keys <= set(table) and "y_hat_single" not in table and "y_hat_CGP" not in table
    assert np.array_equal(table["y_true"], y) and np.array_equal(table["pit"], np.linspace(0.1, 0.9, n))
    assert np.array_equal(table["LL"], np.arange(n) - 1.0) and np.array_equal(table["UL"], np.arange(n) + 1.0)
    assert stub.calls == [("summary", 2, (2, 2 + 2 * d), 1.3, (alpha / 2.0, 1.0 - alpha / 2.0))]
    s = fit.comparison_summary(table)
    assert s["rmspe"] == pytest.approx(float(np.sqrt(np.mean((y - np.arange(n)) ** 2)))) and s["mean_quantile"] == 0.5
    # the single GP: a given model, the plug-in form for a 2-D script, qt on n - 2 degrees of freedom
    stub.calls.clear()
    table = fit.leave_one_out(gp, alpha, draws, D, 1.3, y, single=dict(theta=[2.0, 3.0], sigma2=0.7))
    assert stub.calls[1] == ("batch", 1, (1, 1 + d), (0.7,), api.VAR_PLUGIN)
    var = np.maximum(np.linspace(-1e-18, 4.0, n), 0.0)                        # a variance rounded below zero gives a zero width
    delta = student_t.ppf(1.0 - alpha / 2.0, n - 2) * np.sqrt(var)
    np.testing.assert_allclose(table["LL_single"], np.arange(n) + 0.5 - delta, rtol=1e-15, atol=0)
    np.testing.assert_allclose(table["UL_single"], np.arange(n) + 0.5 + delta, rtol=1e-15, atol=0)
    assert table["LL_single"][0] == table["UL_single"][0] == 0.5
    assert np.array_equal(table["y_hat_single"], np.arange(n) + 0.5) and table["single"]["sigma2"] == 0.7
    assert {"rmspe_single", "coverage_single"} <= set(fit.comparison_summary(table))
