"""ccgp_loo_batch / ccgp_loo_summary -- leave-one-out cross-validation of the Combined GP from one factorisation per draw
(Dubrule 1983) -- on both routes: the register-resident inverse instance (INV = 4) and identity rows on the blocked sweep;
rsurface.CombinedGP.leave_one_out and fit.leave_one_out on top of them.

Yardstick: tests/loo_ref.py (long double through oracle._chol_inverse; bands C eps cond1(R) (1 + rho) times cancellation-free
sizes, C = PREDICT_TOL_C = 128; tests/test_loo_ref.py holds the closed form to predict.post on every subset and a plain fp64
evaluation to the bands, on the host).  Every entry of both tables, beta and Q must lie in its band, in all three variance
forms; the tier is asserted from the timing counters.

Largest |device - reference| / (band / C) per route and form on an MI355X (test_zz_report_headroom prints them; the limit is
C = 128):
    route                          ordinary  plugin   unbiased  mean     beta     Q
    reg (n = 2 ... 128)            0.0114    0.0437   0.00056   0.0167   0.0205   0.0936      (all from n = 2, cond1 = 1)
    blocked (n = 97, 129, 257)     0.0040    0.0046   0.00007   0.00005  0.00035  0.00002
    Matern(2.5), K = 2             0.00073   0.00086  0.00005   0.00003  0.00001  0.000002
    Matern + spline                0.0011    0.0012   0.00007   0.00006  0.00004  0.00002
No route left its band.  Times (scripts/loo_timing.py, profiles/loo.md): one ccgp_loo_batch call 0.21 ms for 1000 draws on
Ground-Vibrations train_50_1 and on Qian, against 6.8 and 9.6 ms for the n calls of ccgp_predict_batch on the n - 1 other
points; 2.8 ms against 5.5 s at n = 2048 with 8 draws, 6 % above one ccgp_loglik_batch of the same draws.
"""
import functools

import numpy as np
import pytest
from scipy.stats import t as student_t

import loo_ref as lr
import summary_ref as sr
import test_gpu_failure_contract as fc
from conftest import golden, load_qian
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import _timed, small_reg_inverse_supported
from test_gpu_routes import assert_tier

pytestmark = pytest.mark.gpu

B, C, SIGMA2 = lr.B, lr.C, lr.SIGMA2
MAX_RATIO = {}
EXACT_CASES = [("reg",) + c for c in lr.reg_shapes()] + [("blocked",) + c for c in lr.BLOCKED_SHAPES]


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def _tier(t, route, n):
    """small_route_loo's tier from the timing counters: the fused launch alone, or the sweep with its epilogue under solve."""
    assert_tier(t, "r" if route == "reg" else "b", n)
    assert (t["solve"][1] == 0) == (route == "reg"), t


def _note(route, name, ratio):
    key = (route, name)
    MAX_RATIO[key] = max(MAX_RATIO.get(key, 0.0), float(ratio) * C)


def _check_row(tag, route, ref, bnd, form, sigma2, mean, var, beta, q):
    """One row of the device's tables against its reference: every entry within its band."""
    name = lr.FORM_NAMES[form]
    e_mean = np.abs(mean - _f64(ref["mean"]))
    want = _f64(lr.variance(ref, form, sigma2))
    vband = lr.variance_band(ref, bnd, form, sigma2)
    e_var = np.abs(var - want)
    e_beta, e_q = abs(beta - float(ref["beta"])), abs(q - float(ref["Q"]))
    print("%s %s %s: var %.3g mean %.3g beta %.3g Q %.3g (x band / C), cond1 %.3g rho %.3g" % (
        route, tag, name, (e_var / vband).max() * C, (e_mean / bnd["mean"]).max() * C, e_beta / bnd["beta"] * C,
        e_q / bnd["Q"] * C, ref["cond1"], ref["rho"]))
    _note(route, name, (e_var / vband).max())
    _note(route, "mean", (e_mean / bnd["mean"]).max())
    _note(route, "beta", e_beta / bnd["beta"])
    _note(route, "Q", e_q / bnd["Q"])
    bad = np.nonzero(~(e_var <= vband))[0]
    assert bad.size == 0, (route, tag, name, bad[:6], var[bad[:6]], want[bad[:6]], (e_var / vband)[bad[:6]])
    assert (e_mean <= bnd["mean"]).all(), (route, tag, name, (e_mean / bnd["mean"]).max())
    assert e_beta <= bnd["beta"], (route, tag, beta, float(ref["beta"]))
    assert e_q <= bnd["Q"], (route, tag, q, float(ref["Q"]), bnd["Q"])


def _forms(n):
    return lr.FORMS if n >= 3 else (lr.ORDINARY, lr.PLUGIN)          # UNBIASED divides by n - 2


# ----------------------------------------------------------------------------- 1. exact on each route, all three forms
@pytest.mark.parametrize("route,n,d,K", EXACT_CASES, ids=["%s-%d-%d-%d" % c for c in EXACT_CASES])
def test_exact_on_each_route_in_every_form(handle, route, n, d, K):
    assert small_reg_inverse_supported(n, d, K) == (route == "reg")
    X, y, P = lr.gauss_case(n, d, K)
    for form in _forms(n):
        s2_in = None if form == lr.UNBIASED else SIGMA2
        (mean, var, beta, q, st), t = _timed(handle, lambda: handle.loo_batch(X, y, K, P, s2_in, form))
        _tier(t, route, n)
        assert not st.any() and mean.shape == (B, n) and var.shape == (B, n)
        for b in range(B):
            ref, bnd = lr.gauss_reference(n, d, K, b)
            _check_row((n, d, K, b), route, ref, bnd, form, SIGMA2[b], mean[b], var[b], beta[b], q[b])


# ----------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("route,n,d,K", [("reg", 50, 9, 2), ("blocked", 129, 3, 2)], ids=["reg", "blocked"])
@pytest.mark.parametrize("form", lr.FORMS)
def test_a_draw_alone_is_the_draw_inside_a_batch(handle, route, n, d, K, form):
    X, y, P = lr.gauss_case(n, d, K)
    s2 = None if form == lr.UNBIASED else SIGMA2
    batched, t = _timed(handle, lambda: handle.loo_batch(X, y, K, P, s2, form))
    _tier(t, route, n)
    for b in range(B):
        one = handle.loo_batch(X, y, K, P[b:b + 1], None if s2 is None else s2[b:b + 1], form)
        assert one[4][0] == 0
        for got, want in zip(one[:4], batched[:4]):
            assert np.array_equal(got, want[b:b + 1]), (route, form, b)


def test_chunks_of_the_sweep_do_not_change_the_bits(handle):
    """n = 257, B = 5 under a workspace limit of 8 MB: a matrix with its identity rows takes 3.4 MB, so the call runs as
    chunks of 2, 2 and 1 (two timed launch groups each: the finish and the epilogue).  sigma2 and Q go by the row of the call."""
    n, d, K = 257, 3, 2
    X, y, P = lr.gauss_case(n, d, K)
    rows = P[[0, 1, 2, 0, 1]].copy()
    rows[3:, :K] *= 0.5
    s2 = 1.3 * 10.0 ** (np.arange(5) - 2.0)
    for form in lr.FORMS:
        arg = None if form == lr.UNBIASED else s2
        whole, t0 = _timed(handle, lambda: handle.loo_batch(X, y, K, rows, arg, form))
        with fc._limit(handle, 8 << 20):
            cut, t1 = _timed(handle, lambda: handle.loo_batch(X, y, K, rows, arg, form))
        _tier(t0, "blocked", n)
        _tier(t1, "blocked", n)
        assert t0["solve"][1] == 2 and t1["solve"][1] == 6, (t0, t1)
        assert not whole[4].any()
        for a, b in zip(whole, cut):
            assert np.array_equal(a, b), form


# ----------------------------------------------------------------------------- 3. the failure contract
@pytest.mark.parametrize("route,n,d,K", [("reg", 65, 2, 2), ("blocked", 129, 3, 2)], ids=["reg", "blocked"])
@pytest.mark.parametrize("form", lr.FORMS)
def test_singular_rows_fail_alone(handle, route, n, d, K, form):
    """Two rows of five with every theta = 1e-4 (a nearly constant correlation, singular to working precision, as in
    tests/test_gpu_sched.py; d <= 3, where the terms of order theta^4 = 1e-16 are reached within n pivots -- at d = 9 the terms
    of order theta^2 alone span 55 dimensions and n = 50 factorises): status = the pivot the mode-0 likelihood reports for the same row, NaN in the row of both tables,
    beta and Q, return value 2; the other rows keep the bits of a call without the singular rows."""
    from ccgp_amd import api
    X, y, P = lr.gauss_case(n, d, K)
    good = P[[0, 1, 2]]
    rows = np.stack([good[0], good[0], good[1], good[2], good[2]])
    rows[1, K:] = 1e-4
    rows[4, K:] = 1e-4
    s2 = 1.3 * 10.0 ** (np.arange(5) - 2.0)
    arg = None if form == lr.UNBIASED else s2
    Xf, rf = np.asfortranarray(X), np.asfortranarray(rows)
    mean, var = np.empty((5, n), order="F"), np.empty((5, n), order="F")
    beta, q, st = np.empty(5), np.empty(5), np.zeros(5, dtype=np.int32)
    handle.enable_timing(True)
    try:
        rc = api.lib().ccgp_loo_batch(handle._h, api._p(Xf), n, d, api._p(y), K, api._p(rf), 5, api._p(arg), form, api._p(mean),
                                      api._p(var), api._p(beta), api._p(q), api._ipt(st))
        t = handle.get_timing()
    finally:
        handle.enable_timing(False)
    _tier(t, route, n)
    assert rc == 2
    _, _, st_ll = handle.loglik_batch(X, y, K, rows, 1.0)
    assert st[1] > 0 and st[4] > 0 and np.array_equal(st, st_ll), (st, st_ll)
    for b in (1, 4):
        assert np.isnan(mean[b]).all() and np.isnan(var[b]).all() and np.isnan(beta[b]) and np.isnan(q[b])
    keep = [0, 2, 3]
    clean = handle.loo_batch(X, y, K, rows[keep], None if arg is None else s2[keep], form)
    assert not clean[4].any()
    for got, want in zip((mean, var, beta, q), clean[:4]):
        assert np.array_equal(got[keep], want), (route, form)


def test_argument_errors_leave_the_outputs_untouched(handle):
    from ccgp_amd import api
    n, d, K = 14, 3, 2
    X, y, P = lr.gauss_case(n, d, K)
    Xf, rf = np.asfortranarray(X), np.asfortranarray(P)
    poison = -1.2345e77

    def raw(n_rows, s2, form, n_draws=B):
        bufs = [np.full((B, n), poison, order="F"), np.full((B, n), poison, order="F"), np.full(B, poison), np.full(B, poison)]
        st = np.full(B, 77, dtype=np.int32)
        rc = api.lib().ccgp_loo_batch(handle._h, api._p(Xf[:n_rows].copy(order="F")), n_rows, d, api._p(y[:n_rows].copy()), K,
                                      api._p(rf), n_draws, api._p(s2), form, api._p(bufs[0]), api._p(bufs[1]), api._p(bufs[2]),
                                      api._p(bufs[3]), api._ipt(st))
        assert all((b == poison).all() for b in bufs) and (st == 77).all(), "outputs were written"
        return rc

    ok = SIGMA2.copy()
    for form in (-1, 3, 7):
        assert raw(n, ok, form) == -1                               # CCGP_EINVAL
    for form in lr.FORMS:
        assert raw(1, ok, form) == -1                               # a fold needs another point
    assert raw(2, None, lr.UNBIASED) == -1                          # n - 2 = 0
    for form in (lr.ORDINARY, lr.PLUGIN):
        assert raw(n, None, form) == -1
        for v in (np.nan, np.inf, -np.inf, -1e-300):
            s2 = ok.copy()
            s2[1] = v
            assert raw(n, s2, form) == -1, (form, v)
    assert raw(n, ok, lr.ORDINARY, n_draws=0) == 0                  # B == 0: CCGP_OK, nothing to write
    # and the same buffers are written by a good call: sigma2 = 0 is allowed, NULL outputs are allowed
    mean, var, _, _, st = handle.loo_batch(X, y, K, P, np.zeros(B), lr.PLUGIN)
    assert not st.any() and (var == 0.0).all() and np.isfinite(mean).all()
    m2, v2 = np.empty((B, n), order="F"), np.empty((B, n), order="F")
    assert api.lib().ccgp_loo_batch(handle._h, api._p(Xf), n, d, api._p(y), K, api._p(rf), B, None, lr.UNBIASED, api._p(m2),
                                    api._p(v2), None, None, None) == 0
    assert np.array_equal(m2, mean) and np.isfinite(v2).all()


# ----------------------------------------------------------------------------- 4. the 1-D families
@pytest.mark.parametrize("family,n", lr.FAMILY_CASES, ids=["matern-14", "matern-129", "matern+spline-14"])
def test_families_exact_on_the_sweep(handle, family, n):
    """Matern(2.5), K = 2, against the exact entries of tests/family_exact.py; CCGP_KERNEL_MATERN_SPLINE against the closed
    form on the normalised R only (its script's predict.post leaves r un-normalised: not what the closed form reproduces)."""
    import test_gpu_family_end_to_end as fe
    from ccgp_amd import api
    x, y, rows = lr.family_case(family, n)
    s2 = np.array([1.3, 0.13])
    out = {}
    try:
        handle.set_kernel(api.KERNEL_MATERN if family == 1 else api.KERNEL_MATERN_SPLINE, lr.NU)
        for form in lr.FORMS:
            out[form], t = _timed(handle, lambda: handle.loo_batch(x[:, None], y, 2, rows, None if form == lr.UNBIASED else s2, form))
            fe._sweep(t)
            assert t["solve"][1] > 0, t
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    for form in lr.FORMS:
        mean, var, beta, q, st = out[form]
        assert not st.any()
        for b in range(len(rows)):
            ref, bnd, _ = lr.family_reference(family, n, b)
            _check_row((family, n, b), "family%d" % family, ref, bnd, form, s2[b], mean[b], var[b], beta[b], q[b])


# ----------------------------------------------------------------------------- 5. the summary
def test_summary_is_the_summary_of_the_tables(handle):
    """loo_summary at (50, 9, 2), S = 64 with one failed draw, against tests/summary_ref.py applied to loo_batch's own tables
    with y_at = y, under the tolerances of tests/test_gpu_predict_summary.py: cdf_at is the PIT value."""
    from test_gpu_predict_summary import check
    n, d, K, S = 50, 9, 2, 64
    X, y, P = lr.gauss_case(n, d, K)
    rows = np.stack([P[s % B] * np.concatenate([np.ones(K), np.full(K * d, 1.0 + 0.01 * (s // B))]) for s in range(S)])
    rows[5, K:] = 1e-9              # constant to working precision: the terms of order theta^2 = 1e-18 lie below the pivot rule
    probs = (0.025, 0.5, 0.975)
    mean, var, beta, _, st = handle.loo_batch(X, y, K, rows, 1.3, lr.ORDINARY)
    res, t = _timed(handle, lambda: handle.loo_summary(X, y, K, rows, 1.3, probs))
    _tier(t, "reg", n)
    assert st[5] != 0 and not np.delete(st, 5).any() and res["n_failed"] == 1
    np.testing.assert_array_equal(res["status"], st)
    np.testing.assert_array_equal(res["beta"], beta)
    check(res, mean, var, st, probs, y)
    want = sr.summarize(mean[:, :3], var[:, :3], st, probs, y[:3])
    assert np.all(np.abs(res["cdf_at"][:3] - want["cdf_at"]) <= 64 * sr.EPS)
    assert np.all((res["cdf_at"] >= 0.0) & (res["cdf_at"] <= 1.0))
    # the sweep's tables feed the same kernel
    Xb, yb, Pb = lr.gauss_case(129, 3, 2)
    mb, vb, bb, _, sb = handle.loo_batch(Xb, yb, 2, Pb, 0.7, lr.ORDINARY)
    resb, tb = _timed(handle, lambda: handle.loo_summary(Xb, yb, 2, Pb, 0.7, (0.05, 0.95)))
    _tier(tb, "blocked", 129)
    np.testing.assert_array_equal(resb["beta"], bb)
    check(dict(resb, quantiles=resb["quantiles"][:4], y_hat=resb["y_hat"][:4]), mb[:, :4], vb[:, :4], sb, (0.05, 0.95), yb[:4])


# ----------------------------------------------------------------------------- 6. the surface
@functools.lru_cache(maxsize=None)
def _qian_oracle():
    """fp64 oracle closed form on the Qian training set under the draws of hx_golden.json: (D, y, sigma2, draws, mean[S, n], var[S, n])."""
    D, y, _, _ = load_qian()
    draws = np.asarray(golden("hx_golden.json")["draws"])
    s2 = float(np.var(y, ddof=1))
    cfs = [lr.fp64_evaluation(orc.mixed_corr_matrix_iso(D, p, t1, t2), y) for p, t1, t2 in draws]
    return D, y, s2, draws, np.stack([c["mean"] for c in cfs]), np.stack([lr.variance(c, lr.ORDINARY, s2) for c in cfs])


def test_fit_leave_one_out_on_the_qian_training_set(handle):
    """The columns of fit.leave_one_out against the fp64 oracle closed form to rtol 1e-8 (BASELINE's target for Qian
    predictions); comparison_summary gives finite leave-one-out RMSPE and coverage, no test set involved."""
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    D, y, s2, draws, mean, var = _qian_oracle()
    n, alpha = D.shape[0], 0.05
    theta1 = np.array([0.4, 0.9, 0.2, 1.5])
    model = dict(theta=theta1, sigma2=0.8 * s2)
    gp = CombinedGP("HX", handle=handle)
    table = fit.leave_one_out(gp, alpha, draws, D, s2, y, single=model)
    assert {"y_hat", "quant", "LL", "UL", "y_true", "y_hat_single", "LL_single", "UL_single"} <= set(table)
    assert not any(k.endswith("_CGP") for k in table) and np.array_equal(table["y_true"], y)
    want = sr.summarize(mean, var, np.zeros(len(draws), dtype=np.int32), (alpha / 2.0, 1.0 - alpha / 2.0), y)
    np.testing.assert_allclose(table["y_hat"], want["y_hat"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(table["LL"], want["quantiles"][:, 0], rtol=1e-8, atol=0)
    np.testing.assert_allclose(table["UL"], want["quantiles"][:, 1], rtol=1e-8, atol=0)
    np.testing.assert_allclose(table["quant"], want["quant"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(table["pit"], want["cdf_at"], rtol=1e-8, atol=1e-12)
    cf = lr.fp64_evaluation(orc.corr_matrix(D, theta1), y)
    delta = student_t.ppf(1.0 - alpha / 2.0, n - 2) * np.sqrt(lr.variance(cf, lr.PLUGIN, model["sigma2"]))
    np.testing.assert_allclose(table["y_hat_single"], cf["mean"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(table["LL_single"], cf["mean"] - delta, rtol=1e-8, atol=0)
    np.testing.assert_allclose(table["UL_single"], cf["mean"] + delta, rtol=1e-8, atol=0)
    s = fit.comparison_summary(table)
    assert all(np.isfinite(s[k]) for k in ("rmspe", "coverage", "mean_quantile", "rmspe_single", "coverage_single")), s
    assert s["rmspe"] == pytest.approx(float(np.sqrt(np.mean((y - want["y_hat"]) ** 2))), rel=1e-8)
    print("Qian leave-one-out: " + " ".join("%s %.4g" % kv for kv in sorted(s.items())))


def test_one_dimensional_surface_wraps_the_column(handle):
    """CombinedGP1D.leave_one_out takes the design as a vector; the single GP of a 1-D script is the UNBIASED form."""
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP1D
    x, y, rows = lr.family_case(1, 14)
    gp = CombinedGP1D(lr.NU, handle=handle)
    draws = [(0.6, rows[0, 2], rows[0, 3]), (0.4, rows[1, 2], rows[1, 3])]
    try:
        table = fit.leave_one_out(gp, 0.1, draws, x, 0.5, y, single=dict(theta=float(rows[0, 2])))
        handle.set_kernel(api.KERNEL_MATERN, lr.NU)
        m1, v1, _, _, st = handle.loo_batch(x[:, None], y, 1, np.array([[1.0, rows[0, 2]]]), None, lr.UNBIASED)
        res = handle.loo_summary(x[:, None], y, 2, gp.draws_to_params(x, draws), 0.5, (0.05, 0.95))
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    assert st[0] == 0 and np.array_equal(table["y_hat_single"], m1[0]) and np.array_equal(table["single_var"], v1[0])
    delta = student_t.ppf(0.95, 14 - 2) * np.sqrt(np.maximum(v1[0], 0.0))
    np.testing.assert_allclose(table["UL_single"] - table["y_hat_single"], delta, rtol=1e-12)
    assert np.array_equal(table["y_hat"], res["y_hat"]) and np.array_equal(table["pit"], res["cdf_at"])
    assert np.array_equal(table["LL"], res["quantiles"][:, 0]) and np.array_equal(table["UL"], res["quantiles"][:, 1])


def test_zz_report_headroom():
    """Largest |device - reference| / (band / C) per route and quantity: C = 128 is the limit."""
    for route in sorted({k[0] for k in MAX_RATIO}):
        print("max ratio %-8s " % route + "  ".join("%s %.3g" % (k[1], v) for k, v in sorted(MAX_RATIO.items()) if k[0] == route))
