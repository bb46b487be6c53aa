"""prediction()'s per-site summaries on the device (ccgp_predict_summary / _dev / ccgp_summary_from_factorset; HX:686-703,
GV:620-638) against the definition evaluated by tests/summary_ref.py on the tables of Handle.predict_batch.

Acceptance of a quantile q at level p, step CDFs included (summary_ref.quantile_residual): with delta = 4 ulp(q) and f the
reference mixture density at q,   F_ref(q - delta) - tol <= p <= F_ref(q + delta) + tol,   tol = 64 eps + 4 ulp(q) f.
64 eps: erfc is at most 16 ulp in a conforming math library, F averages values in [0, 1], the tree sum adds about
log2(S) eps; roughly a factor two of margin.  y_hat / pred_var: 8 eps (log2 S + 2) mean|term| against numpy; quant and
cdf_at: 64 eps.
"""
import os
import re

import numpy as np
import pytest
from scipy.special import ndtri

import summary_ref as ref
from conftest import ROOT, load_gv, load_maximin, synthetic_design
from ccgp_amd import api, fit
from ccgp_amd.rsurface import CombinedGP

pytestmark = pytest.mark.gpu

EPS = ref.EPS
LEVELS = (1e-9, 0.025, 0.5, 0.975, 1.0 - 1e-9)
LEVELS8 = LEVELS + (0.1, 0.25, 0.9)
EINVAL = -1


def lds_cap():
    text = open(os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc", "ccgp_internal.h")).read()
    return int(re.search(r"constexpr int kSummaryLdsDraws = (\d+);", text).group(1))


def iso_params(S, d, seed, t1=(0.5, 4.0), t2=(10.0, 60.0)):
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([[p, 1.0 - p], np.full(d, a), np.full(d, b)])
                     for p, a, b in zip(rng.uniform(0.2, 0.8, S), rng.uniform(*t1, S), rng.uniform(*t2, S))])


def maximin_problem():
    D = load_maximin(14)
    y = np.sin(2 * np.pi * D[:, 0]) + 3.0 * D[:, 1] ** 2 + 5.0
    return D, y


def sites(m, d, seed):
    return np.random.default_rng(seed).random((m, d))


def check(res, mean, var, status, probs, y_at=None):
    """Every column of a summary against the definition on the tables (mean, var, status)."""
    ok = np.asarray(status) == 0
    Sv, m = int(ok.sum()), mean.shape[1]
    probs = np.ravel(np.asarray(probs, dtype=np.float64))
    assert res["quantiles"].shape == (m, probs.size)
    depth = np.log2(Sv) + 2.0
    for t in range(m):
        mu, v = mean[ok, t], np.maximum(var[ok, t], 0.0)
        sd = np.sqrt(v)
        y_hat = float(np.mean(mu))
        assert abs(res["y_hat"][t] - y_hat) <= 8 * EPS * depth * np.mean(np.abs(mu)), (t, res["y_hat"][t], y_hat)
        term = v + (mu - y_hat) ** 2
        assert abs(res["pred_var"][t] - np.mean(term)) <= 8 * EPS * depth * np.mean(np.abs(term)), (t, res["pred_var"][t])
        # quant = 1 - F(y_hat) at the y_hat the call returns (checked above): where sigma ~ 1e-8 and every mu_s agrees to
        # a few ulp (a site on a training point), F at numpy's y_hat, one ulp away, is a different number
        want_quant = ref.sf(float(res["y_hat"][t]), mu, sd)
        assert abs(res["quant"][t] - want_quant) <= 64 * EPS, (t, res["quant"][t], want_quant)
        if y_at is None:
            assert np.isnan(res["cdf_at"][t])
        else:
            assert abs(res["cdf_at"][t] - ref.cdf(float(y_at[t]), mu, sd)) <= 64 * EPS, (t, res["cdf_at"][t])
        for j, p in enumerate(probs):
            q = float(res["quantiles"][t, j])
            assert np.isfinite(q), (t, p, q)
            r, tol = ref.quantile_residual(q, float(p), mu, sd)
            print("site %d level %.17g: q = %.17g residual %.3g eps (tol %.3g eps)" % (t, p, q, r / EPS, tol / EPS))
            assert r <= tol, (t, p, q, r / EPS, tol / EPS)


def run_and_check(handle, X, y, K, P, Xt, sigma2, probs, y_at=None):
    mean, var, beta, st = handle.predict_batch(X, y, K, P, Xt, sigma2)
    res = handle.predict_summary(X, y, K, P, Xt, sigma2, probs, y_at)
    np.testing.assert_array_equal(res["status"], st)
    np.testing.assert_array_equal(res["beta"], beta)
    assert res["n_failed"] == int((st != 0).sum())
    check(res, mean, var, st, probs, y_at)
    return res, mean, var, st


@pytest.mark.parametrize("m", [1, 5, 65])
@pytest.mark.parametrize("S", [1, 3, 257, 1000])
def test_maximin14_against_definition(handle, S, m):
    D, y = maximin_problem()
    P, Xt = iso_params(S, 2, 100 + S), sites(m, 2, 7 + m)
    y_at = np.sin(2 * np.pi * Xt[:, 0]) + 3.0 * Xt[:, 1] ** 2 + 5.0
    res, mean, var, _ = run_and_check(handle, D, y, 2, P, Xt, 1.3, LEVELS, y_at)
    if S == 1:
        # one normal: q = mu + sigma Phi^-1(p).  64 eps on F is 64 eps / f on q; ndtri is good to a few ulp of z
        for t in range(m):
            mu, sd = mean[0, t], np.sqrt(max(var[0, t], 0.0))
            for j, p in enumerate(LEVELS):
                z = ndtri(p) if p <= 0.5 else -ndtri(1.0 - p)
                q, q0 = res["quantiles"][t, j], mu + sd * z
                f = ref.pdf(q0, np.array([mu]), np.array([sd]))
                assert abs(q - q0) <= 64 * EPS / f + 8 * ref.ulp(q0) + 16 * EPS * sd * abs(z), (t, p, q, q0)


def test_n_probs_0_and_8(handle):
    D, y = maximin_problem()
    P, Xt = iso_params(257, 2, 5), sites(5, 2, 3)
    res8, mean, var, st = run_and_check(handle, D, y, 2, P, Xt, 1.3, LEVELS8)
    res0 = handle.predict_summary(D, y, 2, P, Xt, 1.3, [])
    assert res0["quantiles"].shape == (5, 0)
    res5 = handle.predict_summary(D, y, 2, P, Xt, 1.3, LEVELS)
    for k in ("y_hat", "pred_var", "quant"):
        np.testing.assert_array_equal(res0[k], res8[k])
        np.testing.assert_array_equal(res5[k], res8[k])
    # a level's quantile does not depend on which other levels ride along
    np.testing.assert_array_equal(res5["quantiles"], res8["quantiles"][:, :5])


@pytest.fixture(scope="module")
def gv(handle):
    D, y, Dt, yt = load_gv(50, 1)
    rng = np.random.default_rng(11)
    draws = np.column_stack([rng.uniform(0.3, 0.9, 1000), rng.uniform(0.15, 0.5, 1000), rng.uniform(8.0, 25.0, 1000)])
    return dict(D=D, y=y, Dt=Dt, yt=yt, draws=draws, sigma2=10.0, gp=CombinedGP("GV", handle=handle))


def test_gv_set1_kept_factor_route(handle, gv):
    P = gv["gp"].draws_to_params(gv["D"], gv["draws"][:300])
    Dt = gv["Dt"][:150]
    assert Dt.shape[0] == 150
    run_and_check(handle, gv["D"], gv["y"], 2, P, Dt, gv["sigma2"], (0.025, 0.975), gv["yt"][:150])


def test_n130_blocked_route(handle):
    X, y = synthetic_design(130, 3, 4)
    rng = np.random.default_rng(2)
    P = np.array([np.concatenate([[0.6, 0.4], np.exp(rng.uniform(0.0, 1.5, 3)), np.exp(rng.uniform(3.0, 4.0, 3))])
                  for _ in range(4)])
    run_and_check(handle, X, y, 2, P, sites(3, 3, 9), 1.0, LEVELS, np.array([0.1, 0.2, -0.3]))


def test_streamed_route_beyond_the_lds_cap(handle):
    S = lds_cap() + 37
    X, y = synthetic_design(5, 2, 6)
    run_and_check(handle, X, y, 2, iso_params(S, 2, 8, t1=(0.5, 2.0), t2=(5.0, 20.0)), sites(3, 2, 1), 0.8, LEVELS,
                  np.array([0.0, 0.5, 1.0]))


def test_matern_family(handle):
    rng = np.random.default_rng(5)
    X = np.sort(rng.random(8))[:, None]
    y = np.sin(6.0 * X[:, 0])
    P = np.stack([[p, 1.0 - p, a, b] for p, a, b in zip(rng.uniform(0.3, 0.7, 7), rng.uniform(2.0, 6.0, 7),
                                                         rng.uniform(8.0, 20.0, 7))])
    try:
        handle.set_kernel(api.KERNEL_MATERN, 5.0)
        run_and_check(handle, X, y, 2, P, rng.random((4, 1)), 0.7, LEVELS)
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)


@pytest.mark.parametrize("S", [3, 257])
def test_site_on_a_training_point(handle, S):
    """sigma ~ 0 there, and some variances come out slightly negative (sigma = 0: a step): the step-CDF criterion
    holds and nothing is NaN."""
    D, y = maximin_problem()
    Xt = np.vstack([D[3], D[9], [0.4, 0.6]])
    res, mean, var, _ = run_and_check(handle, D, y, 2, iso_params(S, 2, 40 + S), Xt, 1.3, LEVELS, np.array([y[3], y[9], 5.0]))
    for k in ("y_hat", "pred_var", "quant", "cdf_at", "quantiles"):
        assert np.isfinite(res[k]).all(), k
    assert np.all(np.diff(res["quantiles"], axis=1) >= 0.0)


def test_failing_draw_is_left_out(handle):
    D, y = maximin_problem()
    good = iso_params(5, 2, 21)
    bad = np.array([0.5, 0.5, 0.0, 0.0, 0.0, 0.0])     # theta1 = theta2 = 0: R is the all-ones matrix
    P = np.vstack([good[:2], bad, good[2:]])
    Xt = sites(5, 2, 2)
    with_bad = handle.predict_summary(D, y, 2, P, Xt, 1.3, LEVELS, np.full(5, 6.0))
    without = handle.predict_summary(D, y, 2, good, Xt, 1.3, LEVELS, np.full(5, 6.0))
    assert with_bad["n_failed"] == 1 and with_bad["status"][2] != 0 and not np.delete(with_bad["status"], 2).any()
    assert without["n_failed"] == 0
    for k in ("y_hat", "pred_var", "quant", "cdf_at", "quantiles"):
        np.testing.assert_array_equal(with_bad[k], without[k])
    none = handle.predict_summary(D, y, 2, np.vstack([bad, bad]), Xt, 1.3, LEVELS, np.full(5, 6.0))
    assert none["n_failed"] == 2
    for k in ("y_hat", "pred_var", "quant", "cdf_at", "quantiles"):
        assert np.isnan(none[k]).all(), k


def test_a_site_does_not_depend_on_its_neighbours(handle):
    D, y = maximin_problem()
    P, Xt = iso_params(257, 2, 13), sites(65, 2, 17)
    y_at = np.linspace(4.0, 9.0, 65)
    whole = handle.predict_summary(D, y, 2, P, Xt, 1.3, LEVELS, y_at)
    alone = handle.predict_summary(D, y, 2, P, Xt[40:41], 1.3, LEVELS, y_at[40:41])
    perm = np.random.default_rng(0).permutation(65)
    shuffled = handle.predict_summary(D, y, 2, P, Xt[perm], 1.3, LEVELS, y_at[perm])
    for k in ("y_hat", "pred_var", "quant", "cdf_at", "quantiles"):
        np.testing.assert_array_equal(alone[k][0], whole[k][40])
        np.testing.assert_array_equal(shuffled[k], whole[k][perm])


def test_host_dev_and_factorset_entries_agree(handle):
    import torch
    D, y = maximin_problem()
    S, m = 257, 5
    P, Xt = iso_params(S, 2, 13), sites(m, 2, 19)
    y_at = np.linspace(4.0, 9.0, m)
    host = handle.predict_summary(D, y, 2, P, Xt, 1.3, LEVELS, y_at)
    with handle.factor_batch(D, y, 2, P, 1.3) as fs:
        kept = fs.summary(Xt, LEVELS, y_at)
    dev = torch.device("cuda:0")
    col = lambda a: torch.tensor(np.asarray(a, dtype=np.float64).ravel(order="F"), device=dev)  # noqa: E731
    dX, dy, dP, dXt, dyat = col(D), col(y), col(P), col(Xt), col(y_at)
    d_out = torch.empty(m * (4 + len(LEVELS)), dtype=torch.float64, device=dev)
    d_beta = torch.empty(S, dtype=torch.float64, device=dev)
    d_st = torch.empty(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    handle.predict_summary_dev(dX, 14, 2, dy, 2, dP, S, dXt, m, 1.3, LEVELS, dyat, d_out, d_beta, d_st)
    handle.synchronize()
    out = d_out.cpu().numpy().reshape((m, 4 + len(LEVELS)), order="F")
    assert not d_st.cpu().numpy().any()
    np.testing.assert_array_equal(d_beta.cpu().numpy(), host["beta"])
    assert kept["n_failed"] == 0
    for c, k in enumerate(("y_hat", "pred_var", "quant", "cdf_at")):
        np.testing.assert_array_equal(out[:, c], host[k])
        np.testing.assert_array_equal(kept[k], host[k])
    np.testing.assert_array_equal(out[:, 4:], host["quantiles"])
    np.testing.assert_array_equal(kept["quantiles"], host["quantiles"])
    # without y_at, beta and status buffers
    handle.predict_summary_dev(dX, 14, 2, dy, 2, dP, S, dXt, m, 1.3, LEVELS, None, d_out)
    handle.synchronize()
    out2 = d_out.cpu().numpy().reshape((m, 4 + len(LEVELS)), order="F")
    assert np.isnan(out2[:, 3]).all()
    np.testing.assert_array_equal(np.delete(out2, 3, axis=1), np.delete(out, 3, axis=1))


@pytest.mark.parametrize("probs", [[0.0], [1.0], [float("nan")], [0.5, 0.0], list(np.linspace(0.1, 0.9, 9))])
def test_bad_levels_are_refused(handle, probs):
    D, y = maximin_problem()
    with pytest.raises(api.CcgpError) as e:
        handle.predict_summary(D, y, 2, iso_params(3, 2, 1), sites(2, 2, 1), 1.3, probs)
    assert e.value.code == EINVAL
    with handle.factor_batch(D, y, 2, iso_params(3, 2, 1), 1.3) as fs:
        with pytest.raises(api.CcgpError) as e:
            fs.summary(sites(2, 2, 1), probs)
        assert e.value.code == EINVAL


def test_no_sites_is_refused(handle):
    D, y = maximin_problem()
    with pytest.raises(api.CcgpError) as e:
        handle.predict_summary(D, y, 2, iso_params(3, 2, 1), np.empty((0, 2)), 1.3, [0.5])
    assert e.value.code == EINVAL


def test_compare_gp_exact(handle, gv):
    Dt, yt, draws = gv["Dt"][:12], gv["yt"][:12], gv["draws"][:300]
    t = fit.compare_GP(gv["gp"], Dt, 0.05, yt, draws, gv["D"], gv["sigma2"], gv["y"], exact=True)
    assert sorted(t) == ["LL", "UL", "quant", "y_hat", "y_true"]
    assert np.all(t["LL"] < t["y_hat"]) and np.all(t["y_hat"] < t["UL"])
    assert np.all((t["quant"] > 0.0) & (t["quant"] < 1.0))
    np.testing.assert_array_equal(t["y_true"], yt)
    p = gv["gp"].prediction(Dt, 0.05, draws, gv["D"], gv["sigma2"], gv["y"], y_test=yt)
    np.testing.assert_array_equal(p["LL"], t["LL"])
    assert np.all((p["cdf_at"] >= 0.0) & (p["cdf_at"] <= 1.0))


def test_default_compare_gp_is_unchanged(handle, gv):
    Dt, yt, draws = gv["Dt"][:12], gv["yt"][:12], gv["draws"][:300]
    got = fit.compare_GP(gv["gp"], Dt, 0.05, yt, draws, gv["D"], gv["sigma2"], gv["y"], rng=0)
    tab = gv["gp"].prediction_table(Dt, draws, gv["D"], gv["sigma2"], gv["y"])
    rng = np.random.default_rng(0)
    mean, var = tab["mean"], tab["var"]
    y_hat = mean.mean(axis=0)
    post = rng.normal(mean, np.sqrt(np.maximum(var, 0.0)))
    want = dict(y_hat=y_hat, quant=(y_hat[None, :] <= post).mean(axis=0), LL=np.quantile(post, 0.025, axis=0),
                UL=np.quantile(post, 0.975, axis=0), mean=mean, var=var, y_true=yt)
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])


def test_sampled_interval_converges_to_the_exact_one(handle, gv):
    """200 runs of the sampled path at S = 1000: the mean of the sampled LL against the exact LL.  The sampled path draws
    ONE variate from each draw's normal, so its empirical CDF at q is unbiased for F(q) with variance <= p (1 - p) / S:
    MCSE = sqrt(p (1 - p) / S) / f bounds the standard error of the sample quantile to first order, and the mean of 200
    runs lies within 4 MCSE / sqrt(200).  The sample-quantile estimator (numpy's default, linear interpolation between
    order statistics) is biased at O(1 / S): its plotting position is off by at most 1 / S in probability, 1 / (S f) in
    q, and the curvature of F^-1 adds p (1 - p) |f'| / (2 S f^3) (second-order delta method).  Both from the reference
    density."""
    S, reps, p = 1000, 200, 0.025
    Dt = gv["Dt"][:8]
    tab = gv["gp"].prediction_table(Dt, gv["draws"], gv["D"], gv["sigma2"], gv["y"])
    assert not tab["status"].any()
    exact = fit.compare_GP(gv["gp"], Dt, 2 * p, gv["yt"][:8], gv["draws"], gv["D"], gv["sigma2"], gv["y"], exact=True)
    mean, sd = tab["mean"], np.sqrt(np.maximum(tab["var"], 0.0))
    rng = np.random.default_rng(2024)
    LL = np.stack([np.quantile(rng.normal(mean, sd), p, axis=0) for _ in range(reps)])
    for t in range(Dt.shape[0]):
        mu, s = mean[:, t], sd[:, t]
        q = exact["LL"][t]
        f = ref.pdf(q, mu, s)
        hstep = 1e-4 * np.sqrt(np.mean(s ** 2))
        fprime = (ref.pdf(q + hstep, mu, s) - ref.pdf(q - hstep, mu, s)) / (2 * hstep)
        mcse = np.sqrt(p * (1 - p) / S) / f
        bias = 1.0 / (S * f) + p * (1 - p) * abs(fprime) / (2 * S * f ** 3)
        band = 4 * mcse / np.sqrt(reps) + bias
        print("site %d: exact LL %.6f sampled mean %.6f band %.2e" % (t, q, LL[:, t].mean(), band))
        assert abs(LL[:, t].mean() - q) <= band, (t, LL[:, t].mean(), q, band)
