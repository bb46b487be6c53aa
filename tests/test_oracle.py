"""Pins for the CPU oracle (oracle/ccgp_oracle.py).

The reference has no golden vectors and cannot run here (no R), so the oracle is
"parity unpinned" with respect to the reference itself; what CAN be pinned is:
  * agreement with an independent 50-digit mpmath evaluation (different formulation),
  * analytic properties of the model,
  * stability of the committed fixtures (tests/golden/*.json).
"""
import math

import numpy as np
import pytest

from conftest import golden, load_gv, load_hyper, load_maximin, load_qian
from oracle import ccgp_oracle as orc
from oracle import mp_check


def test_gram_matrix_properties():
    D, y, _, _ = load_qian()
    R = orc.corr_matrix(D, [0.3, 1.1, 2.0, 0.7])
    np.testing.assert_allclose(R, R.T, rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.diag(R), 1.0, rtol=0, atol=1e-14)   # expanded form: not exactly 1
    assert np.all(R > 0) and np.all(R <= 1 + 1e-14)
    # direct squared-difference form agrees (HX:352-355 is only an expansion of it)
    diff = D[:, None, :] - D[None, :, :]
    direct = np.exp(-(diff ** 2 * np.array([0.3, 1.1, 2.0, 0.7])).sum(-1))
    np.testing.assert_allclose(R, direct, rtol=1e-13)
    np.testing.assert_allclose(orc.corr_matrix_iso(D, 0.45), orc.corr_matrix(D, [0.45] * 4), rtol=0, atol=0)


def test_corr_vec_is_a_gram_row():
    D, _, Dt, _ = load_qian()
    full = orc.corr_matrix_iso(np.vstack([Dt[:1], D]), 0.8)
    np.testing.assert_allclose(orc.corr_vec_iso(Dt[0], D, 0.8), full[0, 1:], rtol=1e-13)


def test_mix_limits():
    D, _, _, _ = load_qian()
    np.testing.assert_allclose(orc.mixed_corr_matrix_iso(D, 1.0, 0.3, 9.0), orc.corr_matrix_iso(D, 0.3), rtol=1e-15)
    np.testing.assert_allclose(orc.mixed_corr_matrix_iso(D, 0.0, 0.3, 9.0), orc.corr_matrix_iso(D, 9.0), rtol=1e-15)
    D2 = load_maximin(14)
    np.testing.assert_allclose(orc.mixed_corr_matrix_aniso(D2, 0.7, 0.5, 0.9, 0.0),
                               orc.corr_matrix(D2, [0.5, 0.9]), rtol=1e-14)
    w, Th = orc.unpack_params(orc.params_from_iso(0.7, 0.3, 15.0, 4), 2, 4)
    np.testing.assert_allclose(orc.mixed_corr_matrix_general(D, w, Th),
                               orc.mixed_corr_matrix_iso(D, 0.7, 0.3, 15.0), rtol=1e-14)


def test_logpost_decomposition_and_invariances():
    D, y, _, _ = load_qian()
    s2 = 10.0
    t = [math.log(0.3), math.log(15.0), math.log(0.8 / 0.2)]
    lp = orc.logpost(D, t, y, s2, "HX", (7, 3, 3, 28))
    assert lp["val"] == pytest.approx(lp["log_like"] + orc.log_jacobian(t) + orc.log_prior(t, "HX", (7, 3, 3, 28)), rel=1e-15)
    # profiled intercept: shifting y shifts beta and leaves the likelihood alone
    lp2 = orc.logpost(D, t, y + 3.5, s2, "HX", (7, 3, 3, 28))
    assert lp2["beta"] == pytest.approx(lp["beta"] + 3.5, rel=1e-11)
    assert lp2["log_like"] == pytest.approx(lp["log_like"], rel=1e-10)
    # R.Inv really is the inverse; beta.MLE / sigma2.MLE agree with their definitions
    R = orc.mixed_corr_matrix_iso(D, 0.8, 0.3, 15.0)
    np.testing.assert_allclose(lp["R_inv"] @ R, np.eye(64), atol=1e-9)
    one = np.ones(64)
    assert orc.beta_mle(lp["R_inv"], y) == pytest.approx((one @ np.linalg.solve(R, y)) / (one @ np.linalg.solve(R, one)), rel=1e-10)
    u = y - lp["beta"]
    assert orc.sigma2_mle(lp["R_inv"], y, lp["beta"]) == pytest.approx(u @ np.linalg.solve(R, u) / 64, rel=1e-9)
    # general-K form reproduces the likelihood term
    w, Th = orc.unpack_params(orc.params_from_iso(0.8, 0.3, 15.0, 4), 2, 4)
    ll, beta = orc.loglik_general(D, y, w, Th, s2)
    assert ll == pytest.approx(lp["log_like"], rel=1e-13) and beta == pytest.approx(lp["beta"], rel=1e-13)


def test_priors_match_each_script():
    t3 = [0.2, 1.5, -0.4]
    th1, th2 = math.exp(0.2), math.exp(1.5)
    assert orc.log_prior(t3, "GV") == pytest.approx(-4 * 0.2 - 1 / th1 - 6 * 1.5 - 75 / th2)
    assert orc.log_prior(t3, "ISO") == pytest.approx(-4 * 0.2 - 2 / th1 - 6 * 1.5 - 16 / th2)
    assert orc.log_prior(t3, "BSQ") == orc.log_prior(t3, "ISO") == orc.log_prior(t3, "D1")
    assert orc.log_prior(t3, "HX", (7, 3, 3, 28)) == pytest.approx(-8 * 0.2 - 3 / th1 - 4 * 1.5 - 28 / th2)
    t4 = t3 + [0.7]
    assert orc.log_prior(t4, "ANI") == pytest.approx(-0.2 - 0.02 - 1.5 - 1.125 - 2.8 - 4 / math.exp(0.7))
    assert orc.log_jacobian(t4) == pytest.approx(orc.log_jacobian(t3) + 0.7)


def test_dmnorm_against_scipy():
    import scipy.stats as sst
    rng = np.random.default_rng(3)
    A = rng.normal(size=(9, 9))
    S = A @ A.T + 9 * np.eye(9)
    x = rng.normal(size=9)
    assert orc.dmnorm_log(x, 0.3, S) == pytest.approx(sst.multivariate_normal(np.full(9, 0.3), S).logpdf(x), rel=1e-12)
    with pytest.raises(np.linalg.LinAlgError):
        orc.dmnorm_log(x, 0.0, -S)


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_vs_mpmath_maximin14(mode):
    D = load_maximin(14)
    y = np.array([orc.test_function_2d(a, b, 3) for a, b in D])
    for row, K, d in ((orc.params_from_iso(0.8, 1.0, math.exp(0.5), 2), 2, 2),
                      (orc.params_from_aniso(0.7, 0.9, 1.4, 3.0), 2, 2),
                      (np.array([0.5, 0.3, 0.2, 1.0, 2.0, 5.0, 7.0, 20.0, 30.0]), 3, 2)):
        w, Th = orc.unpack_params(row, K, d)
        ll, beta = orc.loglik_general(D, y, w, Th, 0.37, mode, 100.0 ** 2)
        mll, mbeta = mp_check.loglik(D, y, w, Th, 0.37, mode, 100.0 ** 2)
        # 14 points under smooth kernels are badly conditioned (and tau^2 11' makes it worse):
        # fp64 can only be asked for cond * eps, which is also all the reference's R gets.
        S = 0.37 * np.sum(w ** 2) * orc.mixed_corr_matrix_general(D, w, Th) + (mode * 100.0 ** 2)
        tol = 20 * np.linalg.cond(S) * np.finfo(float).eps
        assert abs(ll - float(mll)) <= tol * max(1.0, abs(float(mll))) + 1e-10
        assert abs(beta - float(mbeta)) <= tol * max(1.0, abs(float(mbeta))) + 1e-12


def test_oracle_vs_mpmath_qian_and_prediction():
    D, y, Dt, _ = load_qian()
    s2 = float(np.var(y, ddof=1))
    w, Th = orc.unpack_params(orc.params_from_iso(0.8, 0.3, 15.0, 4), 2, 4)
    for mode in (0, 1):
        ll, beta = orc.loglik_general(D, y, w, Th, s2, mode, 2500.0)
        mll, mbeta = mp_check.loglik(D, y, w, Th, s2, mode, 2500.0)
        assert ll == pytest.approx(float(mll), rel=1e-10)
        assert beta == pytest.approx(float(mbeta), rel=1e-10, abs=1e-12)
    means, variances, _ = mp_check.predict(D, y, w, Th, s2, Dt[:3])
    for j in range(3):
        m, v = orc.predict_post_iso(Dt[j], D, y, 0.8, 0.3, 15.0, s2)
        assert m == pytest.approx(float(means[j]), rel=1e-10)
        assert v == pytest.approx(float(variances[j]), rel=1e-8)


def test_halton_and_qigamma_definitions():
    u = orc.runif_halton(8)
    assert u.tolist() == [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875, 0.0625]
    assert float(mp_check.halton2(5)) == 0.625
    import scipy.stats as sst
    np.testing.assert_allclose(orc.qigamma(u, 7.0, 3.0), sst.invgamma.ppf(u, 7.0, scale=3.0), rtol=1e-12)


def test_golden_files_are_what_the_oracle_produces():
    """Spot re-computation of committed fixtures (guards against oracle drift)."""
    D, y, Dt, _ = load_qian()
    g = golden("hx_golden.json")
    assert len(g["grid"]["values"]) == 624
    for case in g["cases"][::5]:
        p, t1, t2 = case["draw"]
        lp = orc.logpost(D, case["theta_t"], y, case["sigma2"], "HX", (*g["theta1_pars"], *g["theta2_pars"]))
        assert lp["val"] == pytest.approx(case["val"], rel=1e-12)
        assert lp["beta"] == pytest.approx(case["beta"], rel=1e-12)
        assert orc.cond_like_log(D, y, p, t1, t2, case["sigma2"], 50.0) == pytest.approx(case["cond_like_log"], rel=1e-12)
    H = load_hyper("hx")
    i = g["grid"]["which_max"]
    m = orc.likeli_hyperpars(D, y, H[i, :2], H[i, 2:], g["grid"]["sigma2"], 1000, 50.0)
    assert math.log(m) == pytest.approx(g["grid"]["values"][i], rel=1e-11)
    mean, var, beta = orc.predict_table(D, y, g["draws"][:2], Dt, g["predict"]["sigma2"])
    np.testing.assert_allclose(mean, np.array(g["predict"]["mean"])[:2], rtol=1e-11)
    np.testing.assert_allclose(var, np.array(g["predict"]["var"])[:2], rtol=1e-9)

    gv = golden("gv_golden.json")
    for s in gv["sets"]:
        Dg, yg, Dtg, _ = load_gv(s["size"])
        mean, var, _ = orc.predict_table(Dg, yg, s["draws"][:1], Dtg[:5], s["sigma2"])
        np.testing.assert_allclose(mean[0], np.array(s["mean"])[0, :5], rtol=1e-11)

    ga = golden("adv_golden.json")
    D14 = load_maximin(14)
    assert len(ga["grid"]["values"]) == 60 and 0 <= ga["grid"]["which_max"] < 60
    c = ga["cases"][0]
    lp = orc.logpost(D14, c["theta_t"], np.array(ga["y"]), ga["sigma2"], "ADV", tuple(c["prior_pars"]))
    assert lp["val"] == pytest.approx(c["val"], rel=1e-12) and lp["like"] == pytest.approx(c["like"], rel=1e-11)


def test_config1_matern_plumbing():
    """BASELINE config 1 is CPU-only plumbing: Matern nu = 5 on an 8-point 1-D design (D1:348-374)."""
    g = golden("d1_golden.json")
    X = np.array(g["X"]).reshape(-1, 1)
    R = orc.corr_matrix_matern(g["nu"], X, 0.7)
    assert R.shape == (8, 8)
    np.testing.assert_allclose(np.diag(R), 1.0)
    np.testing.assert_allclose(R, R.T)
    assert np.all(np.linalg.eigvalsh(R) > 0)
    # closed form for half-integer nu = 5/2 cross-checks the besselK restatement
    h, th, nu = 0.37, 0.9, 2.5
    z = 2 * math.sqrt(nu) * h / th
    closed = (1 + z + z * z / 3) * math.exp(-z)
    assert float(orc.matern_corr(nu, h, th)) == pytest.approx(closed, rel=1e-12)
    for c in g["cases"]:
        lp = orc.logpost_1d(X, c["theta_t"], np.array(g["y"]), c["sigma2"], g["nu"])
        assert lp["val"] == pytest.approx(c["val"], rel=1e-12)


def test_two_family_script_restatement_and_fixture():
    """D1F: Matern + non-negative cubic spline.  Known answers of the spline (D1F:346-357), the un-normalised
    corr.vec.combined (D1F:479) and the committed fixture."""
    g = golden("d1f_golden.json")
    X = np.array(g["X"]).reshape(-1, 1)
    y = np.array(g["y"])
    assert float(orc.spline_corr(2.0, 0.0)) == 1.0
    assert float(orc.spline_corr(2.0, 1.0)) == pytest.approx(1 - 6 * 0.25 + 6 * 0.125)      # u = 1/2, first branch
    assert float(orc.spline_corr(2.0, 1.5)) == pytest.approx(2 * 0.25 ** 3)                 # u = 3/4, second branch
    assert float(orc.spline_corr(2.0, 2.5)) == 0.0
    Rs = orc.corr_matrix_spline(X, 0.45)
    assert np.all(np.linalg.eigvalsh(Rs) > 0) and np.allclose(np.diag(Rs), 1.0)
    p, t1, t2, nu = 0.7, 0.5, 0.6, g["nu"]
    r = orc.corr_vec_combined(0.41, X, p, t1, t2, nu)
    np.testing.assert_allclose(r, g["r_combined"], rtol=1e-13)
    normalised = r / (p ** 2 + (1 - p) ** 2)
    np.testing.assert_allclose(normalised, (p ** 2 * orc.corr_vec_matern(0.41, X, t1, nu) + (1 - p) ** 2 *
                                            orc.corr_vec_spline(0.41, X, t2)) / (p ** 2 + (1 - p) ** 2), rtol=1e-14)
    for c in g["cases"]:
        lp = orc.logpost_2f(X, c["theta_t"], y, c["sigma2"], nu)
        assert lp["val"] == pytest.approx(c["val"], rel=1e-12)


def test_solve_refuses_a_computationally_singular_matrix_like_base_r():
    """solve(R) inside logpost (HX:454): base R's solve.default stops when rcond < .Machine$double.eps, the reference's
    try() turns that into R.Inv <- NA.  A duplicated design point is singular only up to rounding (LU meets a pivot of
    +-1e-17, not 0): without the rcond test the restatement would return a garbage inverse where R returns NA."""
    from conftest import load_qian
    D, y, _, _ = load_qian()
    Dd = D.copy()
    Dd[40] = Dd[3]
    R = orc.mixed_corr_matrix_iso(Dd, 0.8, 0.3, 15.0)
    with pytest.raises(np.linalg.LinAlgError, match="singular"):
        orc.solve_inverse(R)
    lp = orc.logpost(Dd, [math.log(0.3), math.log(15.0), math.log(4.0)], y, 10.0, "GV")
    assert lp["R_inv"] is None and math.isnan(lp["val"])
    # a well-conditioned matrix goes through and is the LAPACK inverse
    R = orc.mixed_corr_matrix_iso(D, 0.8, 0.3, 15.0)
    np.testing.assert_array_equal(orc.solve_inverse(R), np.linalg.inv(R))


def test_log_likeli_of_the_1d_scripts_known_answer():
    """D1:437-444: log(det(R)) + n log(sigma2.MLE), against a direct evaluation through eigenvalues / lstsq."""
    g = golden("d1_golden.json")
    X, y, nu = np.array(g["X"]).reshape(-1, 1), np.array(g["y"]), g["nu"]
    R = orc.corr_matrix_matern(nu, X, 0.25)
    w = np.linalg.eigvalsh(R)
    one = np.ones(8)
    a = np.linalg.solve(R, np.stack([y, one], axis=1))
    beta = (one @ a[:, 0]) / (one @ a[:, 1])
    r = y - beta
    s2 = (r @ np.linalg.solve(R, r)) / 8
    assert orc.log_likeli_1d(nu, 0.25, X, y) == pytest.approx(np.log(w).sum() + 8 * math.log(s2), rel=1e-9)


# --------------------------------------------------------------------------- exact gradient reference (host only)
LD_EPS = float(np.finfo(np.longdouble).eps)
F64_EPS = float(np.finfo(np.float64).eps)


def _grad_case(n, d, K, seed, sigma2=1.3):
    from conftest import synthetic_design
    X, y = synthetic_design(n, d, seed=seed)
    row, _ = orc.conditioned_row(X, K, d, np.random.default_rng(seed), kappa_max=1e6)
    return X, y, row, sigma2


def test_host_has_extended_precision():
    """The gradient reference needs np.longdouble wider than fp64; it never falls back quietly."""
    orc.require_extended_precision()


@pytest.mark.parametrize("n,d,K", [(12, 1, 1), (17, 4, 1), (20, 1, 3), (24, 4, 3)])
def test_exact_gradient_fp64_longdouble_and_50_digits_agree(n, d, K):
    orc.require_extended_precision()
    X, y, row, s2 = _grad_case(n, d, K, seed=100 + n)
    parts = orc.loglik_grad_parts(X, y, row, K, d, s2, np.longdouble)
    kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
    ll_ld, beta_ld, g_ld, scale = orc.loglik_grad_exact(X, y, row, K, d, s2, np.longdouble)
    ll_64, beta_64, g_64, _ = orc.loglik_grad_exact(X, y, row, K, d, s2, np.float64)
    w, Th = orc.unpack_params(row, K, d)
    g_mp = np.array([float(v) for v in mp_check.loglik_grad(X, y, w, Th, s2)])
    ll_mp, beta_mp = (float(v) for v in mp_check.loglik(X, y, w, Th, s2))
    # long double against 50 digits: a few long-double ulps of cond x scale (plus the fp64 rounding of the results)
    assert np.all(np.abs(g_ld - g_mp) <= 64 * LD_EPS * kappa * scale + 2 * F64_EPS * np.abs(g_mp)), (g_ld - g_mp) / scale
    assert ll_ld == pytest.approx(ll_mp, rel=1e-15) and beta_ld == pytest.approx(beta_mp, rel=1e-14, abs=1e-15)
    # the fp64 closed form (LAPACK) meets the same band the device is held to
    assert np.all(np.abs(g_64 - g_mp) <= orc.grad_tolerance(scale, kappa)), (g_64 - g_mp) / scale
    assert ll_64 == pytest.approx(ll_mp, rel=1e-12) and beta_64 == pytest.approx(beta_mp, rel=1e-11, abs=1e-13)


@pytest.mark.parametrize("n,d,K", [(60, 3, 2), (33, 5, 4)])
def test_exact_gradient_against_central_differences(n, d, K):
    """Central differences with step h_j = 1e-6 max(1, |row_j|) reach about 1e-7 of scale[j] (truncation) plus the
    cancellation of two log-likelihoods, ~10 eps |ll| / h_j; the closed form must sit inside that in every component."""
    X, y, row, s2 = _grad_case(n, d, K, seed=7 * n)
    ll, _, g, scale = orc.loglik_grad_exact(X, y, row, K, d, s2, np.longdouble)
    fd = orc.loglik_grad_fd(X, y, row, K, d, s2)
    h = 1e-6 * np.maximum(1.0, np.abs(row))
    assert np.all(np.abs(fd - g) <= 1e-7 * scale + 10 * F64_EPS * max(1.0, abs(ll)) / h)


def _rejected(g_mut, g_ref, scale, kappa, X, row, K, d):
    rho = orc.expanded_form_magnitude(X, row, K, d)
    return bool(np.any(np.abs(g_mut - g_ref) > orc.grad_tolerance(scale, kappa, rho)))


def _mutation_case(n, d, K, seed):
    X, y, row, s2 = _grad_case(n, d, K, seed)
    parts = orc.loglik_grad_parts(X, y, row, K, d, s2, np.longdouble)
    kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
    g, scale = orc.grad_from_parts(parts, X, row, K, d, s2)
    return X, row, s2, parts, kappa, g, scale


def test_gradient_tolerance_rejects_the_kernel_bugs_it_is_meant_to_catch():
    """The band of tests/test_gpu_gradient_exact.py must be able to fail: each model of a plausible kernel bug, applied to
    the reference formula, moves at least one component outside it."""
    orc.require_extended_precision()
    # diagonal pairs weighted 1 instead of 1/2 (the full sum counts each diagonal term twice)
    for n, d, K in [(40, 3, 2), (130, 2, 1)]:
        X, row, s2, parts, kappa, g, scale = _mutation_case(n, d, K, seed=n)
        W = np.ones((n, n)) + np.eye(n)
        gm, _ = orc.grad_from_parts(parts, X, row, K, d, s2, weights=W)
        assert _rejected(gm, g, scale, kappa, X, row, K, d), "diagonal weight"
    # one lower 64 x 64 tile block of M dropped or doubled at n = 193 (three full row blocks and a one-row ragged one)
    n, d, K = 193, 3, 2
    X, row, s2, parts, kappa, g, scale = _mutation_case(n, d, K, seed=193)
    for (I, J) in [(1, 0), (2, 2), (3, 0), (3, 3)]:
        for factor in (0.0, 2.0):
            W = np.ones((n, n))
            W[64 * I:64 * I + 64, 64 * J:64 * J + 64] = factor
            W[64 * J:64 * J + 64, 64 * I:64 * I + 64] = factor
            gm, _ = orc.grad_from_parts(parts, X, row, K, d, s2, weights=W)
            assert _rejected(gm, g, scale, kappa, X, row, K, d), ("tile", I, J, factor)
    # a padded dimension slot clamped to kk = d - 1 accumulating into dimension d - 1 (d = 5: a KG = 4 pass pads 3 slots)
    n, d, K = 50, 5, 2
    X, row, s2, parts, kappa, g, scale = _mutation_case(n, d, K, seed=5)
    gm = g.copy()
    for q in range(K):
        gm[K + q * d + d - 1] += g[K + q * d + d - 1]
    assert _rejected(gm, g, scale, kappa, X, row, K, d), "padded dimension"
    # the last component group (components 6, 7 of K = 8 in groups of three) never contracted
    n, d, K = 40, 4, 8
    X, row, s2, parts, kappa, g, scale = _mutation_case(n, d, K, seed=8)
    gm = g.copy()
    for q in (6, 7):
        gm[q] = 0.0
        gm[K + q * d:K + (q + 1) * d] = 0.0
    assert _rejected(gm, g, scale, kappa, X, row, K, d), "component group"


def test_exact_inverse_against_lapack():
    orc.require_extended_precision()
    X, y, row, s2 = _grad_case(70, 3, 2, seed=70)
    w, Th = orc.unpack_params(row, 2, 3)
    R = orc.mixed_corr_matrix_general(X, w, Th)
    Rinv = orc.solve_inverse_exact(R)
    kappa = orc.cond1(R, Rinv)
    assert np.abs(np.asarray(Rinv @ R.astype(np.longdouble) - np.eye(70), dtype=np.float64)).max() <= 70 * 70 * LD_EPS * kappa
    bound = np.abs(np.asarray(Rinv, np.float64)) @ np.abs(R) @ np.abs(np.asarray(Rinv, np.float64))
    assert np.all(np.abs(np.linalg.inv(R) - np.asarray(Rinv, np.float64)) <= 16 * 70 * F64_EPS * bound)


# --------------------------------------------------------------------------- exact predict.post tables (host only)
def _predict_sites(X, rng):
    """a training point, that point + 1e-6 and + 1e-3 in one coordinate, two interior points, one far point"""
    d = X.shape[1]
    e = np.eye(d)[d - 1]
    return np.vstack([X[3], X[3] + 1e-6 * e, X[3] + 1e-3 * e, rng.random((2, d)), np.full(d, 50.0)])


def _mpf(v):
    """a long double as an mpf, exactly: its fp64 rounding plus the remainder"""
    hi = float(v)
    return mp_check.mp.mpf(hi) + mp_check.mp.mpf(float(v - np.longdouble(hi)))


def _predict_host_cases():
    from conftest import synthetic_design
    D = load_maximin(14)
    y14 = np.array([orc.test_function_2d(a, b, 3) for a, b in D])
    X33, y33 = synthetic_design(33, 3, seed=33)
    return [(D, y14, 2, 2, 14), (X33, y33 + 0.3 * X33[:, 0], 2, 3, 33)]


def test_predict_reference_against_50_digits():
    """The long-double tables sit within band / 64 of mp_check.predict at 50 digits: at a training point (variance ~ 1e-17
    sigma2), its 1e-6 and 1e-3 neighbours, two interior sites and the far site, on maximin-14 and n = 33, d = 3, K = 2."""
    orc.require_extended_precision()
    for X, y, K, d, seed in _predict_host_cases():
        rng = np.random.default_rng(seed)
        row, _ = orc.conditioned_row(X, K, d, rng, kappa_max=1e8)
        Xt = _predict_sites(X, rng)
        parts = orc.predict_parts(X, y, row, K, d, 0.8, Xt, np.longdouble)
        band = orc.predict_bands(parts, 0.8)
        w, Th = orc.unpack_params(row, K, d)
        m_mp, v_mp, b_mp = mp_check.predict(X, y, w, Th, 0.8, Xt)
        # the differences are formed at 50 digits: a variance of 1e-17 is not rounded to fp64 before it is compared
        ev = np.array([abs(float(_mpf(v) - vm)) for v, vm in zip(parts["var"], v_mp)])
        em = np.array([abs(float(_mpf(v) - vm)) for v, vm in zip(parts["mean"], m_mp)])
        eb = abs(float(_mpf(parts["beta"]) - b_mp))
        assert float(parts["var"][0]) < 1e-12 * 0.8 and (np.asarray(parts["r"][-1], np.float64) == 0).all()
        assert (ev <= band["var"] / 64).all(), ev / band["var"]
        assert (em <= band["mean"] / 64).all(), em / band["mean"]
        assert eb <= band["beta"] / 64


def _planted(dev, sigma2, plant, s11_other=None):
    """oracle.predict_device_finish with one planted kernel mistake."""
    w, rd, z1, zy, beta, s11 = dev["w"], dev["rd"].copy(), dev["z1"], dev["zy"], dev["beta"], dev["s11"]
    n = rd.shape[0]
    if plant == "reciprocal twice":
        rd[n // 2] *= rd[n // 2]
    if plant == "neighbour r":
        w = np.roll(w, -1, axis=0)
    wr = w * rd[None, :]
    ww = (w[:, :n - 1] * wr[:, :n - 1]).sum(axis=1) if plant == "row n-1 out of ww" else (w * wr).sum(axis=1)
    z1w, zyw = wr @ z1, wr @ zy
    u = 1.0 - z1w
    if plant == "neighbour s11":
        s11 = s11_other
    mean = beta + (zyw + beta * z1w if plant == "beta z1w sign" else zyw - beta * z1w)
    var = sigma2 * (1.0 - ww + (0.0 if plant == "u u / s11 dropped" else u * u / s11))
    return mean, var


def test_predict_band_rejects_the_kernel_mistakes_it_is_meant_to_catch():
    """Each planted mistake, applied to the fp64 restatement of the device's formula, leaves the band by a factor of at least
    1e3 at some site; the restatement itself stays inside."""
    orc.require_extended_precision()
    for X, y, K, d, seed in _predict_host_cases():
        rng = np.random.default_rng(seed)
        rows = [orc.conditioned_row(X, K, d, rng, kappa_max=1e8)[0] for _ in range(2)]
        Xt = np.vstack([_predict_sites(X, rng), X[-1]])
        parts = orc.predict_parts(X, y, rows[0], K, d, 0.8, Xt, np.longdouble)
        band = orc.predict_bands(parts, 0.8)
        ref_mean, ref_var = np.asarray(parts["mean"], np.float64), np.asarray(parts["var"], np.float64)
        dev = orc.predict_device_restatement(X, y, rows[0], K, d, Xt)
        other = orc.predict_device_restatement(X, y, rows[1], K, d, Xt)["s11"]

        def off(plant):
            mean, var = _planted(dev, 0.8, plant, other)
            return max((np.abs(var - ref_var) / band["var"]).max(), (np.abs(mean - ref_mean) / band["mean"]).max())
        assert off(None) <= 1.0
        for plant in ("row n-1 out of ww", "neighbour r", "u u / s11 dropped", "neighbour s11", "beta z1w sign", "reciprocal twice"):
            assert off(plant) >= 1e3, (plant, off(plant))


_PREDICT_CASE_STATS = {}


def _predict_case_stats():
    """Over every table case of tests/test_gpu_predict_exact.py and its three draws: the largest |fp64 restatement - long
    double| / (band / C) for (var, mean, beta), and the largest band_var / sigma2 at a site on or within 1e-6 of a training
    point, per case.  Computed once for the tests below."""
    if not _PREDICT_CASE_STATS:
        import test_gpu_predict_exact as tp
        orc.require_extended_precision()
        ratio = np.zeros(3)
        caps = {}
        for route, n, d, K, m, kind in tp.all_table_cases():
            X, y, P, Xt = tp.make_case(n, d, K, m, kind)
            near = tp.near_training(X, Xt)
            assert near.any() == (kind == "full")
            for s in range(tp.S):
                parts, band, kappa = tp.reference(X, y, P[s], K, Xt, tp.SIGMA2)
                assert kappa <= tp.KAPPA_MAX, (n, d, K, s, kappa)
                mean, var, *_ = orc.predict_device_finish(orc.predict_device_restatement(X, y, P[s], K, d, Xt), tp.SIGMA2)
                dev_beta = orc.predict_device_restatement(X, y, P[s], K, d, Xt[:1])["beta"]
                ratio = np.maximum(ratio, [(np.abs(var - np.asarray(parts["var"], np.float64)) / band["var"]).max() * tp.C,
                                           (np.abs(mean - np.asarray(parts["mean"], np.float64)) / band["mean"]).max() * tp.C,
                                           abs(dev_beta - float(parts["beta"])) / band["beta"] * tp.C])
                if near.any():
                    key = (route, n, d, K, m)
                    caps[key] = max(caps.get(key, 0.0), float(band["var"][near].max()) / tp.SIGMA2)
                if kind == "plain" and d == 1:
                    caps["rho"] = max(caps.get("rho", 0.0), parts["rho"])
        _PREDICT_CASE_STATS.update(ratio=ratio, caps=caps)
    return _PREDICT_CASE_STATS


def test_predict_constant_has_its_margin_over_the_fp64_restatement():
    """PREDICT_TOL_C is at least 8 times what a plain fp64 evaluation of the device's formula needs, over every case the
    device is run at (the recorded figures: tests/test_gpu_predict_exact.py's docstring)."""
    ratio = _predict_case_stats()["ratio"]
    print("fp64 restatement, largest |fp64 - long double| / (band / C): var %.3g mean %.3g beta %.3g" % tuple(ratio))
    assert orc.PREDICT_TOL_C >= 8.0 * ratio.max(), ratio


def test_predict_variance_band_is_not_vacuous_where_the_variance_cancels():
    """On a training point or within 1e-6 of one the variance band is at most 1e-9 sigma2 in every case with such sites (all
    but the d = 63 witness and the d = 1 case, which has rho ~ 1e4 to exercise that term instead)."""
    caps = dict(_predict_case_stats()["caps"])
    assert caps.pop("rho") >= 3e3
    assert len(caps) == 36                                        # 19 kept-factor, 8 extra-row and 9 blocked cases
    worst = max(caps, key=caps.get)
    print("largest band_var / sigma2 near a training point: %.3g at %s" % (caps[worst], worst))
    assert caps[worst] <= 1e-9, (worst, caps[worst])


# --------------------------------------------------------------------------- exact marginal likelihood, mode 1 (host only)
def _marginal_host_cases():
    from conftest import synthetic_design
    D = load_maximin(14)
    y14 = np.array([orc.test_function_2d(a, b, 3) for a, b in D])
    X21, y21 = synthetic_design(21, 3, seed=21)
    return [(D, y14, 2, 2, 14), (X21, y21 + 0.3 * X21[:, 0], 3, 3, 21)]


@pytest.mark.parametrize("tau2", [0.0, 2500.0])
def test_marginal_reference_against_50_digits(tau2):
    """oracle.marginal_parts in long double against mp_check.loglik(..., 1, tau2): 1e-17 relative on maximin-14 (K = 2) and on
    n = 21, d = 3, K = 3; the difference is formed at 50 digits."""
    orc.require_extended_precision()
    for X, y, K, d, seed in _marginal_host_cases():
        row, _ = orc.conditioned_row(X, K, d, np.random.default_rng(seed), kappa_max=1e3)
        parts = orc.marginal_parts(X, y, row, K, d, 0.8, tau2, np.longdouble)
        w, Th = orc.unpack_params(row, K, d)
        ll_mp, beta_mp = mp_check.loglik(X, y, w, Th, 0.8, 1, tau2)
        assert beta_mp == 0 and parts["beta"] == 0
        assert abs(float(_mpf(parts["loglik"]) - ll_mp)) <= 1e-17 * abs(float(ll_mp)), (seed, tau2)
        # the two matrices differ by tau2 exactly, and M is the derivative the band is built on: central difference in tau2
        assert np.array_equal(parts["Sigma"] - parts["Sigma0"], np.full_like(parts["Sigma"], np.longdouble(tau2)))
        h = np.longdouble(1e-4) * max(tau2, 1.0)
        up = orc.marginal_parts(X, y, row, K, d, 0.8, np.longdouble(tau2) + h, np.longdouble)["loglik"]
        dn = orc.marginal_parts(X, y, row, K, d, 0.8, np.longdouble(tau2) - h, np.longdouble)["loglik"] if tau2 else None
        if dn is not None:
            assert float((up - dn) / (2 * h)) == pytest.approx(float(parts["M"].sum()), rel=1e-6)


def test_logmeanexp_exact_known_answers():
    orc.require_extended_precision()
    assert float(orc.logmeanexp_exact([-3.5])) == -3.5 and float(orc.logmeanexp_exact([-3.5], False)) == pytest.approx(math.exp(-3.5), rel=1e-16)
    assert float(orc.logmeanexp_exact([0.0, math.log(3.0)])) == pytest.approx(math.log(2.0), rel=1e-15)
    assert float(orc.logmeanexp_exact([-1e5, -1e5 - 800.0, -1e5 - 2.0])) == pytest.approx(-1e5 + math.log((1 + math.exp(-2.0)) / 3), rel=1e-16)
    v = orc.logmeanexp_exact([-11000.0, -11001.0], False)
    assert 0 < v < np.finfo(np.float64).tiny and float(np.log(v)) == pytest.approx(-11000.0 + math.log((1 + math.exp(-1.0)) / 2), rel=1e-15)


def test_marginal_case_lists_of_the_device_module():
    """Host check of tests/test_gpu_marginal_exact.py's lists: the sizes, dimensions and component counts its docstring names,
    and that no Gaussian likelihood shape below n = 129 takes the blocked sweep (the witness is n = 129)."""
    import route_witnesses
    import test_gpu_marginal_exact as tm
    assert tm.WITNESS == (129, 1, 1) and route_witnesses.RESERVE_CHANGES[0][0] == 0
    small = tm.REG8_CASES + tm.WAVE_CASES + tm.REG16_CASES
    assert {d for _, d, _ in small} == set(range(1, 10)) and {K for _, _, K in small} == {1, 2, 3, 8}
    assert [n for n, _, _ in small] == [2, 5, 8, 9, 63, 64, 65, 72, 104, 105, 127, 128]
    assert [n for n, _, _ in tm.BLOCKED_CASES[1:]] == [129, 191, 192, 193, 255, 256, 257, 383, 385, 520]
    assert {K for _, _, K in tm.BLOCKED_CASES} == {1, 2, 8}
    assert all(tm._lds_fits(tm._reg_lds_doubles8(*c)) for c in tm.WAVE_CASES)
    assert [n for n, _, _ in tm.PAIR_SHAPES] == [14, 100, 128, 257] and [n for n, _, _ in tm.TINY_SHAPES] == [64, 257]
    assert 0.0 < tm.TINY_TAU2[1] < np.finfo(np.float64).tiny and tm.TINY_TAU2[0] == 1e-300


def test_marginal_constant_comes_from_the_fp64_lapack_evaluation():
    """The measurement that fixes MARGINAL_TOL_C: the fp64 LAPACK likelihood with the exponent in the expanded form, on every
    mode-1 draw the device module checks, in units of oracle.marginal_unit; every draw within the condition cap.  C = 32 x the
    largest ratio, rounded up to a power of two, capped at GRAD_TOL_C."""
    import test_gpu_marginal_exact as tm
    orc.require_extended_precision()
    worst, worst_at, kappa_max = 0.0, None, 0.0
    for case in tm.mode1_draws():
        n, d, K, B, b, s2, tau2 = case
        ll_ref, unit, kappa = tm.mode1_reference(*case)
        assert kappa <= orc.MARGINAL_COND_MAX, (case, kappa)
        X, y, rows = tm.make_case(n, d, K, B)
        ll = float(orc.marginal_parts(X, y, rows[b], K, d, s2, tau2, np.float64, expanded=True)["loglik"])
        assert abs(ll - orc.loglik_general(X, y, *orc.unpack_params(rows[b], K, d), s2, 1, tau2)[0]) <= unit   # the scripts' dmnorm
        ratio = abs(ll - ll_ref) / unit
        kappa_max = max(kappa_max, kappa)
        if ratio > worst:
            worst, worst_at = ratio, case
    print("fp64 LAPACK, expanded exponent: largest |ll - ll_ref| / unit %.4g at %s; largest cond1(Sigma) %.3g" % (worst, worst_at, kappa_max))
    want = min(orc.GRAD_TOL_C, 2.0 ** math.ceil(math.log2(32.0 * orc.MARGINAL_LAPACK_MAX)))
    assert orc.MARGINAL_TOL_C == want, (orc.MARGINAL_TOL_C, want)
    # the recorded maximum is this host's LAPACK; another build's must still leave the factor 32 under the same C
    assert 32.0 * worst <= orc.MARGINAL_TOL_C, (worst, worst_at)


def _marginal_ll(Sigma, y):
    """The mode-1 value of a (possibly wrong) Sigma in long double; -inf where it is not positive definite (the device would
    report a failed draw)."""
    LD = np.longdouble
    try:
        Sinv, logdet = orc._chol_inverse(Sigma, LD)
    except np.linalg.LinAlgError:
        return -np.inf
    yv = np.asarray(y, dtype=LD)
    return -(LD(len(yv)) * orc._log_2pi(LD) + logdet + yv @ (Sinv @ yv)) / 2


def _marginal_bugs(X, y, row, K, d, s2, tau2, parts):
    """name -> the Sigma a modelled kernel bug would factorise, built from the long-double reference's pieces."""
    LD = np.longdouble
    n = len(y)
    w, Th = orc.unpack_params(row, K, d)
    sw = (np.asarray(w, dtype=LD) ** 2).sum()
    S0, t2 = parts["Sigma0"], LD(tau2)
    bugs = {}
    if tau2 > 0:
        bugs["tau2 added before the scaling"] = S0 + LD(s2) * sw * t2
        bugs["tau instead of tau^2"] = S0 + np.sqrt(t2)
    bugs["sigma2 without sum w^2"] = S0 / sw + t2
    q = K - 1
    bugs["last weight unsquared"] = S0 + LD(s2) * (LD(w[q]) - LD(w[q]) ** 2) * parts["Rc"][q] + t2
    X0 = np.array(X, dtype=np.float64)
    X0[n - 1] = 0.0
    leak = S0.copy()
    for c in range(K):
        Rc0 = orc.component_corr(X0, Th[c], LD)
        delta = LD(s2) * LD(w[c]) ** 2 * (Rc0[n - 1, :n - 1] - parts["Rc"][c][n - 1, :n - 1])
        leak[n - 1, :n - 1] += delta
        leak[:n - 1, n - 1] += delta
    bugs["padded row leaking into row n - 1"] = leak + t2
    if n > 64:
        hi = min(n, 128)
        if tau2 > 0:
            S = parts["Sigma"].copy()
            S[64:hi, :64] -= t2
            S[:64, 64:hi] -= t2
            bugs["tau2 missing on tile (1, 0)"] = S
        for name, f in (("dropped", 0), ("doubled", 2)):
            S = S0.copy()
            S[64:hi, :64] *= f
            S[:64, 64:hi] *= f
            bugs["tile (1, 0) of Sigma0 %s" % name] = S + t2
            S = S0.copy()
            S[64:hi, 64:hi] *= f
            bugs["tile (1, 1) of Sigma0 %s" % name] = S + t2
    return bugs


def test_marginal_band_rejects_the_kernel_bugs_it_is_meant_to_catch():
    """Each modelled bug, applied to the long-double reference's Sigma, moves the value by at least 4 C units, at every shape
    and pair of the device module's (sigma2, tau2) table (the tile bugs where there is a second 64-row tile: n = 100, 128,
    257; the tau2 bugs where tau2 > 0).  The smallest figure per bug is printed."""
    import test_gpu_marginal_exact as tm
    orc.require_extended_precision()
    least = {}
    for n, d, K in tm.PAIR_SHAPES:
        X, y, rows = tm.make_case(n, d, K)
        for s2, tau2 in tm.PAIRS + [tm.S2_TAU2]:
            parts = orc.marginal_parts(X, y, rows[0], K, d, s2, tau2, np.longdouble)
            unit = orc.marginal_unit(parts, X, rows[0], K, d)
            for name, S in _marginal_bugs(X, y, rows[0], K, d, s2, tau2, parts).items():
                units = abs(float(_marginal_ll(S, y) - parts["loglik"])) / unit
                assert units >= 4.0 * orc.MARGINAL_TOL_C, (name, n, s2, tau2, units)
                if units <= least.get(name, (np.inf,))[0]:
                    least[name] = (units, n, s2, tau2)
    for name in sorted(least):
        print("%-36s at least %.3g units (n = %d, sigma2 = %g, tau2 = %g)" % ((name,) + least[name]))
    assert len(least) == 10
