"""Which tier serves which call (csrc/small_layout.h: small_route), on the device: for every reachable (op, route) cell of
the Gaussian family its witness shape (tests/route_witnesses.py: smallest n, then d, then K; pinned against the CPU check
program by tests/test_small_layout.py) goes through the op's entry point once, with B = 2 draws or designs.  The timing
counters say which tier ran, and the values are held to the oracle at the tolerance of the op's own test:

  loglik          test_gpu_random_shapes.test_likelihood_both_mean_modes
  predict (m = 3) test_gpu_random_shapes.test_prediction_tables
  inverse         test_gpu_gradient_exact.test_explicit_inverse_componentwise (ccgp_logpost with R.Inv: K = 2)
  grad            test_gpu_gradient_exact.check_draw's bands, written without the division (at n = 1 the theta
                  components and their scale are both exactly zero)
  logdet_designs  test_gpu_random_shapes.test_kept_factors_and_design_logdets
  design_grad     test_gpu_design_grad.test_gradient_matches_numpy (n_fixed = 0); its `u` cell is a refusal

Tier: the register-resident and in-LDS evaluators are timed as `fused` and launch nothing of the sweep (`update`, `diag`
== 0); the blocked sweep launches no `fused` kernel, a `diag` launch for its first block column and, from the second
block column on (n > 128), `update` launches.  Four of the blocked witnesses have n <= 128 -- one tile, so no update launch
can exist -- and are held to `diag` instead.  No witness needs more than a few MB of workspace: none was replaced.

The Matern family (n = 14) must take the sweep for the likelihood and for prediction, and a prediction after
ccgp_reserve at the shape where ccgp_reserve's behaviour changed must equal the unreserved one bit for bit."""
import math

import numpy as np
import pytest

import route_witnesses
from oracle import ccgp_oracle as orc
from test_gpu_design_grad import EUNSUPPORTED, _band, _case
from test_gpu_gradient_exact import EPS, INV_C, KAPPA_MAX, _design, _rows, _timed
from test_gpu_random_shapes import draws

pytestmark = pytest.mark.gpu
CELLS = {(op, r): (n, d, K) for op, r, n, d, K in route_witnesses.WITNESSES[0]}


def _cells(op):
    return [pytest.param(r, *CELLS[(o, r)], id="%s-n%d-d%d-K%d" % ((r,) + CELLS[(o, r)])) for (o, r) in CELLS if o == op]


def assert_tier(t, route, n):
    if route in "rl":
        assert t["fused"][1] > 0 and t["update"][1] == 0 and t["diag"][1] == 0 and t["sweep"][1] == 0, t
    else:
        assert t["fused"][1] == 0 and t["diag"][1] > 0, t
        assert n <= 128 or t["update"][1] > 0, t


def test_every_cell_has_its_case():
    ops = {"loglik": "rb", "predict": "rb", "inverse": "rlb", "grad": "rlb", "logdet_designs": "rb", "design_grad": "ru",
           "reserve": "b"}
    assert sorted(CELLS) == sorted((op, r) for op, rs in ops.items() for r in rs)


def check_loglik(X, y, K, P, sigma2, got, R_of):
    ll, beta, st = got
    assert not st.any()
    for b in range(len(P)):
        R = R_of(P[b])
        cond = np.linalg.cond(R)
        w = P[b, :K]
        want_beta = orc.beta_mle(orc.solve_inverse(R), y)
        want_ll = orc.dmnorm_log(y, want_beta, sigma2 * np.sum(w ** 2) * R)
        assert ll[b] == pytest.approx(want_ll, rel=max(1e-10, 50 * cond * EPS)), (b, cond)
        assert beta[b] == pytest.approx(want_beta, rel=max(1e-9, 100 * cond * EPS), abs=1e-9), (b, cond)


def check_predict(X, y, K, P, Xt, sigma2, got, R_of, r_of):
    mean, var, beta, st = got
    assert not st.any() and mean.shape == (len(P), len(Xt)) and var.shape == mean.shape
    for s in range(len(P)):
        R = R_of(P[s])
        cond = np.linalg.cond(R)
        R_inv = orc.solve_inverse(R)
        b_ = orc.beta_mle(R_inv, y)
        mf, v1, v2 = orc.factors(R_inv, b_, y)
        tol = max(1e-8, 200 * cond * EPS)
        assert beta[s] == pytest.approx(b_, rel=tol, abs=1e-9)
        for t in range(len(Xt)):
            want = orc.predict_post_from_factors(r_of(Xt[t], P[s]), b_, mf, v1, v2, R_inv, sigma2)
            assert mean[s, t] == pytest.approx(want[0], rel=tol, abs=tol), (s, t, cond)
            assert var[s, t] == pytest.approx(want[1], rel=10 * tol, abs=10 * tol * sigma2), (s, t, cond)


def _gauss(X, K, d):
    def R_of(row):
        return orc.mixed_corr_matrix_general(X, *orc.unpack_params(row, K, d))

    def r_of(x, row):
        return orc.mixed_corr_vec_general(x, X, *orc.unpack_params(row, K, d))
    return R_of, r_of


@pytest.mark.parametrize("route,n,d,K", _cells("loglik"))
def test_loglik_route(handle, route, n, d, K):
    X, y = _design(n, d, seed=n + d)
    P = draws(np.random.default_rng(n), n, d, K, 2)
    got, t = _timed(handle, lambda: handle.loglik_batch(X, y, K, P, 1.3))
    assert_tier(t, route, n)
    check_loglik(X, y, K, P, 1.3, got, _gauss(X, K, d)[0])


@pytest.mark.parametrize("route,n,d,K", _cells("predict"))
def test_predict_route(handle, route, n, d, K):
    X, y = _design(n, d, seed=n + d)
    rng = np.random.default_rng(n)
    P, Xt = draws(rng, n, d, K, 2), rng.random((3, d))
    got, t = _timed(handle, lambda: handle.predict_batch(X, y, K, P, Xt, 1.3))
    assert_tier(t, route, n)
    check_predict(X, y, K, P, Xt, 1.3, got, *_gauss(X, K, d))


@pytest.mark.parametrize("route,n,d,K", _cells("inverse"))
def test_inverse_route(handle, route, n, d, K):
    from ccgp_amd import api
    assert K == 2
    X, y = _design(n, d, seed=6000 + n)
    rough = 2.0 * n ** (2.0 / d) / d
    p, t1, t2 = 0.7, 0.3 * rough, 1.5 * rough
    R = (p ** 2 * orc.component_corr(X, [t1] * d) + (1 - p) ** 2 * orc.component_corr(X, [t2] * d)) / (p ** 2 + (1 - p) ** 2)
    Rinv_ref = np.asarray(orc.solve_inverse_exact(R), dtype=np.float64)
    assert orc.cond1(R, Rinv_ref) <= KAPPA_MAX
    theta_t = [math.log(t1), math.log(t2), math.log(p / (1 - p))]
    r, t = _timed(handle, lambda: handle.logpost(X, y, 1.3, api.PRIOR_GV, theta_t))
    assert r["status"] == 0
    assert_tier(t, route, n)
    A = np.abs(Rinv_ref)
    assert (np.abs(r["R_inv"] - Rinv_ref) <= INV_C * n * EPS * (A @ np.abs(R) @ A)).all()


@pytest.mark.parametrize("route,n,d,K", _cells("grad"))
def test_grad_route(handle, route, n, d, K):
    X, y = _design(n, d, seed=2000 + n + d)
    rows = _rows(X, K, d, 2, seed=n + d + K)
    (ll, beta, grad, st), t = _timed(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 1.1))
    assert not st.any()
    assert_tier(t, route, n)
    assert route != "b" or t["solve"][1] > 0
    for b in range(2):
        parts = orc.loglik_grad_parts(X, y, rows[b], K, d, 1.1, np.longdouble)
        kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
        assert kappa <= KAPPA_MAX
        g_ref, scale = orc.grad_from_parts(parts, X, rows[b], K, d, 1.1)
        s_ll, s_beta = orc.loglik_beta_scales(parts, y)
        band = orc.GRAD_TOL_C * EPS * kappa * (1.0 + orc.expanded_form_magnitude(X, rows[b], K, d))
        assert (np.abs(grad[b] - g_ref.astype(np.float64)) <= band * scale.astype(np.float64)).all(), (b, kappa)
        assert abs(ll[b] - float(parts["loglik"])) <= band * s_ll and abs(beta[b] - float(parts["beta"])) <= band * s_beta


@pytest.mark.parametrize("route,n,d,K", _cells("logdet_designs"))
def test_logdet_designs_route(handle, route, n, d, K):
    designs = np.stack([_design(n, d, seed=n + i)[0] for i in range(2)])
    row = draws(np.random.default_rng(n), n, d, K, 1)[0]
    (ld, st), t = _timed(handle, lambda: handle.mixed_logdet_designs(designs, K, row))
    assert not np.any(st)
    assert_tier(t, route, n)
    for i in range(2):
        want = np.linalg.slogdet(_gauss(designs[i], K, d)[0](row))[1]
        assert ld[i] == pytest.approx(want, rel=1e-8, abs=1e-7), i


@pytest.mark.parametrize("route,n,d,K", _cells("design_grad"))
def test_design_grad_route(handle, route, n, d, K):
    from ccgp_amd import api
    from design_ref import logdet_grad_general
    rng = np.random.default_rng(n)
    X, row = _case(rng, n, d, K)
    designs = np.stack([X, _case(rng, n, d, K)[0]])
    if route == "u":
        with pytest.raises(api.CcgpError) as e:
            handle.mixed_logdet_grad_designs(designs, K, row, 0)
        assert e.value.code == EUNSUPPORTED
        return
    (ld, g, st), t = _timed(handle, lambda: handle.mixed_logdet_grad_designs(designs, K, row, 0))
    assert not st.any() and g.shape == (2, n, d)
    assert_tier(t, route, n)
    for b in range(2):
        want_ld, want_g = logdet_grad_general(designs[b], K, row, 0)
        band, cond, gen = _band(designs[b], K, row, 0)
        assert abs(ld[b] - want_ld) <= 1e-10 * max(1.0, abs(want_ld)) + 8 * EPS * cond * gen * n
        assert (np.abs(g[b] - want_g) <= band).all()


def test_matern_goes_blocked(handle):
    """n = 14 is a register-evaluator size for the Gaussian family; the Matern family exists on the sweep only.  Setup and
    tolerances of test_gpu_random_shapes.test_matern_family_on_both_paths."""
    from ccgp_amd import api
    n, nu, K = 14, 2.5, 2
    rng = np.random.default_rng(14)
    x = np.sort((np.arange(n) + rng.uniform(0.2, 0.8, n)) / n)[:, None]
    y = np.sin(9.0 * x[:, 0]) + 0.3 * np.cos(31.0 * x[:, 0])
    P = np.column_stack([rng.uniform(0.3, 0.9, 2), rng.uniform(0.1, 0.7, 2), rng.uniform(1.5, 3.0, 2) / n, rng.uniform(0.3, 0.8, 2) / n])
    Xt = rng.random((3, 1))
    try:
        handle.set_kernel(api.KERNEL_MATERN, nu)
        got_ll, t_ll = _timed(handle, lambda: handle.loglik_batch(x, y, K, P, 1.7))
        got_pr, t_pr = _timed(handle, lambda: handle.predict_batch(x, y, K, P, Xt, 1.7))
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    assert_tier(t_ll, "b", n)
    assert_tier(t_pr, "b", n)
    ll, beta, st = got_ll
    mean, var, _, st2 = got_pr
    assert not st.any() and not st2.any()
    for b in range(2):
        w = P[b, :2]
        R = (w[0] ** 2 * orc.corr_matrix_matern(nu, x, P[b, 2]) + w[1] ** 2 * orc.corr_matrix_matern(nu, x, P[b, 3])) / np.sum(w ** 2)
        R_inv = orc.solve_inverse(R)
        b_ = orc.beta_mle(R_inv, y)
        tol = max(1e-9, 100 * np.linalg.cond(R) * EPS)
        assert ll[b] == pytest.approx(orc.dmnorm_log(y, b_, 1.7 * np.sum(w ** 2) * R), rel=tol)
        assert beta[b] == pytest.approx(b_, rel=10 * tol, abs=1e-9)
        mf, v1, v2 = orc.factors(R_inv, b_, y)
        for t in range(3):
            r = (w[0] ** 2 * orc.corr_vec_matern(Xt[t, 0], x, P[b, 2], nu) +
                 w[1] ** 2 * orc.corr_vec_matern(Xt[t, 0], x, P[b, 3], nu)) / np.sum(w ** 2)
            wm, wv = orc.predict_post_from_factors(r, b_, mf, v1, v2, R_inv, 1.7)
            assert mean[b, t] == pytest.approx(wm, rel=10 * tol, abs=10 * tol)
            assert var[b, t] == pytest.approx(wv, rel=100 * tol, abs=100 * tol * 1.7)


def test_reserved_prediction_equals_the_unreserved_one():
    """Gaussian, n <= 128, prediction on the sweep: ccgp_reserve(..., m > 0) now grows the sweep's workspace ahead of the
    call.  Two fresh handles, so that neither finds a workspace an earlier test left."""
    from ccgp_amd import api
    n, d, K = CELLS[("reserve", "b")]
    assert CELLS[("predict", "b")] == (n, d, K) and n <= 128
    X, y = _design(n, d, seed=n + d)
    rng = np.random.default_rng(n)
    P, Xt = draws(rng, n, d, K, 2), rng.random((3, d))
    out = []
    for reserve in (False, True):
        h = api.Handle(0)
        try:
            if reserve:
                h.reserve(n, d, K, 2, 3)
            got, t = _timed(h, lambda: h.predict_batch(X, y, K, P, Xt, 1.3))
        finally:
            h.close()
        assert_tier(t, "b", n)
        assert not got[3].any()
        out.append(got)
    for a, b in zip(*out):
        assert np.array_equal(np.asarray(a).view(np.uint64) if a.dtype == np.float64 else a,
                              np.asarray(b).view(np.uint64) if b.dtype == np.float64 else b)
