"""ccgp_profile_batch -- the likelihood with sigma2 concentrated out, sigma2_hat itself and the gradient at (beta_hat,
sigma2_hat) from one factorisation per draw -- on every device route, and fit.ordinary_kriging_fit on top of it.

Yardstick of the values: the one of tests/test_gpu_gradient_exact.py (check_draw: every gradient component, the
log-likelihood and beta within GRAD_TOL_C eps cond1 (1 + rho) of their cancellation-free sizes), with the long-double
reference and the sizes taken at the long-double sigma2_hat (tests/profile_ref.py).  sigma2_hat is held to
GRAD_TOL_C eps cond1 (1 + rho) sigma2_ref: it is a sum of squares of the same triangular solve whose error the constant
covers, and its relative error enters the gradient through terms no larger than scale[j].

Each case has B = 5 distinct draws whose weights are scaled by 10^(-b / 2), so that sigma2_hat spans four decades inside
one call, a trended y, and a different scale of y per case: a draw that read another draw's sigma2 misses every band.

Bounds that are derived here, not measured:
  * profile value against ccgp_loglik_batch at sigma2 = sigma2_hat: 8 eps (n + |l_p|).  The likelihood forms cs' =
    fl(fl(cs_hat / sw) sw) = cs_hat (1 + 2 u) and n log cs' + q / cs' where the profiled mode has n log cs_hat + n: at most
    (2 + 3) u n before the halving, plus the roundings of the final sums, each of a term no larger than 2 |l_p|; eps = 2 u.
  * Matern value against the host oracle (scipy's K_nu): first-order perturbation of log det R + n log sigma2_hat under a
    relative error delta of every kernel value, delta = 5e-14 + 4 eps z (what csrc/ccgp_internal.h states for matern_corr
    and tests/test_gpu_family_corr_exact.py holds it to) plus GRAD_TOL_C eps cond1 for the factorisation.
"""
import math

import numpy as np
import pytest

import exact_designs as ex
import route_witnesses
import test_gpu_failure_contract as fc
import test_gpu_gradient_exact as gx
from conftest import golden, load_gv, load_hyper, load_qian
from oracle import ccgp_oracle as orc
from profile_ref import NumpyHandle, sigma2_exact

pytestmark = pytest.mark.gpu
EPS = gx.EPS
C = orc.GRAD_TOL_C
B = 5
LDS_WITNESS = next((n, d, K) for op, r, n, d, K in route_witnesses.WITNESSES[0] if (op, r) == ("grad", "l"))
REG = [(2, 1, 1), (5, 4, 2), (17, 9, 1), (50, 9, 1), (64, 8, 8), (65, 4, 3), (128, 9, 4)]
LDS = [LDS_WITNESS]
BLOCKED = [(129, 1, 1), (108, 63, 1), (300, 5, 3)]
CASES = [(c, "reg") for c in REG] + [(c, "lds") for c in LDS] + [(c, "blocked") for c in BLOCKED]
IDS = ["%s-%d-%d-%d" % (r, *c) for c, r in CASES]
ONE_PER_ROUTE = [((17, 9, 1), "reg"), (LDS_WITNESS, "lds"), ((129, 1, 1), "blocked")]
MAX_RATIO = {}
_CASE = {}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _case(shape):
    """(X, y, rows) of a shape, built once: the design and draws of the gradient tests, weights scaled per draw, y per case."""
    if shape not in _CASE:
        n, d, K = shape
        X, y = gx._design(n, d, seed=7000 + 17 * n + d)
        rows = gx._rows(X, K, d, B, seed=n * 64 + d * 8 + K + 1)
        rows[:, :K] *= 10.0 ** (-0.5 * np.arange(B))[:, None]
        idx = [c for c, _ in CASES].index(shape) if shape in [c for c, _ in CASES] else 0
        _CASE[shape] = (X, y * 10.0 ** (idx % 5 - 2), rows)
    return _CASE[shape]


def _route_counters(t, want):
    if want == "blocked":
        assert t["fused"][1] == 0 and t["solve"][1] > 0, t
    else:
        assert t["fused"][1] > 0 and t["solve"][1] == 0, t


def _check_sigma2(X, y, row, K, d, s2_dev, tag):
    """sigma2_hat of one draw against long double; returns the reference (long double) for check_draw."""
    s2_ref, p1 = sigma2_exact(X, y, row, K, d)
    kappa = orc.cond1(p1["Sigma"], p1["Sinv"])
    unit = EPS * kappa * (1.0 + orc.expanded_form_magnitude(X, row, K, d))
    ratio = abs(s2_dev - float(s2_ref)) / (unit * float(s2_ref))
    MAX_RATIO[tag + "-sigma2"] = max(MAX_RATIO.get(tag + "-sigma2", 0.0), ratio)
    print("%s sigma2_hat %.17g ref %.17g ratio %.3g" % (tag, s2_dev, float(s2_ref), ratio))
    assert ratio <= C, (tag, s2_dev, float(s2_ref), ratio, kappa)
    return s2_ref


# ----------------------------------------------------------------------------- 1. exactness on every route
@pytest.mark.parametrize("shape,want", CASES, ids=IDS)
def test_profile_exact_on_every_route(handle, shape, want):
    n, d, K = shape
    assert gx.route(n, d, K) == want
    X, y, rows = _case(shape)
    (ll, s2, beta, grad, st), t = gx._timed(handle, lambda: handle.profile_batch(X, y, K, rows, grad=True))
    _route_counters(t, want)
    assert not st.any() and grad.shape == (B, K + K * d)
    assert s2.max() / s2.min() > 1e3                       # the draws' sigma2 really are decades apart
    for b in range(B):
        s2_ref = _check_sigma2(X, y, rows[b], K, d, s2[b], want)
        gx.check_draw(X, y, rows[b], K, d, s2_ref, (ll[b], beta[b], grad[b]), "profile-" + want)
    MAX_RATIO["%s-grad" % want] = max(MAX_RATIO.get("%s-grad" % want, 0.0), gx.MAX_RATIO["profile-" + want])


def test_value_only_on_the_full_8x8_instance(handle):
    """n = 64 = 8 x 8 with more than 64 draws: the FULL instance of the 8 x 8 grid, four matrices per workgroup (up to 64
    draws the 16 x 16 grid serves the call: checked too, B = 5).  70 draws = the 5 of the case, 14 times over with the
    weights doubled from copy to copy: the normalised matrix keeps its bits, so loglik and beta repeat bit for bit and
    sigma2_hat scales by exactly 1/4 per copy -- in every slot of every workgroup."""
    n, d, K = 64, 4, 2
    X, y = gx._design(n, d, seed=7064)
    rows = gx._rows(X, K, d, B, seed=7064)
    rows[:, :K] *= 10.0 ** (-0.5 * np.arange(B))[:, None]
    big = np.concatenate([rows * np.concatenate([np.full(K, 2.0 ** c), np.ones(K * d)]) for c in range(14)])
    for batch in (rows, big):
        (ll, s2, beta, grad, st), t = gx._timed(handle, lambda: handle.profile_batch(X, y, K, batch, grad=False))
        _route_counters(t, "reg")
        assert grad is None and not st.any()
        for b in range(B):
            s2_ref = _check_sigma2(X, y, rows[b], K, d, s2[b], "value")
            parts = orc.loglik_grad_parts(X, y, rows[b], K, d, s2_ref, np.longdouble)
            unit = EPS * orc.cond1(parts["Sigma"], parts["Sinv"]) * (1.0 + orc.expanded_form_magnitude(X, rows[b], K, d))
            s_ll, s_beta = orc.loglik_beta_scales(parts, y)
            gx.check_loglik_beta(float(parts["loglik"]), float(parts["beta"]), unit * s_ll, unit * s_beta, ll[b], beta[b], "value")
    for c in range(1, 14):
        sl = slice(B * c, B * c + B)
        assert _same((ll[sl], beta[sl], s2[sl] * 4.0 ** c), (ll[:B], beta[:B], s2[:B])), c


# ----------------------------------------------------------------------------- 2. sigma2_hat stays with its draw
@pytest.mark.parametrize("shape,want", CASES, ids=IDS)
def test_a_draw_alone_has_the_bits_it_has_in_the_batch(handle, shape, want):
    n, d, K = shape
    X, y, rows = _case(shape)
    for g in (True, False):
        whole = handle.profile_batch(X, y, K, rows, grad=g)
        for b in range(B):
            alone = handle.profile_batch(X, y, K, rows[b:b + 1], grad=g)
            keep = [k for k in range(5) if whole[k] is not None]
            assert _same([alone[k][0] for k in keep], [whole[k][b] for k in keep]), (g, b)


def test_chunks_and_scheduler_leave_the_bits_alone(handle):
    """n = 300, B = 3.  The workspace limit holds two such matrices: two chunks, the second
    starting at b0 = 2 -- sigma2_hat is written and read at b0 + b.  Then the same call with the sweep as one persistent
    launch (CCGP_OPT_SCHED = 1) against one launch per phase (0)."""
    from ccgp_amd import api
    n, d, K = 300, 5, 3
    X, y, rows = _case((n, d, K))
    rows = rows[[0, 2, 4]]
    for g in (True, False):
        one, t1 = gx._timed(handle, lambda: handle.profile_batch(X, y, K, rows, grad=g))
        # per matrix: 384 columns of 384 + 128 (1 + 3) rows with the identity riding (2.75 MB), of 384 + 128 without (1.6 MB),
        # plus 0.6 MB of diagonal-block inverses and padded inputs: two matrices fit, three do not
        two, t2 = gx._chunked(handle, lambda: handle.profile_batch(X, y, K, rows, grad=g), (8 << 20) if g else (5 << 20))
        assert t2["solve"][1] >= 2 * t1["solve"][1] > 0, (t1, t2)
        keep = [k for k in range(5) if one[k] is not None]
        assert _same([two[k] for k in keep], [one[k] for k in keep]), g
        handle.set_option(api.OPT_SCHED, 0)
        try:
            launches, t0 = gx._timed(handle, lambda: handle.profile_batch(X, y, K, rows, grad=g))
            handle.set_option(api.OPT_SCHED, 1)
            sched, ts = gx._timed(handle, lambda: handle.profile_batch(X, y, K, rows, grad=g))
        finally:
            handle.set_option(api.OPT_SCHED, 3)
        assert t0["sweep"][1] == 0 and ts["sweep"][1] > 0, (t0, ts)
        assert _same([sched[k] for k in keep], [launches[k] for k in keep]), g
        assert _same([launches[k] for k in keep], [one[k] for k in keep]), g


# ----------------------------------------------------------------------------- 3. consistency with the existing entry points
@pytest.mark.parametrize("shape,want", CASES, ids=IDS)
def test_consistent_with_loglik_batch_and_loglik_grad_batch(handle, shape, want):
    n, d, K = shape
    X, y, rows = _case(shape)
    ll, s2, beta, _, st = handle.profile_batch(X, y, K, rows, grad=False)
    assert not st.any()
    for b in range(B):
        ll_b = handle.loglik_batch(X, y, K, rows, s2[b])[0][b]
        bound = 8.0 * EPS * (n + abs(ll[b]))
        print("%s draw %d: l_p %.17g, loglik_batch at sigma2_hat %.17g, |diff| / bound %.3g" % (IDS[CASES.index((shape, want))], b, ll[b], ll_b, abs(ll_b - ll[b]) / bound))
        assert abs(ll_b - ll[b]) <= bound, (b, ll_b, ll[b])
    _, _, beta_g, _, st_g = handle.profile_batch(X, y, K, rows, grad=True)
    _, ref_beta, _, ref_st = handle.loglik_grad_batch(X, y, K, rows, 1.0)
    assert np.array_equal(_bits(beta_g), _bits(ref_beta)) and np.array_equal(st_g, ref_st)


# ----------------------------------------------------------------------------- 4. exact scaling
@pytest.mark.parametrize("shape,want", ONE_PER_ROUTE, ids=["reg", "lds", "blocked"])
def test_scaling_y_by_four_scales_sigma2_by_sixteen_exactly(handle, shape, want):
    n, d, K = shape
    X, y, rows = _case(shape)
    for g in (True, False):
        a = handle.profile_batch(X, y, K, rows, grad=g)
        b = handle.profile_batch(X, 4.0 * y, K, rows, grad=g)
        assert np.array_equal(_bits(b[1]), _bits(16.0 * a[1])) and np.array_equal(_bits(b[2]), _bits(4.0 * a[2])), g


# ----------------------------------------------------------------------------- 5. failure contract
def _profile(h, D, K, g=True):
    def call(rows):
        ll, s2, beta, grad, st = h.profile_batch(D.X, D.y, K, rows, grad=g)
        out = dict(ll=ll, sigma2=s2, beta=beta, status=st)
        if g:
            out["grad"] = grad
        return out
    return call


@pytest.mark.parametrize("n,n_pad,K,want", [(17, 0, 2, "reg"), (97, 52, 8, "lds"), (257, 0, 2, "blocked")],
                         ids=["register", "lds", "blocked"])
def test_failure_contract(handle, n, n_pad, K, want):
    """The exact 0/1 designs and draws that tests/test_gpu_failure_contract.py feeds to ccgp_loglik_grad_batch: the same
    status, NaN in all four outputs of a failed draw, the neighbours' bits as without it, the return value.  Where R = I
    sigma2_hat has a closed form: sum (y - mean y)^2 / (n sum w^2)."""
    D = ex.ExactDesign(n, ex.GRAD_BLOCKED_SEPS if want == "blocked" else (2, n), n_pad)
    assert gx.route(D.n, D.d, K) == want
    rows, exp = D.draws(K, D.mixed())
    D.guard(K, rows)
    out, t = fc._contract(handle, _profile(handle, D, K), rows, exp)
    _route_counters(t, want)
    assert out["grad"].shape == (len(exp), K + K * D.d)
    _, _, _, ref_st = handle.loglik_grad_batch(D.X, D.y, K, rows, 1.3)
    assert np.array_equal(out["status"], ref_st)
    ybar = math.fsum(D.y) / n
    s2 = math.fsum((float(v) - ybar) ** 2 for v in D.y) / (n * K)
    for b in np.nonzero(exp == 0)[0]:
        assert abs(out["sigma2"][b] - s2) <= C * EPS * s2, (b, out["sigma2"][b], s2)
    fc._contract(handle, _profile(handle, D, K, False), rows, exp)     # the value-only call: same contract


@pytest.mark.parametrize("shape,want", ONE_PER_ROUTE, ids=["reg", "lds", "blocked"])
def test_constant_y(handle, shape, want):
    """y = 2 exactly: every operation that carries y' through the elimination scales the row of 1' by a power of two, so
    z_y = 2 z_1 to the bit, beta = 2 and Q = 0 exactly: sigma2_hat = 0, l_p = +Inf, no gradient, and no failure."""
    n, d, K = shape
    X, _, rows = _case(shape)
    for g in (True, False):
        ll, s2, beta, grad, st = handle.profile_batch(X, np.full(n, 2.0), K, rows, grad=g)
        assert not st.any() and (s2 == 0.0).all() and (ll == np.inf).all() and (beta == 2.0).all(), (g, ll, s2, beta, st)
        assert grad is None or np.isnan(grad).all()


def test_matern_value_only_and_gradient_refused(handle):
    from ccgp_amd import api, fit
    nu, n = 2.5, 8
    D = (np.arange(n) + np.array([0.1, 0.4, 0.2, 0.45, 0.05, 0.3, 0.15, 0.35]))[:, None] / n
    y = np.sin(5.0 * D[:, 0]) + 0.3 * D[:, 0]
    thetas = np.array([0.08, 0.15, 0.3])
    got = fit.matern_profile(handle, D, y, nu, thetas)
    assert not got["status"].any()
    for b, th in enumerate(thetas):
        R = orc.corr_matrix_matern(nu, D, th)
        Rinv = np.linalg.inv(R)
        want = orc.log_likeli_1d(nu, th, D, y)
        a = Rinv @ (y - orc.beta_mle(Rinv, y))
        Q = float((y - orc.beta_mle(Rinv, y)) @ a)
        size = float((np.abs(Rinv) * np.abs(R)).sum() + n * (np.abs(a) @ np.abs(R) @ np.abs(a)) / Q)
        z_max = 2.0 * math.sqrt(nu) * float(D.max() - D.min()) / th
        delta = 5e-14 + 4.0 * EPS * z_max + C * EPS * orc.cond1(R, Rinv)
        print("Matern theta %.3g: log.likeli %.15g, oracle %.15g, |diff| / band %.3g" % (th, got["loglikeli"][b], want, abs(got["loglikeli"][b] - want) / (delta * size)))
        assert abs(got["loglikeli"][b] - want) <= delta * size
        assert abs(got["sigma2"][b] - Q / n) <= delta * size / n * (Q / n)
    # bound 3 under the Matern family
    handle.set_kernel(api.KERNEL_MATERN, nu)
    try:
        rows = np.stack([np.ones_like(thetas), thetas], axis=1)
        ll, s2, _, _, _ = handle.profile_batch(D, y, 1, rows, grad=False)
        for b in range(len(thetas)):
            assert abs(handle.loglik_batch(D, y, 1, rows, s2[b])[0][b] - ll[b]) <= 8.0 * EPS * (n + abs(ll[b]))
        with pytest.raises(api.CcgpError) as err:
            handle.profile_batch(D, y, 1, rows, grad=True)
        assert err.value.code == -4      # CCGP_EUNSUPPORTED
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)


# ----------------------------------------------------------------------------- 6. known answer
def test_sigma2_at_the_recovered_mlegp_theta(handle):
    fx = golden("gv_mlegp_recovered.json")
    D, y, _, _ = load_gv(50)
    for g in (True, False):
        _, s2, beta, _, st = handle.profile_batch(D, y, 1, np.concatenate([[1.0], fx["theta"]])[None], grad=g)
        print("sigma2_hat %.15g, recorded %.15g, relative difference %.3g" % (s2[0], fx["sigma2"], abs(s2[0] - fx["sigma2"]) / fx["sigma2"]))
        assert st[0] == 0 and abs(s2[0] - fx["sigma2"]) <= 1e-10 * fx["sigma2"]


# ----------------------------------------------------------------------------- 7. the fit
class _Counting:
    """The handle with its profile_batch calls and the points they carried counted."""

    def __init__(self, h):
        self.h, self.calls, self.points = h, 0, 0

    def profile_batch(self, X, y, K, params, grad=False):
        self.calls += 1
        self.points += np.atleast_2d(params).shape[0]
        return self.h.profile_batch(X, y, K, params, grad=grad)


def test_fit_on_qian(handle):
    from ccgp_amd import fit
    D, y, _, _ = load_qian()
    cpu = fit.ordinary_kriging_fit(NumpyHandle(), D, y, starts=8, rng=0)
    ch = _Counting(handle)
    r = fit.ordinary_kriging_fit(ch, D, y, starts=8, rng=0)
    print("Qian: %d profile_batch calls carrying %d points, best log-likelihood %.6f (host %.6f), sigma2 %.4f, per start %s" % (
        r["calls"], r["evaluations"], r["loglik"], cpu["loglik"], r["sigma2"], np.round(-r["f"], 4).tolist()))
    assert abs(r["loglik"] - cpu["loglik"]) <= 1e-3
    assert 57.5 <= r["sigma2"] <= 66.75
    assert ch.calls == r["calls"] and ch.points == r["evaluations"] and 2 * r["calls"] < r["evaluations"]
    H = load_hyper("hx")
    target = int(np.where((H == np.array([7.0, 3.0, 3.0, 28.0])).all(axis=1))[0][0])
    _, arg = handle.grid_marginal(D, y, r["sigma2"], H, 1000, 50.0, True)
    assert arg == target == 292


def test_fit_on_ground_vibrations_from_the_mlegp_theta(handle):
    from ccgp_amd import fit
    fx = golden("gv_mlegp_recovered.json")
    D, y, _, _ = load_gv(50)
    ll0 = handle.profile_batch(D, y, 1, np.concatenate([[1.0], fx["theta"]])[None], grad=True)[0][0]
    ch = _Counting(handle)
    r = fit.ordinary_kriging_fit(ch, D, y, starts=8, rng=0, extra_starts=[fx["theta"]])
    print("GV: %d profile_batch calls carrying %d points, best log-likelihood %.6f, at the mlegp theta %.6f, from it %.6f, sigma2 %.4f" % (
        r["calls"], r["evaluations"], r["loglik"], ll0, -r["f"][8], r["sigma2"]))
    assert r["f"].shape == (9,) and -r["f"][8] >= ll0
    assert r["loglik"] > ll0 + 1.0
    assert ch.calls == r["calls"] and ch.points == r["evaluations"] and 2 * r["calls"] < r["evaluations"]


def test_zz_report_headroom():
    for k in sorted(MAX_RATIO):
        print("profile max ratio %-16s %.3g" % (k, MAX_RATIO[k]))
