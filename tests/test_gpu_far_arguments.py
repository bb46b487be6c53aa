"""Every Gaussian route at arguments beyond exp's range, held to base R's exp(-x) = 0.

Fixtures (tests/exact_designs.py): the identity lattices at component rates (2^k, 2^(k+1)), k in FAR_K = (95, 140, 200, 260, 1000);
the two-scale mix (component 0 far, component 1 at the dyadic rate 2^-4: R = (I + R2) / 2); a far test site on a valid factor.
Every far rate makes the bands of the exact modules vacuous (their rho is the size of the expanded exponent's terms, ~2^k), so
no new tolerance exists here:
  equality    a call at a far magnitude returns what the same call returns with 2048 / 4096 in its place: outputs, status and
              return value, by np.testing.assert_array_equal (value equality with NaN positions; the sign of an exact zero is
              not pinned);
  closed form on the identity lattices the 2048 result is also held to exact_designs.identity_closed_forms;
  reference   on the two-scale mix the 2048 result is held, once per route, to that operation's long-double reference within
              its module's own band and constant, with rho = 0 (both components' exponents are exact);
  raw entries are held to the fp64 oracle's entries, NaN positions included: exactly 0 off the diagonal and 1 on it.
tests/test_far_arguments_host.py shows without a GPU that the fixtures are exact, that the oracle and the CPU evaluator meet
the equality, and that the assertion rejects both device routines as they were before the range select.

What is strict (include/ccgp.h, "Domain of the rates"): the raw entry points, everything on the blocked sweep and cov_kernel,
and every cross-correlation vector on every route, at every magnitude.  The matrix generation loops of the small-n evaluators
(small_reg.hip, small.hip) keep the unselected polynomial exp -- the select there was measured and rejected
(profiles/exp_poly_range_select.md); only the extra-row prediction instances of small_reg.hip, which that measurement never
ran, select, and are strict throughout -- so the routes marked `hot` are strict up to k = 140, and at k >= 200 each row is EITHER
equal to the 2048 row OR a failed row under the failure contract: status a pivot index, every output NaN, the return value
counting it (its neighbours are then rows of one of the two kinds themselves).  Never a finite wrong value, never a
non-finite value with status 0.  test_zz_report prints which of the two each such route gave.

Shapes: one, the smallest, witness per route (tests/route_witnesses.py, tests/test_gpu_failure_contract.py), m <= 5, and B <= 9
(the mixed batch of a three-separator lattice) except where the route itself needs more than 64 draws (the one-wave-per-matrix
forms) or 32 (the scheduled sweep).
csrc/small.hip serves gradients only (no likelihood or prediction shape reaches it: route_witnesses has no such cell), so its
witness appears under the gradient.
"""
import numpy as np
import pytest

import design_exact as dx
import exact_designs as ex
import krige_ref as kr
import loo_ref as lr
from oracle import ccgp_oracle as orc
from test_gpu_failure_contract import (S2, WITNESS, _blocked, _call, _identity_loglik, _identity_predict, _option, _repeat,
                                       _Returned, _small, sites_supported)
from test_gpu_gradient_exact import route, scheduled

pytestmark = pytest.mark.gpu
EPS = ex.EPS
KAPPA_MAX = 1e8
STRICT_HOT_K = 140                 # the last magnitude at which the unselected polynomial exp is still right
OUTCOMES = {}                      # (route, k) -> "equal" | "failed rows [...]" for the hot routes at k >= 200


# ----------------------------------------------------------------------------- the two assertions
def _same(got, rc, base, rc0, what):
    assert sorted(got) == sorted(base), what
    for name in sorted(base):
        np.testing.assert_array_equal(np.asarray(got[name]), np.asarray(base[name]), err_msg="%s: %s" % (what, name))
    assert rc == rc0, (what, rc, rc0)


def _equal_or_failed(got, rc, base, rc0, n, what):
    """Each row is the 2048 row or a failed row; returns the failed rows."""
    st = np.asarray(got["status"])
    failed = []
    for b in range(st.size):
        if all(np.array_equal(np.asarray(got[k])[b], np.asarray(base[k])[b], equal_nan=True) for k in base):
            continue
        assert 1 <= st[b] <= n, "%s: row %d differs from the 2048 row with status %d" % (what, b, st[b])
        for k in base:
            if not k.startswith("status"):
                assert np.isnan(np.asarray(got[k], dtype=np.float64)[b]).all(), "%s: failed row %d holds a number in %s" % (what, b, k)
        failed.append(b)
    if rc0 is not None:
        assert rc == int(np.count_nonzero(st)), (what, rc, st.tolist())
    return failed


def _far(run, n, hot, what, magnitudes=None):
    """run(theta) -> (outputs, C return value or None).  Returns the 2048 result."""
    base, rc0 = run(ex.THETA)
    for k, theta in magnitudes or list(zip(ex.FAR_K, ex.FAR)):
        got, rc = run(theta)
        if hot and k > STRICT_HOT_K:
            failed = _equal_or_failed(got, rc, base, rc0, n, "%s k=%d" % (what, k))
            OUTCOMES[(what, k)] = "%d of %d rows failed, the others equal" % (len(failed), np.asarray(got["status"]).size) if failed else "equal"
        else:
            _same(got, rc, base, rc0, "%s k=%d" % (what, k))
    return base


def _lattice(h, D, K, zs, fn, tier, hot, what):
    """fn(rows) -> outputs on the identity lattice D with the separator subsets zs; the 2048 result has the derived status."""
    def run(theta):
        rows, _ = D.draws(K, zs, theta)
        out, rc, t = _call(h, lambda: fn(rows))
        tier(t)
        return out, rc
    exp = D.draws(K, zs)[1]
    base = _far(run, D.n, hot, what)
    assert np.array_equal(base["status"], exp), (what, base["status"], exp)
    return base, exp


def _any(t):
    pass


# ----------------------------------------------------------------------------- raw entry points
def _raw_blocks(h, X, Xt, K, row):
    d = X.shape[1]
    w, Th = orc.unpack_params(row, K, d)
    with np.errstate(over="ignore", invalid="ignore"):
        want = [orc.corr_matrix(X, Th[0]), np.stack([orc.corr_vec(x, X, Th[0]) for x in Xt]),
                orc.mixed_corr_matrix_general(X, w, Th), np.stack([orc.mixed_corr_vec_general(x, X, w, Th) for x in Xt])]
    got = [h.corr_matrix(X, Th[0]), h.corr_cross(Xt, X, Th[0]), h.mixed_corr_matrix(X, K, row), h.mixed_corr_cross(Xt, X, K, row)]
    return got, want


@pytest.mark.parametrize("n", [5, 130])
def test_raw_entry_points_on_the_identity_lattice(handle, n):
    """n = 130: a tile edge of cov_kernel (64 x 64 tiles).  Entries: the fp64 oracle's, exactly 0 / 1."""
    D = ex.ExactDesign(n, (2, n))
    Xt, on = D.sites(5, 4)
    for theta in [ex.THETA] + ex.FAR:
        for zero in ((), (0,), (1, 0)):
            got, want = _raw_blocks(handle, D.X, Xt, 2, D.row(2, zero, theta))
            for g, w, name in zip(got, want, ("corr_matrix", "corr_cross", "mixed_corr_matrix", "mixed_corr_cross")):
                assert np.isin(w, (0.0, 1.0)).all()
                np.testing.assert_array_equal(np.asarray(g), w, err_msg="%s n=%d theta=%g zero=%s" % (name, n, theta[0], zero))
            assert (np.diag(got[0]) == 1.0).all() and (np.asarray(got[1])[np.nonzero(on >= 0)[0], on[on >= 0]] == 1.0).all()


@pytest.mark.parametrize("n", [5, 130])
def test_raw_entry_points_on_the_two_scale_mix(handle, n):
    """(I + R2) / 2 at every magnitude: the 2048 blocks within tests/gauss_exact.py's band of its 40-digit reference (exact
    distances: delta_c = 0), every far block equal to them; the far component alone is the oracle's 0 / 1 block."""
    import gauss_exact as gx
    T = ex.TwoScaleDesign(n)
    Xt, _ = T.sites(5)
    got0, want0 = _raw_blocks(handle, T.X, Xt, 2, T.row())
    w, Th = orc.unpack_params(T.row(), 2, T.d)
    for g, Xnew in ((got0[2], None), (got0[3], Xt)):
        ref = gx.Case("far", "two-scale-%d" % n, w, Th, Xnew, T.X, exact_distance=True).reference()
        worst, bad = gx.worst_ratio(np.asarray(g), ref)
        print("two-scale raw n=%d %s: largest |d| / band %.3g" % (n, "matrix" if Xnew is None else "cross", worst))
        assert not bad, bad[:6]
    for a, _ in ex.FAR:
        got, want = _raw_blocks(handle, T.X, Xt, 2, T.row(a))
        for j in (0, 1):
            assert np.isin(want[j], (0.0, 1.0)).all()
            np.testing.assert_array_equal(np.asarray(got[j]), want[j], err_msg="two-scale far component n=%d a=%g" % (n, a))
        for j in (2, 3):
            np.testing.assert_array_equal(want[j], want0[j])
            np.testing.assert_array_equal(np.asarray(got[j]), np.asarray(got0[j]), err_msg="two-scale mix n=%d a=%g" % (n, a))


def test_raw_cross_entry_points_at_an_argument_of_exactly_infinity(handle):
    """d = 1 (in d >= 2 the scripts' X^2 %*% Theta forms Inf * 0 = NaN itself).  Coordinate 1e160 at rate 1e100: x theta = 1e260 is
    finite, u = x^2 theta overflows.  A site at the origin against that row: (0 - 2 * 0) + Inf = Inf and R gives exp(-Inf) = 0; a
    site whose own u overflows too: Inf - Inf = NaN in R."""
    X = np.array([[0.0], [1.0], [1e160], [3.0]])
    Xt = np.array([[0.0], [1e160], [1.0]])
    row = np.array([1.0, 1.0, 1e100, 2e100])
    got, want = _raw_blocks(handle, X, Xt, 2, row)
    for j in (1, 3):
        assert want[j][0, 2] == 0.0 and np.isnan(want[j][1, 2]) and want[j][1, 0] == 0.0
        assert want[j][0, 0] == 1.0 and want[j][2, 1] == 1.0 and want[j][0, 1] == 0.0 and want[j][2, 2] == 0.0
        np.testing.assert_array_equal(np.asarray(got[j]), want[j])


@pytest.mark.parametrize("z", [1e5, 1e20, 1e150, 1e300])
@pytest.mark.parametrize("family,nu", [(1, 1.5), (1, 5.0), (2, 1.5), (2, 5.0)], ids=["matern1.5", "matern5", "spline1.5", "spline5"])
def test_families_are_exactly_zero_far_out(handle, family, nu, z):
    """z = 2 sqrt(nu) |h| / theta: z^nu K_nu(z) / (Gamma(nu) 2^(nu - 1)) underflows beyond z ~ 750 + nu log z, and the spline is 0
    beyond |h| / theta = 1 (tests/family_exact.py at 40 digits says the same): every off-diagonal entry exactly 0, the
    diagonal exactly 1, nothing NaN.  The kernels form z^2 = rate h^2, which overflows at z = 1e300; the spacing is then 1e200
    and theta = 2 sqrt(nu) 1e-100 so that the rate itself stays finite."""
    from ccgp_amd import api
    h0 = 1e200 if z > 1e154 else 1.0
    theta = 2.0 * np.sqrt(nu) * h0 / z
    X = (h0 * np.arange(5.0))[:, None]
    Xt = (h0 * np.array([-1.0, 2.0, 7.5]))[:, None]
    row = np.array([0.5, 0.5, theta, theta / 3.0])
    try:
        handle.set_kernel(api.KERNEL_MATERN if family == 1 else api.KERNEL_MATERN_SPLINE, nu)
        blocks = [handle.mixed_corr_matrix(X, 2, row), handle.mixed_corr_cross(Xt, X, 2, row)]
        if family == 1:           # the two-family pair exists for K = 2 only
            blocks += [handle.corr_matrix(X, [theta]), handle.corr_cross(Xt, X, [theta])]
        dth = [handle.family_corr_dtheta(X[:, 0], 2, row, q) for q in (0, 1)]     # d R_q / d theta_q: matern_corr_grad, the spline's
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    on = np.zeros((3, 5), dtype=bool)
    on[1, 2] = True
    for g, where in zip(blocks, (np.eye(5, dtype=bool), on) * 2):
        g = np.asarray(g)
        assert not np.isnan(g).any(), (family, nu, z, g)
        assert (g[~where] == 0.0).all(), (family, nu, z, g)
        # coincident points: 1, or sum w^2 = 1/2 where the two-family script leaves the mix un-normalised (D1F:479)
        assert np.isin(g[where], (1.0, 0.5)).all() and np.unique(g[where]).size == 1, (family, nu, z, g)
    for g in dth:                 # the derivative underflows with the value: exactly 0 everywhere, the diagonal included
        assert not np.asarray(g).any() and not np.isnan(np.asarray(g)).any(), (family, nu, z, g)


# ----------------------------------------------------------------------------- likelihood
def _ll(h, D, K, mode):
    def fn(rows):
        ll, beta, st = h.loglik_batch(D.X, D.y, K, rows, S2[mode], mode, 0.0)
        return dict(ll=ll, beta=beta, status=st)
    return fn


def _loglik_route(h, n, seps, mode, tier, hot, what, many=False):
    D = ex.ExactDesign(n, seps)
    zs = _repeat(D.mixed(), 64) if many else D.mixed()
    assert (len(zs) > 64) == many and (many or len(zs) <= 9)
    base, exp = _lattice(h, D, 2, zs, _ll(h, D, 2, mode), tier, hot, what)
    _identity_loglik(base, exp, D, 2, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_register_tier_8x8(handle, mode):
    _loglik_route(handle, 9, ex.LOGLIK_REG8[9], mode, _small, True, "loglik reg8 mode %d" % mode, many=True)


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_four_waves_per_matrix(handle, mode):
    _loglik_route(handle, 9, ex.LOGLIK_REG8[9], mode, _small, True, "loglik wide mode %d" % mode)


@pytest.mark.parametrize("grid16", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_one_wave_per_matrix(handle, mode, grid16):
    from ccgp_amd import api
    with _option(handle, api.OPT_SMALL_GRID16, grid16, 0):
        _loglik_route(handle, 65, ex.LOGLIK_WAVE[65], mode, _small, True, "loglik wave grid16=%d mode %d" % (grid16, mode), many=True)


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_register_tier_16x16(handle, mode):
    _loglik_route(handle, 105, ex.LOGLIK_REG16[105], mode, _small, True, "loglik reg16 mode %d" % mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_blocked_launches(handle, mode):
    assert WITNESS[("loglik", "b")][0] == 129
    _loglik_route(handle, 129, ex.LOGLIK_BLOCKED[129], mode, lambda t: _blocked(t, 129), False, "loglik blocked mode %d" % mode)


FORCED_SWEEP_N, FORCED_SWEEP_SEPS = 385, (2, 129, 385)          # 4 x 4 tiles of 128; pivots in the first, second and last tile


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_forced_scheduled_sweep(handle, mode, sched):
    """CCGP_OPT_SCHED = 1 and 2 force the persistent sweep at n = 385 (tests/test_gpu_marginal_exact.py): eight draws, every
    magnitude of FAR, strict."""
    from ccgp_amd import api
    D = ex.ExactDesign(FORCED_SWEEP_N, FORCED_SWEEP_SEPS)
    zs = D.mixed()[:8]
    assert any(len(z) == 0 for z in zs) and {j for z in zs for j in z} == {0, 1, 2}

    def tier(t):
        assert t["sweep"][1] > 0 and t["fused"][1] == 0, t
    with _option(handle, api.OPT_SCHED, sched, 3):
        base, exp = _lattice(handle, D, 2, zs, _ll(handle, D, 2, mode), tier, False, "loglik forced sweep %d mode %d" % (sched, mode))
    _identity_loglik(base, exp, D, 2, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_scheduled_sweep(handle, mode):
    """n = 2048, B = 32: the smallest shape the persistent sweep takes at the default CCGP_OPT_SCHED; every magnitude of FAR."""
    n, B = ex.SCHED_N, ex.SCHED_B
    assert scheduled(n, B)
    D = ex.ExactDesign(n, ex.SCHED_SEPS)

    def tier(t):
        assert t["sweep"][1] > 0 and t["fused"][1] == 0, t
    base, exp = _lattice(handle, D, 2, ex.SCHED_ZERO, _ll(handle, D, 2, mode), tier, False, "loglik sweep mode %d" % mode)
    _identity_loglik(base, exp, D, 2, mode)


def _hypercube(d=4):
    """The points of {0, 1}^d with at most two ones: u_i is 0, theta or 2 theta and x_i' Theta x_i the same sum, so the diagonal's
    expanded exponent is exactly 0 for ANY rate -- ccgp_logpost_batch forms theta = exp(psi), which need not be a power of
    two -- and distinct points are at least theta (1 - 8 eps) apart."""
    pts = [np.zeros(d)]
    for a in range(d):
        e = np.zeros(d)
        e[a] = 1.0
        pts.append(e)
        for b in range(a):
            f = e.copy()
            f[b] = 1.0
            pts.append(f)
    X = np.stack(pts)
    return X, np.sin(0.7 * np.arange(len(X))) + 0.5


def test_logpost_batch(handle):
    """theta_t = (log theta1, log theta2, logit p) with p = 1/2 (weights 1/2, 1/2): the log-likelihood, beta and status of
    every far row equal the rates-of-2048 row's; val carries the prior and the Jacobian of its own theta_t and is not compared."""
    from ccgp_amd import api
    X, y = _hypercube()

    def run(theta):
        tt = np.array([[np.log(theta[0]), np.log(theta[1]), 0.0]] * 3)
        (val, beta, ll, st), rc, t = _call(handle, lambda: handle.logpost_batch(X, y, 1.3, api.PRIOR_INVGAMMA, tt, [7.0, 3.0, 3.0, 28.0]))
        _small(t)
        return dict(ll=ll, beta=beta, status=st), rc
    base = _far(run, len(X), True, "logpost_batch")
    assert not base["status"].any() and np.isfinite(base["ll"]).all()
    c = 1.3 * 0.5
    assert abs(base["beta"][0] - y.mean()) <= 16 * EPS * np.abs(y).mean()
    want = -(len(y) * np.log(2.0 * np.pi * c) + ((y - y.mean()) ** 2).sum() / c) / 2.0
    assert abs(base["ll"][0] - want) <= orc.GRAD_TOL_C * EPS * (len(y) + ((y - y.mean()) ** 2).sum() / c)


def _two_sets(D):
    return np.stack([D.X, D.X]), np.stack([D.y, 1.0 - 2.0 * D.y])


def test_loglik_batch_sets(handle):
    D = ex.ExactDesign(9, ex.LOGLIK_REG8[9])
    Xs, ys = _two_sets(D)
    zs = D.mixed()
    set_of = np.arange(len(zs)) % 2

    def fn(rows):
        ll, beta, st = handle.loglik_batch_sets(Xs, ys, [1.3, 1.3], 2, rows, set_of[:len(rows)])
        return dict(ll=ll, beta=beta, status=st)
    base, exp = _lattice(handle, D, 2, zs, fn, _small, True, "loglik_batch_sets")
    one = _ll(handle, D, 2, 0)(D.draws(2, zs)[0])
    even = set_of == 0
    np.testing.assert_array_equal(base["ll"][even], one["ll"][even])


def test_profile_batch_sets(handle):
    D = ex.ExactDesign(9, ex.LOGLIK_REG8[9])
    Xs, ys = _two_sets(D)
    zs = D.mixed()
    set_of = np.arange(len(zs)) % 2

    def fn(rows):
        ll, s2, beta, g, st = handle.profile_batch_sets(Xs, ys, 2, rows, set_of[:len(rows)], grad=True)
        return dict(ll=ll, s2=s2, beta=beta, grad=g, status=st)
    base, exp = _lattice(handle, D, 2, zs, fn, _any, True, "profile_batch_sets")
    ok = exp == 0
    assert not base["grad"][ok][:, 2:].any()                 # R_c = I: every rate derivative is exactly 0


# ----------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("n,n_pad,K,want", [(17, 0, 2, "reg"), (97, 52, 8, "lds"), (108, 59, 1, "blocked")],
                         ids=["register", "lds", "blocked"])
def test_gradient(handle, n, n_pad, K, want):
    """The witnesses of tests/route_witnesses.py: the far components' rate derivatives are exactly 0 (R_c = I)."""
    D = ex.ExactDesign(n, (2, n), n_pad)
    assert route(D.n, D.d, K) == want
    if want != "reg":
        assert WITNESS[("grad", "l" if want == "lds" else "b")] == (D.n, D.d, K)

    def fn(rows):
        ll, beta, grad, st = handle.loglik_grad_batch(D.X, D.y, K, rows, 1.3)
        return dict(ll=ll, beta=beta, grad=grad, status=st)
    tier = (lambda t: _blocked(t, n)) if want == "blocked" else _small
    base, exp = _lattice(handle, D, K, D.mixed(), fn, tier, want != "blocked", "gradient " + want)
    ll, beta, b_ll, b_beta = ex.identity_closed_forms(D.y, 1.3, K, 0)
    for b in np.nonzero(exp == 0)[0]:
        assert abs(base["ll"][b] - ll) <= b_ll and abs(base["beta"][b] - beta) <= b_beta
        assert not base["grad"][b, K:].any(), base["grad"][b, K:]


# ----------------------------------------------------------------------------- prediction
def _pred(h, D, K, Xt, s2=1.3):
    def fn(rows):
        mean, var, beta, st = h.predict_batch(D.X, D.y, K, rows, Xt, s2)
        return dict(mean=mean, var=var, beta=beta, status=st)
    return fn


def _predict_route(h, D, K, tier, hot, what):
    Xt, on = D.sites(5, 4)
    base, exp = _lattice(h, D, K, D.mixed(), _pred(h, D, K, Xt), tier, hot, what)
    _identity_predict(base, exp, D, on, K, 1.3)


@pytest.mark.parametrize("n", [9, 104])
def test_predict_kept_factor_scheme(handle, n):
    D = ex.ExactDesign(n, ex.predict_seps(n))
    assert sites_supported(D.n, D.d, 2)
    _predict_route(handle, D, 2, _small, True, "predict kept n=%d" % n)


def test_predict_extra_row_scheme(handle):
    """n = 128 is outside the kept-factor scheme (n <= 104): the sites ride through the register-resident elimination.  Its 12 x 11
    lattice has exponents up to 221 * 2^141 at k = 140, beyond the domain of the unselected polynomial exp (include/ccgp.h:
    exponents below 2^148.47), so these instances take their matrix entries through the range select and are strict at EVERY
    magnitude, like their cross vectors."""
    D = ex.ExactDesign(128, ex.predict_seps(128))
    assert not sites_supported(D.n, D.d, 2)
    _predict_route(handle, D, 2, _small, False, "predict extra rows n=128")


def test_predict_extra_row_scheme_by_option(handle):
    from ccgp_amd import api
    D = ex.ExactDesign(9, ex.predict_seps(9))
    with _option(handle, api.OPT_PREDICT_FACTOR, 0, 1):
        _predict_route(handle, D, 2, _small, False, "predict extra rows n=9")


def test_predict_blocked_below_129(handle):
    n, d, K = WITNESS[("predict", "b")]
    D = ex.ExactDesign(n, (2, n), d - 4)
    assert (D.n, D.d, K) == (108, 63, 1)
    _predict_route(handle, D, K, lambda t: _blocked(t, n), False, "predict blocked n=108")


def test_predict_blocked(handle):
    D = ex.ExactDesign(129, ex.predict_seps(129))
    _predict_route(handle, D, 2, lambda t: _blocked(t, 129), False, "predict blocked n=129")


@pytest.mark.parametrize("n", [9, 129])
def test_factor_set(handle, n):
    from ccgp_amd import api
    D = ex.ExactDesign(n, ex.predict_seps(n))
    Xt, on = D.sites(5, 4)
    zs = D.mixed()

    def run(theta):
        rows, _ = D.draws(2, zs, theta)
        with _Returned(handle, 2) as ret:
            fs = handle.factor_batch(D.X, D.y, 2, rows, 1.3)
            mean, var = fs.predict(Xt)
        out = dict(ll=fs.loglik, beta=fs.beta, mean=mean, var=var, status=fs.status)
        assert api.lib().ccgp_factorset_free(handle._h, fs._fs) == 0
        fs._fs = None
        return out, ret.rcs[0]
    base = _far(run, n, n <= 128, "factor set n=%d" % n)
    exp = D.draws(2, zs)[1]
    assert np.array_equal(base["status"], exp)
    _identity_predict(base, exp, D, on, 2, 1.3)


@pytest.mark.parametrize("n", [9, 130])
def test_literal_predict_post(handle, n):
    """ccgp_predict_post: Mixed.corr.vec on the device, then the quadratic forms with the caller's cached terms (R = I: R.Inv = I,
    beta = mean(y)); no status, no elimination: strict at every magnitude."""
    D = ex.ExactDesign(n, (2, n))
    Xt, on = D.sites(5, 4)
    beta = float(np.mean(D.y))
    mf, v1, v2 = orc.factors(np.eye(n), beta, D.y)

    def run(theta):
        mean, var = handle.predict_post(Xt, D.X, 2, D.row(2, (), theta), beta, mf, v1, v2, np.eye(n), 1.3)
        return dict(mean=mean, var=var, status=np.zeros(1, dtype=np.int32)), None
    base = _far(run, n, False, "predict_post n=%d" % n)
    for t in range(5):
        want = orc.predict_post_from_factors(np.eye(n)[on[t]] if on[t] >= 0 else np.zeros(n), beta, mf, v1, v2, np.eye(n), 1.3)
        assert abs(base["mean"][t] - want[0]) <= 8 * EPS * (abs(beta) + np.abs(D.y).max())
        assert abs(base["var"][t] - want[1]) <= 8 * EPS * 1.3 * 2.0


@pytest.mark.parametrize("n", [9, 129])
def test_predict_summary(handle, n):
    D = ex.ExactDesign(n, ex.predict_seps(n))
    Xt, _ = D.sites(5, 4)
    keys = ("y_hat", "pred_var", "quant", "cdf_at", "quantiles")

    def run(theta):
        rows, _ = D.draws(2, D.mixed(), theta)
        got = handle.predict_summary(D.X, D.y, 2, rows, Xt, 1.3, [0.025, 0.975], np.linspace(-1.0, 2.0, 5))
        out = dict(beta=got["beta"], status=got["status"])
        return (out, got["n_failed"]), np.column_stack([np.asarray(got[k]).reshape(5, -1) for k in keys])
    (base, rc0), table0 = run(ex.THETA)
    exp = D.draws(2, D.mixed())[1]
    assert np.array_equal(base["status"], exp) and rc0 == np.count_nonzero(exp) and not np.isnan(table0).any()
    for k, theta in zip(ex.FAR_K, ex.FAR):
        (got, rc), table = run(theta)
        what = "predict_summary n=%d k=%d" % (n, k)
        if n <= 128 and k > STRICT_HOT_K:
            failed = _equal_or_failed(got, rc, base, rc0, n, what)
            OUTCOMES[("predict_summary n=%d" % n, k)] = "failed rows %s" % failed if failed else "equal"
            if not failed:
                np.testing.assert_array_equal(table, table0, err_msg=what)
            else:           # the summary leaves the failed draws out: finite, or NaN throughout when none is left
                assert np.isfinite(table).all() or np.isnan(table).all(), what
        else:
            _same(got, rc, base, rc0, what)
            np.testing.assert_array_equal(table, table0, err_msg=what)


def test_predict_batch_sets(handle):
    D = ex.ExactDesign(9, ex.predict_seps(9))
    Xs, ys = _two_sets(D)
    Xt, on = D.sites(5, 4)
    zs = D.mixed()
    set_of = np.arange(len(zs)) % 2

    def fn(rows):
        mean, var, beta, st = handle.predict_batch_sets(Xs, ys, [1.3, 1.3], 2, rows, set_of[:len(rows)], np.stack([Xt, Xt]))
        return dict(mean=mean, var=var, beta=beta, status=st)
    base, exp = _lattice(handle, D, 2, zs, fn, _any, True, "predict_batch_sets")
    one = _pred(handle, D, 2, Xt)(D.draws(2, zs)[0])
    even = set_of == 0
    np.testing.assert_array_equal(base["mean"][even], one["mean"][even])
    np.testing.assert_array_equal(base["var"][even], one["var"][even])


# ----------------------------------------------------------------------------- a far site on a valid factor
@pytest.mark.parametrize("scheme,n,d", [("kept", 9, 1), ("extra", 9, 1), ("sweep", 108, 63)])
def test_far_site_on_a_valid_factor(handle, scheme, n, d):
    """The training matrix exp(-s (i - j)^2) is the same well-conditioned matrix at every k and lies inside every exp's range; only the
    cross vector sees an argument >= 2^k.  A cross vector passes no pivot test, so this is STRICT on every scheme: status 0, the
    rates-of-2048 design's mean and variance to the value, mean = beta and var = sigma2 (1 + 1 / 1'R^-1 1) within the band of
    tests/test_gpu_predict_exact.py (rho = 0: exact exponents; r = 0).  kept: site_corr_kernel; extra: the extra rows of
    small_reg_kernel (CCGP_OPT_PREDICT_FACTOR = 0); sweep: the n = 108 witness, whose prediction rides the blocked sweep."""
    from ccgp_amd import api
    m, s2 = 3, 1.3

    def run(D):
        with _option(handle, api.OPT_PREDICT_FACTOR, 0 if scheme == "extra" else 1, 1):
            (mean, var, beta, st), rc, t = _call(handle, lambda: handle.predict_batch(D.X, D.y, 1, D.row()[None], D.sites(m), s2))
        (_small if scheme != "sweep" else (lambda t: _blocked(t, n)))(t)
        return dict(mean=mean, var=var, beta=beta, status=st), rc
    if scheme == "kept":
        assert sites_supported(n, d, 1)
    for ks in ([k for k in ex.FAR_K if k % 2], [k for k in ex.FAR_K if k % 2 == 0]):
        S = ex.FarSiteDesign(n, ks[0], d).stand_in()
        assert S.guard() <= KAPPA_MAX
        base, rc0 = run(S)
        assert rc0 == 0 and not base["status"].any()
        parts = orc.predict_parts(S.X, S.y, S.row(), 1, d, s2, S.sites(m), rho=0.0, rho_t=np.zeros(m))
        bands = orc.predict_bands(parts, s2)
        assert not np.asarray(parts["r"], dtype=np.float64).any()
        assert (np.abs(base["mean"][0] - np.asarray(parts["mean"], dtype=np.float64)) <= bands["mean"]).all()
        assert (np.abs(base["var"][0] - np.asarray(parts["var"], dtype=np.float64)) <= bands["var"]).all()
        assert abs(base["beta"][0] - float(parts["beta"])) <= bands["beta"]
        for k in ks:
            got, rc = run(ex.FarSiteDesign(n, k, d))
            _same(got, rc, base, rc0, "far site %s n=%d k=%d" % (scheme, n, k))


# ----------------------------------------------------------------------------- other consumers of R
@pytest.mark.parametrize("n", [14, 129])
def test_loo_batch(handle, n):
    D = ex.ExactDesign(n, (2, n))

    def fn(rows):
        mean, var, beta, q, st = handle.loo_batch(D.X, D.y, 2, rows, 1.3, lr.ORDINARY)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    base, exp = _lattice(handle, D, 2, D.mixed(), fn, _small if n <= 128 else (lambda t: _blocked(t, n)), n <= 128, "loo n=%d" % n)
    # R = I: the fold without point i predicts the mean of the others, with variance sigma2 (1 + 1 / (n - 1))
    want = (D.y.sum() - D.y) / (n - 1)
    for b in np.nonzero(exp == 0)[0]:
        assert (np.abs(base["mean"][b] - want) <= orc.PREDICT_TOL_C * EPS * np.abs(D.y).max()).all()
        assert (np.abs(base["var"][b] - 1.3 * (1.0 + 1.0 / (n - 1))) <= orc.PREDICT_TOL_C * EPS * 1.3).all()


def test_krige_predict_batch(handle):
    D = ex.ExactDesign(9, ex.predict_seps(9))
    Xt, on = D.sites(5, 4)

    def fn(rows):
        mean, var, beta, q, st = handle.krige_predict_batch(D.X, D.y, 2, rows, 1.3, Xt, kr.ORDINARY)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    base, exp = _lattice(handle, D, 2, D.mixed(), fn, _any, True, "krige_predict_batch")
    _identity_predict(base, exp, D, on, 2, 1.3)


def test_profile_batch(handle):
    D = ex.ExactDesign(9, ex.LOGLIK_REG8[9])

    def fn(rows):
        ll, s2, beta, g, st = handle.profile_batch(D.X, D.y, 2, rows, grad=True)
        return dict(ll=ll, s2=s2, beta=beta, grad=g, status=st)
    base, exp = _lattice(handle, D, 2, D.mixed(), fn, _any, True, "profile_batch")
    # R = I: sigma2-hat = sum (y - ybar)^2 / (n sum w^2)
    want = ((D.y - D.y.mean()) ** 2).sum() / (D.n * 2.0)
    for b in np.nonzero(exp == 0)[0]:
        assert abs(base["s2"][b] - want) <= orc.GRAD_TOL_C * EPS * want
        assert not base["grad"][b, 2:].any()


def test_mixed_logdet_designs(handle):
    def run(theta):
        designs, K, row, exp = ex.duplicate_designs(theta=theta)
        (ld, st), rc, t = _call(handle, lambda: handle.mixed_logdet_designs(designs, K, row))
        _small(t)
        return dict(logdet=ld, status=st), rc
    base = _far(run, 20, True, "mixed_logdet_designs")
    assert np.array_equal(base["status"], ex.duplicate_designs()[3]) and base["logdet"][1] == 0.0


@pytest.mark.parametrize("n_fixed", [0, 5])
def test_mixed_logdet_grad_designs(handle, n_fixed):
    def run(theta):
        designs, K, row, exp = ex.duplicate_designs(theta=theta)
        (ld, g, st), rc, t = _call(handle, lambda: handle.mixed_logdet_grad_designs(designs, K, row, n_fixed))
        _small(t)
        return dict(logdet=ld, grad=g, status=st), rc
    base = _far(run, 20, True, "mixed_logdet_grad_designs n_fixed=%d" % n_fixed)
    assert np.array_equal(base["status"], ex.duplicate_designs()[3])
    assert base["logdet"][1] == 0.0 and not base["grad"][1].any()


# ----------------------------------------------------------------------------- the two-scale mix: R = (I + R2) / 2
def _two_scale(h, T, fn, hot, what, n=None):
    """fn(rows) -> outputs of ONE call on the six rows (2048, then the far magnitudes): every row must equal row 0."""
    out, rc, t = _call(h, lambda: fn(T.rows()))
    st = np.asarray(out["status"])
    assert st[0] == 0, (what, st)
    for b, k in enumerate(ex.FAR_K, start=1):
        row = {name: np.asarray(v)[b:b + 1] for name, v in out.items()}
        row0 = {name: np.asarray(v)[0:1] for name, v in out.items()}
        if hot and k > STRICT_HOT_K:
            failed = _equal_or_failed(row, None, row0, None, T.n, "%s k=%d" % (what, k))
            OUTCOMES[(what, k)] = "failed" if failed else "equal"
        else:
            _same(row, 0, row0, 0, "%s k=%d" % (what, k))
    assert rc == int(np.count_nonzero(st)), (what, rc, st)
    return {name: np.asarray(v)[0] for name, v in out.items()}, t


@pytest.mark.parametrize("n,n_pad,want", [(17, 0, "reg"), (101, 62, "lds"), (129, 0, "blocked")], ids=["register", "lds", "blocked"])
def test_two_scale_likelihood_and_gradient(handle, n, n_pad, want):
    """orc.loglik_grad_parts in long double; band of tests/test_gpu_gradient_exact.py (GRAD_TOL_C eps cond1 scale) at rho = 0.  The
    far component's rate derivative is exactly 0."""
    T = ex.TwoScaleDesign(n, n_pad)
    assert route(T.n, T.d, 2) == want
    kappa_guard = T.guard()
    assert kappa_guard <= KAPPA_MAX

    def fn(rows):
        ll, beta, grad, st = handle.loglik_grad_batch(T.X, T.y, 2, rows, 1.3)
        return dict(ll=ll, beta=beta, grad=grad, status=st)
    base, t = _two_scale(handle, T, fn, want != "blocked", "two-scale gradient " + want)
    (_small if want != "blocked" else (lambda t: _blocked(t, n)))(t)
    parts = orc.loglik_grad_parts(T.X, T.y, T.row(), 2, T.d, 1.3, np.longdouble)
    kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
    assert kappa <= KAPPA_MAX
    g_ref, scale = orc.grad_from_parts(parts, T.X, T.row(), 2, T.d, 1.3)
    unit = EPS * kappa
    ratio = np.abs(base["grad"] - g_ref.astype(np.float64)) / np.maximum(unit * scale.astype(np.float64), 1e-300)
    far = slice(2, 2 + T.d)
    assert not base["grad"][far].any() and np.abs(g_ref[far]).max() < 1e-300     # (long double does not underflow at 2048)
    ratio[far] = 0.0
    print("two-scale gradient %s: cond1 %.3g, largest ratio %.3g of %g" % (want, kappa, ratio.max(), orc.GRAD_TOL_C))
    assert (ratio <= orc.GRAD_TOL_C).all(), ratio
    s_ll, s_beta = orc.loglik_beta_scales(parts, T.y)
    assert abs(base["ll"] - float(parts["loglik"])) <= orc.GRAD_TOL_C * unit * s_ll
    assert abs(base["beta"] - float(parts["beta"])) <= orc.GRAD_TOL_C * unit * s_beta
    # the plain likelihood call of the same rows, mode 0: the same evaluation
    def fl(rows):
        ll, beta, st = handle.loglik_batch(T.X, T.y, 2, rows, 1.3, 0, 0.0)
        return dict(ll=ll, beta=beta, status=st)
    b2, _ = _two_scale(handle, T, fl, n <= 128, "two-scale loglik n=%d" % n)
    assert abs(b2["ll"] - float(parts["loglik"])) <= orc.GRAD_TOL_C * unit * s_ll
    assert abs(b2["beta"] - float(parts["beta"])) <= orc.GRAD_TOL_C * unit * s_beta


@pytest.mark.parametrize("n", [9, 129])
def test_two_scale_marginal_likelihood(handle, n):
    """Mean mode 1 (sigma2 sum(w^2) R + tau2): orc.marginal_parts in long double, band MARGINAL_TOL_C units of orc.marginal_unit at
    rho = 0 (tests/test_gpu_marginal_exact.py)."""
    T = ex.TwoScaleDesign(n)
    s2, tau2 = 1.3, 2.5

    def fn(rows):
        ll, beta, st = handle.loglik_batch(T.X, T.y, 2, rows, s2, 1, tau2)
        return dict(ll=ll, beta=beta, status=st)
    base, _ = _two_scale(handle, T, fn, n <= 128, "two-scale marginal n=%d" % n)
    parts = orc.marginal_parts(T.X, T.y, T.row(), 2, T.d, s2, tau2)
    assert orc.cond1(parts["Sigma"], parts["Sinv"]) <= orc.MARGINAL_COND_MAX
    unit = orc.marginal_unit(parts, T.X, T.row(), 2, T.d, rho=0.0)
    r = abs(base["ll"] - float(parts["loglik"])) / unit
    print("two-scale marginal n=%d: %.3g of %g units" % (n, r, orc.MARGINAL_TOL_C))
    assert r <= orc.MARGINAL_TOL_C


@pytest.mark.parametrize("n,scheme", [(9, "kept"), (128, "extra"), (129, "blocked")])
def test_two_scale_prediction(handle, n, scheme):
    """orc.predict_parts / predict_bands (tests/test_gpu_predict_exact.py, PREDICT_TOL_C) at rho = 0; integer sites, on and off
    the training points."""
    T = ex.TwoScaleDesign(n)
    Xt, _ = T.sites(5)
    s2 = 1.3

    def fn(rows):
        mean, var, beta, st = handle.predict_batch(T.X, T.y, 2, rows, Xt, s2)
        return dict(mean=mean, var=var, beta=beta, status=st)
    base, t = _two_scale(handle, T, fn, scheme == "kept", "two-scale predict " + scheme)
    (_small if scheme != "blocked" else (lambda t: _blocked(t, n)))(t)
    assert sites_supported(n, T.d, 2) == (scheme == "kept")
    parts = orc.predict_parts(T.X, T.y, T.row(), 2, T.d, s2, Xt, rho=0.0, rho_t=np.zeros(5))
    bands = orc.predict_bands(parts, s2)
    for name in ("mean", "var"):
        d = np.abs(base[name] - np.asarray(parts[name], dtype=np.float64))
        print("two-scale predict %s %s: largest |d| / band %.3g" % (scheme, name, (d / bands[name]).max()))
        assert (d <= bands[name]).all(), (name, d / bands[name])
    assert abs(base["beta"] - float(parts["beta"])) <= bands["beta"]


@pytest.mark.parametrize("n", [14, 129])
def test_two_scale_leave_one_out(handle, n):
    """tests/loo_ref.py: reference() in long double, bands() with unit = C eps cond1 (rho = 0)."""
    T = ex.TwoScaleDesign(n)
    s2 = 1.3

    def fn(rows):
        mean, var, beta, q, st = handle.loo_batch(T.X, T.y, 2, rows, s2, lr.ORDINARY)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    base, _ = _two_scale(handle, T, fn, n <= 128, "two-scale loo n=%d" % n)
    ref = lr.reference(T.X, T.y, T.row(), 2, rho=0.0)
    assert ref["cond1"] <= lr.KAPPA_MAX
    bnd = lr.bands(ref)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    assert (np.abs(base["mean"] - f64(ref["mean"])) <= bnd["mean"]).all()
    assert (np.abs(base["var"] - f64(lr.variance(ref, lr.ORDINARY, s2))) <= lr.variance_band(ref, bnd, lr.ORDINARY, s2)).all()
    assert abs(base["beta"] - float(ref["beta"])) <= bnd["beta"] and abs(base["q"] - float(ref["Q"])) <= bnd["Q"]


def test_two_scale_kriging_prediction(handle):
    """tests/krige_ref.py: reference() / bands() at rho = 0, the three variance forms' shared mean, beta and Q and the ORDINARY
    variance."""
    T = ex.TwoScaleDesign(9)
    Xt, _ = T.sites(5)
    s2 = 1.3

    def fn(rows):
        mean, var, beta, q, st = handle.krige_predict_batch(T.X, T.y, 2, rows, s2, Xt, kr.ORDINARY)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    base, _ = _two_scale(handle, T, fn, True, "two-scale krige")
    ref = kr.reference(T.X, T.y, T.row(), 2, Xt, rho=0.0, rho_t=np.zeros(5))
    bnd = kr.bands(ref)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    assert (np.abs(base["mean"] - f64(ref["mean"])) <= bnd["mean"]).all()
    assert (np.abs(base["var"] - f64(kr.variance(ref, kr.ORDINARY, s2))) <= kr.variance_band(ref, bnd, kr.ORDINARY, s2)).all()
    assert abs(base["beta"] - float(ref["beta"])) <= bnd["beta"] and abs(base["q"] - float(ref["Q"])) <= bnd["Q"]


def test_two_scale_design_criteria(handle):
    """tests/design_exact.py: reference(exact_exponent = True), constants design_constants(); two copies of one design, the row
    shared per call, so one call per magnitude."""
    T = ex.TwoScaleDesign(14)
    C_LD, C_G = dx.design_constants()
    designs = np.stack([T.X] * 2)

    def grad(theta):
        (ld, g, st), rc, t = _call(handle, lambda: handle.mixed_logdet_grad_designs(designs, 2, T.row(theta[0]), 0))
        return dict(logdet=ld, grad=g, status=st), rc

    def logdet(theta):
        (ld, st), rc, t = _call(handle, lambda: handle.mixed_logdet_designs(designs, 2, T.row(theta[0])))
        return dict(logdet=ld, status=st), rc
    bg = _far(grad, 14, True, "two-scale design gradient")
    bl = _far(logdet, 14, True, "two-scale design logdet")
    assert not bg["status"].any() and not bl["status"].any()
    ref = dx.reference(T.X, T.row(), 2, exact_exponent=True)
    assert dx.ratio_ld(bg["logdet"][0], ref) <= C_LD and dx.ratio_ld(bl["logdet"][0], ref) <= C_LD
    assert dx.ratio_g(bg["grad"][0], ref) <= C_G


def test_zz_report():
    """Which of the two allowed outcomes each hot route gave at k >= 200 (DESIGN.md (c) records them)."""
    for key in sorted(OUTCOMES):
        print("%-48s k=%-5d %s" % (key[0], key[1], OUTCOMES[key]))
