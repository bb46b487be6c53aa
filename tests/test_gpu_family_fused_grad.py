"""The 1-D families' analytic gradient and profiled mode on the register-resident evaluator (CCGP_OPT_FAMILY_FUSED_GRAD: the
FAM + PROF and FAM + INV = 2 instances of csrc/small_reg.hip, family_corr_grad, family_dcorr_kernel).

Held, always with the option on and nu = 2.5 unless a case says otherwise:
  entries   ccgp_family_corr_dtheta against tests/family_grad_exact.py's 40-digit derivative inside its bands over family_exact's
            sweep (every nu, two thetas; the spline across both branches and the knots); the diagonal exactly 0, entries with
            z >= 1e4 exactly 0, the table symmetric, a NaN coordinate poisons its row and column alone;
  gradient  ccgp_loglik_grad_batch and ccgp_profile_batch(grad=True) on test_gpu_family_fused.make_case at families 1 and 2,
            n = 8, 17, 32, Matern K = 1 at nu = 5, Matern K = 4 (the component loop's second pass), n = 2 (a single pair) and
            n = 16 (a full block): every gradient column within
                GRAD_TOL_C eps cond1 (1 + rho) scale_j + sigma2 w_q^2 sum_ab |M_ab| dband_q,ab      (second term: theta columns)
            of the long-double closed form built from the exact entries (oracle.loglik_grad_parts(..., Rc=...),
            family_grad_exact.family_grad_from_parts); rho from the Gram bands as test_gpu_family_fused.reference takes it;
            cond1 <= 1e8 asserted; log-likelihood and beta by check_loglik_beta; the profiled call at the long-double
            sigma2_hat, sigma2_hat itself within GRAD_TOL_C eps cond1 (1 + rho) sigma2_ref as tests/test_gpu_profile.py holds
            it.  ccgp_profile_batch(grad=False), fused, on both grids (B = 2 and the same rows inside a call of 70: the same
            bits) within the same value bands;
  bits      every row of ccgp_profile_batch_sets(grad=True) equals the single-set call on its set (C = 3, n 8 and 17, B 1, 5,
            70, mixed set_of, both families); cutting B changes nothing; the same bits after ccgp_debug_fill_scratch(0x00 /
            0xFF) and after a Gaussian call of another shape;
  failure   a duplicated point gives the 1-based pivot index and a NaN row, gradient included, in its set alone; a NaN
            coordinate poisons its set alone; constant y gives sigma2_hat = 0, l_p = +Inf, a NaN gradient and status 0;
  option    0 and 1 only; off: all three gradient calls refused with -4 and no output touched (the one case that passes
            without the feature); on: n = 33 and d = 2 still refused; options 11 and 12 move nothing of this;
  fit       fit.matern_MLEs_sets on 6 seeded designs of n = 8 at nu = 5: per set a profiled log-likelihood within 1e-3 of
            matern_MLEs(fused=True) on that set (test_fit_on_qian's tolerance), the same bits alone and in the group, and
            fewer device calls for the group than for one set's matern_MLEs.

Nothing in a band comes from a device run.  Measured on an MI355X (test_zz_report_headroom): see DESIGN.md K20.
"""
import functools
import math

import numpy as np
import pytest

import family_exact as fx
import family_grad_exact as gx
import test_gpu_family_fused as ff
from oracle import ccgp_oracle as orc
from profile_ref import sigma2_exact
from test_gpu_gradient_exact import _timed, check_loglik_beta

pytestmark = pytest.mark.gpu

EPS = fx.EPS
NU = ff.NU
C = orc.GRAD_TOL_C
KAPPA_MAX = 1e8
MAX_RATIO = {}
# (family, n, nu, K)
CASES = [(fam, n, NU, 2) for fam in (1, 2) for n in (8, 17, 32)] + [(1, 8, 5.0, 1), (1, 8, NU, 4), (1, 2, NU, 2), (2, 2, NU, 2),
                                                                     (1, 16, NU, 2), (2, 16, NU, 2)]
IDS = ["family%d-n%d-nu%g-K%d" % c for c in CASES]
same_bits = ff.same_bits


def _note(tag, ratio):
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float(ratio))


class fused_grad:
    """The handle under a 1-D family with option 13 at `on` (and options 11 / 12 as given); Gaussian and 0 afterwards."""

    def __init__(self, h, family, nu=NU, on=1, fused=0, fused_predict=0):
        self.h, self.family, self.nu, self.on, self.o11, self.o12 = h, family, nu, on, fused, fused_predict

    def __enter__(self):
        from ccgp_amd import api
        self.h.set_kernel(api.KERNEL_MATERN if self.family == 1 else api.KERNEL_MATERN_SPLINE, self.nu)
        self.h.set_option(api.OPT_FAMILY_FUSED_GRAD, self.on)
        self.h.set_option(api.OPT_FAMILY_FUSED, self.o11)
        self.h.set_option(api.OPT_FAMILY_FUSED_PREDICT, self.o12)
        return self.h

    def __exit__(self, *exc):
        from ccgp_amd import api
        for o in (api.OPT_FAMILY_FUSED_GRAD, api.OPT_FAMILY_FUSED, api.OPT_FAMILY_FUSED_PREDICT):
            self.h.set_option(o, 0)
        self.h.set_kernel(api.KERNEL_GAUSS, 0.0)


# ----------------------------------------------------------------------------- entries
def _check_entries(handle, family, nu, row, K, q, x, tag):
    """The table of component q on the coordinates x (x[0] = 0): row 0 and column 0 against the exact derivative, the whole
    table symmetric with a zero diagonal."""
    with fused_grad(handle, family, nu, on=0):                      # the entry point needs no option
        D = handle.family_corr_dtheta(x, K, row, q)
    assert D.shape == (x.size, x.size)
    assert same_bits(D, D.T) and (np.diag(D) == 0.0).all()
    T = gx.dtable(family, nu, row[K:], q, x[:1], x)
    if not (family == 2 and q == 1):
        # at or below the switch z^2 <= 9e-20 (the kernel's z^2, formed as the kernel forms it) the derivative is exactly 0, and
        # the true value it stands for is at most 2.1e-18 / theta: those entries are held to that, not to the band
        theta = float(row[K + q])
        below = (4.0 * nu / (theta * theta)) * (x * x) <= gx.SWITCH_Z2
        assert (D[0, below] == 0.0).all() and (D[below, 0] == 0.0).all()
        assert (T.hi[0, below] * theta <= gx.BELOW_SWITCH).all()
        T.has[0, below] = False
    for dev in (D[:1, :], D[:, :1].T):
        ratio, bad = fx.worst_ratio(dev, T)
        assert not bad, (tag, bad[:5])
        _note(tag, ratio)
    return D


@pytest.mark.parametrize("nu", fx.NUS)
def test_matern_entries_inside_the_bands_over_the_sweep(handle, nu):
    for theta in fx.SWEEP_THETAS:
        h = fx.sweep_h(nu, theta)                                   # ..., z = 1e4, h = 0
        x = np.concatenate([[0.0], h])
        D = _check_entries(handle, 1, nu, np.array([1.0, theta]), 1, 0, x, "entries/matern")
        far = 2.0 * math.sqrt(nu) * np.abs(x[:, None] - x[None, :]) / theta >= 1e4
        assert far.any() and (D[far] == 0.0).all()
        assert D[0, -1] == 0.0 and D[0, -2] == 0.0                   # the coincident point, and z = 1e4 from the origin
        assert (D[0, 1:-2] > 0.0).sum() >= 150                       # and the sweep itself is not zero


def test_spline_entries_inside_the_bands(handle):
    for theta in (1.0, 0.3):
        h = list(np.linspace(0.0, 1.2, 49)[1:] * theta)
        for knot in (theta / 2.0, theta):
            h += [np.nextafter(knot, 0.0), knot, np.nextafter(knot, 2.0)]
        h.append(theta * (1.0 + 8.0 * EPS))
        x = np.concatenate([[0.0], h])
        D = _check_entries(handle, 2, NU, np.array([0.75, 0.5, 0.5, theta]), 2, 1, x, "entries/spline")
        assert D[0, -1] == 0.0 and (D[0, x > theta * (1.0 + 8.0 * EPS)] == 0.0).all()
        # component 0 of the pair is the Matern one
        _check_entries(handle, 2, NU, np.array([0.75, 0.5, 0.5, theta]), 2, 0, x[:20], "entries/matern")


def test_a_nan_coordinate_poisons_its_row_and_column_alone(handle):
    x = np.concatenate([[0.0], fx.near_coincident_design(0.0)])
    xn = x.copy()
    xn[5] = math.nan
    row = np.array([0.75, 0.5, 0.5, 1.0])
    with fused_grad(handle, 2, on=0):
        for q in (0, 1):
            clean, D = handle.family_corr_dtheta(x, 2, row, q), handle.family_corr_dtheta(xn, 2, row, q)
            keep = np.ones(x.size, dtype=bool)
            keep[5] = False
            assert np.isnan(D[5, :]).all() and np.isnan(D[:, 5]).all()
            assert same_bits(D[np.ix_(keep, keep)], clean[np.ix_(keep, keep)]) and np.isfinite(clean).all()


def test_the_entry_point_refuses_the_gaussian_family(handle):
    from ccgp_amd import api
    with pytest.raises(api.CcgpError) as e:
        handle.family_corr_dtheta(np.linspace(0.0, 1.0, 5), 1, [1.0, 0.3], 0)
    assert e.value.code == -4


# ----------------------------------------------------------------------------- gradient: the references
@functools.lru_cache(maxsize=None)
def reference(family, n, nu, K, b):
    """What draw b of test_gpu_family_fused.make_case is held to, in long double from the exact entries: the plain call at
    sigma2 = S2_TAU2[0] and the profiled call at the long-double sigma2_hat."""
    x, y, rows = ff.make_case(family, n, nu, K)
    row, X = rows[b], x[:, None]
    gram = ff.component_tables(family, nu, row, K, x) if K <= 2 else [fx.table(1, nu, (1.0,), (row[K + c],), x, x) for c in range(K)]
    der = [gx.dtable(family, nu, row[K:], q, x, x) for q in range(K)]
    Rc, Dc, dband = [T.longdouble() for T in gram], [T.longdouble() for T in der], [T.band for T in der]
    w2 = row[:K] ** 2
    val = sum(w2[c] * gram[c].hi for c in range(K)) / w2.sum()
    band = sum(w2[c] * gram[c].band for c in range(K)) / w2.sum() + 2.0 * EPS * np.abs(val)
    off = band * (1.0 - np.eye(n))                                            # the device's diagonal is exactly 1
    keep = off > 0
    assert (val[keep] > 0).all()
    rho = float((off[keep] / (EPS * val[keep])).max())

    def held(s2, parts):
        kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
        unit = EPS * kappa * (1.0 + rho)
        grad, scale, extra = gx.family_grad_from_parts(parts, row, K, Dc, s2, dband)
        s_ll, s_beta = orc.loglik_beta_scales(parts, y)
        return dict(ll=float(parts["loglik"]), beta=float(parts["beta"]), unit_ll=unit * s_ll, unit_beta=unit * s_beta, kappa=kappa,
                    grad=grad.astype(np.float64), unit_grad=unit * scale.astype(np.float64), extra=extra.astype(np.float64))

    s2 = ff.S2_TAU2[0]
    plain = held(s2, orc.loglik_grad_parts(X, y, row, K, 1, s2, np.longdouble, Rc=Rc))
    s2_hat, p1 = sigma2_exact(X, y, row, K, 1, np.longdouble, Rc=Rc)
    prof = held(s2_hat, orc.loglik_grad_parts(X, y, row, K, 1, s2_hat, np.longdouble, Rc=Rc))
    prof["sigma2"] = float(s2_hat)
    prof["unit_sigma2"] = EPS * orc.cond1(p1["Sigma"], p1["Sinv"]) * (1.0 + rho) * float(s2_hat)
    return dict(rho=rho, plain=plain, prof=prof)


def _check_grad(ref, g, tag, what):
    tol = C * ref["unit_grad"] + ref["extra"]
    err = np.abs(g - ref["grad"])
    ratio = err / tol
    print("%s %s: gradient %s ref %s |diff| / band %s (cond1 %.3g)" % (tag, what, g, ref["grad"], np.round(ratio, 4), ref["kappa"]))
    _note("gradient/%s (of the band)" % what, ratio.max())
    assert (err <= tol).all(), (tag, what, g, ref["grad"], ratio)


def _check_value(ref, ll, beta, tag, what):
    assert ref["kappa"] <= KAPPA_MAX, (tag, ref["kappa"])
    r = check_loglik_beta(ref["ll"], ref["beta"], ref["unit_ll"], ref["unit_beta"], ll, beta, tag)
    _note("value/%s (of GRAD_TOL_C = %g)" % (what, C), max(r))


def _check_sigma2(ref, s2, tag):
    ratio = abs(s2 - ref["sigma2"]) / ref["unit_sigma2"]
    print("%s sigma2_hat %.17g ref %.17g ratio %.3g" % (tag, s2, ref["sigma2"], ratio))
    _note("sigma2_hat (of GRAD_TOL_C = %g)" % C, ratio)
    assert ratio <= C, (tag, s2, ref["sigma2"], ratio)


@pytest.mark.parametrize("family,n,nu,K", CASES, ids=IDS)
def test_gradients_exact(handle, family, n, nu, K):
    x, y, rows = ff.make_case(family, n, nu, K)
    X = x[:, None]
    many = np.tile(rows, (35, 1)) * np.concatenate([np.ones((70, K)), 1.0 + 0.004 * np.arange(70)[:, None] * np.ones((1, K))], axis=1)
    many[3], many[66] = rows[0], rows[1]
    with fused_grad(handle, family, nu):
        (ll, beta, g, st), t = _timed(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, ff.S2_TAU2[0]))
        assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["solve"][1] == 0, t
        (pl, ps2, pbeta, pg, pst), t = _timed(handle, lambda: handle.profile_batch(X, y, K, rows, grad=True))
        assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["solve"][1] == 0, t
        (vl, vs2, vbeta, vg, vst), t = _timed(handle, lambda: handle.profile_batch(X, y, K, rows, grad=False))
        assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["solve"][1] == 0 and vg is None, t
        big = handle.profile_batch(X, y, K, many, grad=False)        # the 8 x 8 grid
    assert not st.any() and not pst.any() and not vst.any() and not big[4].any()
    assert g.shape == (2, 2 * K) and pg.shape == (2, 2 * K)
    for k in range(3):                                              # the two grids give the same bits
        assert same_bits(big[k][[3, 66]], (vl, vs2, vbeta)[k]), k
    tag = "family%d-n%d-nu%g-K%d" % (family, n, nu, K)
    for b in range(2):
        ref = reference(family, n, nu, K, b)
        _check_value(ref["plain"], ll[b], beta[b], tag, "plain")
        _check_grad(ref["plain"], g[b], tag, "plain")
        _check_sigma2(ref["prof"], ps2[b], tag)
        _check_value(ref["prof"], pl[b], pbeta[b], tag, "profiled")
        _check_grad(ref["prof"], pg[b], tag, "profiled")
        _check_sigma2(ref["prof"], vs2[b], tag + " value-only")
        _check_value(ref["prof"], vl[b], vbeta[b], tag, "profiled value-only")


# ----------------------------------------------------------------------------- bits
def per_set(h, Xs, ys, P, set_of):
    """The reference: the rows of every set through the single-set call, gradient included."""
    B = len(P)
    ll, s2, beta, st = np.full(B, np.nan), np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    g = np.full((B, P.shape[1]), np.nan)
    for c in np.unique(set_of):
        rows = np.flatnonzero(set_of == c)
        ll[rows], s2[rows], beta[rows], g[rows], st[rows] = h.profile_batch(Xs[c], ys[c], 2, P[rows], grad=True)
    return ll, s2, beta, g, st


def _same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b), k


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("n", [8, 17])
def test_sets_rows_have_the_bits_of_the_single_set_call(handle, n, B):
    Xs, ys, _, P, set_of = ff.sets_case(n, 3, B, 100 * n + B)
    for family in (1, 2):
        with fused_grad(handle, family):
            want = per_set(handle, Xs, ys, P, set_of)
            assert not want[4].any() and np.isfinite(want[3]).all()
            got, t = _timed(handle, lambda: handle.profile_batch_sets(Xs, ys, 2, P, set_of, grad=True))
            assert t["fused"][1] == 1 and t["diag"][1] == 0, t          # one launch for all sets
            _same(got, want)
            if B == 70:
                parts = [handle.profile_batch_sets(Xs, ys, 2, P[a:b], set_of[a:b], grad=True) for a, b in ((0, 33), (33, 70))]
                _same([np.concatenate([p[k] for p in parts]) for k in range(5)], want)
                # the value-only sets form goes set by set through the fused single call
                val, t = _timed(handle, lambda: handle.profile_batch_sets(Xs, ys, 2, P, set_of, grad=False))
                assert t["fused"][1] == 3 and t["diag"][1] == 0 and val[3] is None, t
                for c in range(3):
                    rows = np.flatnonzero(set_of == c)
                    one = handle.profile_batch(Xs[c], ys[c], 2, P[rows], grad=False)
                    _same([val[k][rows] for k in (0, 1, 2, 4)], [one[k] for k in (0, 1, 2, 4)])


def test_bits_do_not_depend_on_the_handles_history(handle):
    Xs, ys, _, P, set_of = ff.sets_case(17, 3, 70, 1700)
    rng = np.random.default_rng(64)
    Xg = rng.random((64, 3))

    def both():
        with fused_grad(handle, 1):
            return (handle.profile_batch_sets(Xs, ys, 2, P, set_of, grad=True),
                    handle.loglik_grad_batch(Xs[0], ys[0], 2, P[:5], 1.3))

    want = both()
    assert not want[0][4].any() and not want[1][3].any()
    try:
        for fill in (0x00, 0xFF, None):
            if fill is None:   # an unrelated Gaussian call of another shape
                handle.loglik_batch(Xg, np.sin(3.0 * Xg).sum(axis=1), 2, np.tile([0.5, 0.5, 1.0, 2.0, 3.0, 30.0, 40.0, 50.0], (5, 1)), 1.0)
            else:
                handle.debug_fill_scratch(fill)
            got = both()
            _same(got[0], want[0])
            _same(got[1], want[1])
    finally:
        handle.debug_fill_scratch(-1)


# ----------------------------------------------------------------------------- failure contract
@pytest.mark.parametrize("family", [1, 2])
def test_a_duplicated_point_fails_its_own_rows_with_the_pivot_index(handle, family):
    n = 9
    Xs, ys, _, P, set_of = ff.sets_case(n, 3, 7, 1200 + family)
    Xs = Xs.copy()
    Xs[1, 7, 0] = Xs[1, 3, 0]                         # rows 3 and 7 of set 1 coincide: two equal rows of R, pivot 7 vanishes
    with fused_grad(handle, family):
        ll, s2, beta, g, st = handle.profile_batch_sets(Xs, ys, 2, P, set_of, grad=True)
        one = handle.profile_batch(Xs[1], ys[1], 2, P[set_of == 1], grad=True)
        plain = handle.loglik_grad_batch(Xs[1], ys[1], 2, P[set_of == 1], 1.0)
    hit = set_of == 1
    assert hit.any() and (~hit).any()
    assert (st[hit] == 8).all() and all(np.isnan(a[hit]).all() for a in (ll, s2, beta, g))
    assert not st[~hit].any() and all(np.isfinite(a[~hit]).all() for a in (ll, s2, beta, g))
    assert (one[4] == 8).all() and all(np.isnan(one[k]).all() for k in range(4))
    assert (plain[3] == 8).all() and all(np.isnan(plain[k]).all() for k in range(3))


@pytest.mark.parametrize("family", [1, 2])
def test_a_nan_coordinate_poisons_its_own_set_alone(handle, family):
    n = 9
    Xs, ys, _, P, set_of = ff.sets_case(n, 3, 7, 1300 + family)
    Xn = Xs.copy()
    Xn[2, 4, 0] = math.nan
    with fused_grad(handle, family):
        clean = handle.profile_batch_sets(Xs, ys, 2, P, set_of, grad=True)
        ll, s2, beta, g, st = handle.profile_batch_sets(Xn, ys, 2, P, set_of, grad=True)
    hit = set_of == 2
    assert hit.any() and (~hit).any() and not clean[4].any()
    assert (st[hit] != 0).all() and all(np.isnan(a[hit]).all() for a in (ll, s2, beta, g))
    assert not st[~hit].any()
    _same([a[~hit] for a in (ll, s2, beta, g)], [a[~hit] for a in clean[:4]])


@pytest.mark.parametrize("family", [1, 2])
def test_a_constant_response_has_no_gradient_and_no_failure(handle, family):
    x, _, rows = ff.make_case(family, 8, NU, 2)
    with fused_grad(handle, family):
        for grad in (True, False):
            ll, s2, beta, g, st = handle.profile_batch(x[:, None], np.full(8, 2.0), 2, rows, grad=grad)
            assert not st.any() and (s2 == 0.0).all() and (ll == np.inf).all() and (beta == 2.0).all(), (grad, ll, s2, beta, st)
            assert g is None or np.isnan(g).all()


# ----------------------------------------------------------------------------- the option
def test_the_option_takes_zero_and_one(handle):
    from ccgp_amd import api
    assert api.OPT_FAMILY_FUSED_GRAD == 13
    for bad in (2, -1):
        with pytest.raises(api.CcgpError) as e:
            handle.set_option(api.OPT_FAMILY_FUSED_GRAD, bad)
        assert e.value.code == -1
    handle.set_option(api.OPT_FAMILY_FUSED_GRAD, 1)
    handle.set_option(api.OPT_FAMILY_FUSED_GRAD, 0)


def _raw_gradient_calls(h, n=8, d=1, K=2):
    """The three gradient entry points through ctypes with every output pre-filled -> [(rc, outputs untouched?)]."""
    from ccgp_amd import api
    rng = np.random.default_rng(n + d)
    X, y = np.asfortranarray(rng.random((n, d))), rng.random(n)
    P = K + K * d
    rows = np.asfortranarray(np.tile(np.concatenate([np.full(K, 0.5), np.full(K * d, 0.3)]), (2, 1)))
    set_of = np.zeros(2, dtype=np.int32)
    out = []
    for which in range(3):
        ll, s2, beta, g, st = np.full(2, 5.0), np.full(2, 6.0), np.full(2, 7.0), np.full((2, P), 8.0, order="F"), np.full(2, 9, dtype=np.int32)
        if which == 0:
            rc = api.lib().ccgp_loglik_grad_batch(h._h, api._p(X), n, d, api._p(y), K, api._p(rows), 2, 1.0, api._p(ll), api._p(beta),
                                                  api._p(g), api._ipt(st))
        elif which == 1:
            rc = api.lib().ccgp_profile_batch(h._h, api._p(X), n, d, api._p(y), K, api._p(rows), 2, api._p(ll), api._p(s2), api._p(beta),
                                              api._p(g), api._ipt(st))
        else:
            rc = api.lib().ccgp_profile_batch_sets(h._h, api._p(X), n, d, api._p(y), 1, K, api._p(rows), api._ipt(set_of), 2, api._p(ll),
                                                   api._p(s2), api._p(beta), api._p(g), api._ipt(st))
        out.append((rc, (ll == 5.0).all() and (s2 == 6.0).all() and (beta == 7.0).all() and (g == 8.0).all() and (st == 9).all()))
    return out


def test_with_the_option_off_the_gradient_is_refused(handle):
    """Today's behaviour, which the option's default keeps: CCGP_EUNSUPPORTED and no output touched, whatever options 11 and 12
    say."""
    for family in (1, 2):
        for o11, o12 in ((0, 0), (1, 1)):
            with fused_grad(handle, family, on=0, fused=o11, fused_predict=o12):
                for rc, untouched in _raw_gradient_calls(handle):
                    assert rc == -4 and untouched


def test_with_the_option_on_beyond_the_domain_it_is_still_refused(handle):
    with fused_grad(handle, 1):
        for rc, untouched in _raw_gradient_calls(handle, n=33):
            assert rc == -4 and untouched
        for rc, untouched in _raw_gradient_calls(handle, n=8, d=2):
            assert rc == -4 and untouched
        for rc, untouched in _raw_gradient_calls(handle, n=32):
            assert rc >= 0 and not untouched
    with fused_grad(handle, 2):
        for rc, untouched in _raw_gradient_calls(handle, n=8, K=3):
            assert rc == -4 and untouched


def test_options_11_and_12_move_nothing_of_this(handle):
    x, y, rows = ff.make_case(1, 17, NU, 2)
    X = x[:, None]
    with fused_grad(handle, 1):
        want = (handle.loglik_grad_batch(X, y, 2, rows, 1.0), handle.profile_batch(X, y, 2, rows, grad=True),
                handle.profile_batch(X, y, 2, rows, grad=False)[:3])
    with fused_grad(handle, 1, fused=1, fused_predict=1):
        got = (handle.loglik_grad_batch(X, y, 2, rows, 1.0), handle.profile_batch(X, y, 2, rows, grad=True),
               handle.profile_batch(X, y, 2, rows, grad=False)[:3])
    for g, w in zip(got, want):
        _same(g, w)
    # and with option 13 off, option 11 leaves the value-only profiled call on the sweep
    with fused_grad(handle, 1, on=0, fused=1):
        (_, _, _, _, st), t = _timed(handle, lambda: handle.profile_batch(X, y, 2, rows, grad=False))
        assert t["fused"][1] == 0 and t["diag"][1] > 0 and not st.any(), t


# ----------------------------------------------------------------------------- the fit
class Counting:
    """A handle proxy that counts the device calls made through it."""

    def __init__(self, h):
        self._h, self.calls = h, 0

    def __getattr__(self, name):
        attr = getattr(self._h, name)
        if not callable(attr) or name in ("close", "set_kernel", "set_option"):
            return attr

        def call(*a, **k):
            self.calls += 1
            return attr(*a, **k)
        return call


def test_matern_mles_sets(handle):
    from ccgp_amd import fit
    nu, n, S = 5.0, 8, 6
    # D1's shape: Latin-hypercube designs of [0, 1], one point per stratum, y = sin 10 x -- the generator of
    # scripts/family_fused_predict_timing.designs.  Not uniform random points: two of those 3e-4 apart give a Matern(5) matrix of
    # condition 1e16 near the optimum, where the fp64 likelihood is rounding noise of +- 0.2 (seen on the CPU in long double
    # against fp64) and no two searches can agree to 1e-3.  The precondition is asserted from the inputs alone.
    Ds = []
    for c in range(S):
        rng = np.random.default_rng(1000 + c)
        Ds.append((rng.permutation(n) + rng.random(n)) / n)
    assert min(np.diff(np.sort(D)).min() for D in Ds) >= 0.01
    ys = [np.sin(10.0 * D) for D in Ds]
    counted = Counting(handle)
    group, t = _timed(handle, lambda: fit.matern_MLEs_sets(counted, Ds, ys, nu))
    assert t["diag"][1] == 0 and t["fused"][1] == counted.calls == max(r["calls"] for r in group), (t, counted.calls)
    single_calls = []
    for c in range(S):
        one = Counting(handle)
        m = fit.matern_MLEs(one, Ds[c], ys[c], nu, fused=True)
        single_calls.append(one.calls)
        lp = fit.matern_profile(handle, Ds[c], ys[c], nu, [m["theta"]], fused_grad=True)
        want = float(-(lp["loglikeli"][0] + n * math.log(2.0 * math.pi) + n) / 2.0)
        print("set %d: lockstep theta %.10g l_p %.12g (%d calls); matern_MLEs theta %.10g l_p %.12g (%d calls)" % (
            c, group[c]["theta"], group[c]["loglik"], group[c]["calls"], m["theta"], want, one.calls))
        assert abs(group[c]["loglik"] - want) <= 1e-3, (c, group[c], m, want)
        alone = fit.matern_MLEs_sets(handle, [Ds[c]], [ys[c]], nu)[0]
        assert alone == group[c], (c, alone, group[c])                          # the same bits alone and in the group
    assert counted.calls < min(single_calls), (counted.calls, single_calls)
    with pytest.raises(ValueError):
        fit.matern_MLEs_sets(handle, [Ds[0], Ds[1][:7]], [ys[0], ys[1][:7]], nu)
    (_, _, st), _ = _timed(handle, lambda: handle.loglik_batch(Ds[0][:, None], ys[0], 2, np.array([[0.6, 0.4, 3.0, 40.0]]), 1.0))
    assert not st.any()                                  # and the handle is Gaussian again, option off


def test_zz_report_headroom():
    for k in sorted(MAX_RATIO):
        print("max ratio %-48s %.3g" % (k, MAX_RATIO[k]))
