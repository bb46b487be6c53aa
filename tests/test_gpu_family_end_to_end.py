"""The 1-D scripts' families end to end, once per family: what is new on their path beside the family-agnostic sweep (held for
Gaussian draws by tests/test_gpu_marginal_exact.py and tests/test_gpu_predict_exact.py) is the lower-tile build with
theta_to_rate, the mode-1 scale and shift in cov_kernel<1>, and family 2's un-normalised cross rows inside prediction
(D1F:470-480, D1F:737-754).

Cases: Matern with K = 2 and Matern + spline; n = 14 (a jittered grid) and n = 129 (a 64 and a 128 tile edge, identity
padding; the grid x_i = (i + j_i) / 128 with j_i in {0, 1/4, 1/2}, not equispaced, so that R is not Toeplitz, and dyadic, so
that it has 645 distinct |h| and not 8256); two draws each, theta 2 - 3 spacings; m = 3 sites: on a design point, 1e-3 of a
spacing beside one, and between two.

Held, with Sigma, R and r built from the exact entries of tests/family_exact.py rounded to long double:
  mode 0   log-likelihood and beta within tests/test_gpu_gradient_exact.py check_loglik_beta's band, GRAD_TOL_C eps cond1
           (1 + rho) size, cond1(Sigma) <= 1e8 asserted;
  mode 1   |ll - ll_ref| <= MARGINAL_TOL_C unit (oracle.marginal_unit), beta == 0, cond1(Sigma) <= MARGINAL_COND_MAX asserted;
  tables   predict.post mean, variance and beta within oracle.predict_bands, cond1(R) <= 1e8 asserted.
In those bands rho is the relative error of a kernel value in units of eps.  For the Gaussian family that is the size of the
expanded exponent; here it is the largest band / (eps |entry|) over the off-diagonal entries of the matrix in question, with
family_exact's component-wise bands (5e-14 + 4 eps z for the Matern: rho = 225 + 4 z): against Sigma0 for the likelihoods,
against W = |L| |L|' >= |R| for the factor and against |r| for a site's row.  Nothing else in the bands changes, and nothing
in them comes from a device run.

Measured on an MI355X (test_zz_report_headroom; Matern / Matern + spline): mode 0 3.9e-5 / 6.2e-5 of the 128 units allowed,
mode 1 0.011 / 0.0072 of 4, tables: variance 0.011 / 0.0067, mean 5.2e-4 / 6.5e-4, beta 1.5e-4 / 1.1e-4 of 128; cond1 <= 635
(mode 0, tables) and <= 1.3e6 (mode 1), rho 285 ... 930.  Under family 2 the variance at a design point is not 0 and can be
negative: r is un-normalised there, as in the script; the reference has the same values.
"""
import functools

import numpy as np
import pytest

import family_exact as fx
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import _timed, check_loglik_beta

pytestmark = pytest.mark.gpu

EPS = fx.EPS
NU = 2.5
S2_TAU2 = (1.0, 25.0)
SIGMA2 = 1.3
KAPPA_MAX = 1e8                    # tests/test_gpu_gradient_exact.py, tests/test_gpu_predict_exact.py
MAX_RATIO = {}
CASES = [(fam, n) for fam in (1, 2) for n in (14, 129)]


# ----------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def make_case(family, n):
    """(x[n], y[n], rows[2, 4], sites[3]) of one case."""
    rng = np.random.default_rng(500 + 10 * n + family)
    if n == 14:
        x = np.sort((np.arange(n) + rng.uniform(0.2, 0.8, n)) / n)
        h = 1.0 / n
    else:
        i = np.arange(n)
        x = (i + ((7 * i * i + i // 5) % 3) / 4.0) / 128.0
        h = 1.0 / 128.0
    y = np.sin(9.0 * x) + 0.3 * np.cos(31.0 * x) + 0.3 * x
    rows = np.column_stack([rng.uniform(0.3, 0.9, 2), rng.uniform(0.3, 0.9, 2), rng.uniform(2.0, 3.0, 2) * h, rng.uniform(2.0, 3.0, 2) * h])
    sites = np.array([x[n // 2], x[3] + 1e-3 * h, 0.5 * (x[n - 2] + x[n - 1])])
    for a in (x, y, rows, sites):
        a.setflags(write=False)
    return x, y, rows, sites


def _component_tables(family, row, XA, XB):
    """The K = 2 component Tables of a block (the spline alone is the pair with weights (0, 1))."""
    first = fx.table(1, NU, (1.0,), (row[2],), XA, XB)
    second = fx.table(1, NU, (1.0,), (row[3],), XA, XB) if family == 1 else fx.table(2, NU, (0.0, 1.0), (row[2], row[3]), XA, XB, raw=True)
    return [first, second]


def _mix(row, tables, normalise=True):
    """(value, band) of sum w_c^2 f_c (/ sum w_c^2) in fp64 from the component tables: what rho is taken from."""
    w2 = row[:2] ** 2
    den = w2.sum() if normalise else 1.0
    val = (w2[0] * tables[0].hi + w2[1] * tables[1].hi) / den
    return val, (w2[0] * tables[0].band + w2[1] * tables[1].band) / den + 2.0 * EPS * np.abs(val)


def _rho(band, against):
    """largest band / (eps |against|) over the entries with a band"""
    keep = band > 0
    assert (against[keep] > 0).all()
    return float((band[keep] / (EPS * against[keep])).max())


@functools.lru_cache(maxsize=None)
def reference(family, n, b):
    """Everything one draw is held to, in long double from the exact entries."""
    x, y, rows, sites = make_case(family, n)
    row, X = rows[b], x[:, None]
    gram = _component_tables(family, row, x, x)
    Rc = [T.longdouble() for T in gram]
    val, band = _mix(row, gram)
    off = band * (1.0 - np.eye(n))                                            # the device's diagonal is exactly 1
    out = {"rho": _rho(off, val)}
    # mode 0
    s2 = S2_TAU2[0]
    p0 = orc.loglik_grad_parts(X, y, row, 2, 1, s2, np.longdouble, Rc=Rc)
    k0 = orc.cond1(p0["Sigma"], p0["Sinv"])
    s_ll, s_beta = orc.loglik_beta_scales(p0, y)
    unit = EPS * k0 * (1.0 + out["rho"])
    out["mode0"] = (float(p0["loglik"]), float(p0["beta"]), unit * s_ll, unit * s_beta, k0)
    # mode 1
    p1 = orc.marginal_parts(X, y, row, 2, 1, s2, S2_TAU2[1], np.longdouble, Rc=Rc)
    out["mode1"] = (float(p1["loglik"]), orc.marginal_unit(p1, X, row, 2, 1, rho=out["rho"]), orc.cond1(p1["Sigma"], p1["Sinv"]))
    # tables: r un-normalised under family 2, as its script leaves it
    f = orc.predict_factor(X, y, row, 2, 1, np.longdouble, Rc=Rc)
    cross = _component_tables(family, row, sites, x)
    rval, rband = _mix(row, cross, normalise=family != 2)
    aL = np.abs(np.asarray(f["L"], dtype=np.float64))
    rho_t = np.array([_rho(rband[t], rval[t]) for t in range(len(sites))])
    parts = orc.predict_parts(X, y, row, 2, 1, SIGMA2, sites[:, None], np.longdouble, factor=f, rc=[T.longdouble() for T in cross],
                              raw_r=family == 2, rho=_rho(off, aL @ aL.T), rho_t=rho_t)
    out["predict"] = (parts, orc.predict_bands(parts, SIGMA2, orc.PREDICT_TOL_C), orc.cond1(f["R"], f["Rinv"]))
    return out


def _family(handle, family):
    from ccgp_amd import api
    handle.set_kernel(api.KERNEL_MATERN if family == 1 else api.KERNEL_MATERN_SPLINE, NU)


def _sweep(t):
    assert t["fused"][1] == 0 and t["diag"][1] > 0, t                         # these families exist on the blocked sweep only


def _note(tag, ratio):
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float(ratio))


# ----------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("family,n", CASES)
def test_likelihoods_exact(handle, family, n):
    from ccgp_amd import api
    x, y, rows, _ = make_case(family, n)
    s2, tau2 = S2_TAU2
    try:
        _family(handle, family)
        (ll0, beta0, st0), t0 = _timed(handle, lambda: handle.loglik_batch(x[:, None], y, 2, rows, s2, 0, 0.0))
        (ll1, beta1, st1), t1 = _timed(handle, lambda: handle.loglik_batch(x[:, None], y, 2, rows, s2, 1, tau2))
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    _sweep(t0)
    _sweep(t1)
    assert not st0.any() and not st1.any()
    for b in range(2):
        ref = reference(family, n, b)
        ll_ref, beta_ref, unit_ll, unit_beta, kappa = ref["mode0"]
        assert kappa <= KAPPA_MAX, (family, n, b, kappa)
        r = check_loglik_beta(ll_ref, beta_ref, unit_ll, unit_beta, ll0[b], beta0[b], "family%d/mode0" % family)
        _note("family%d/mode0 (of GRAD_TOL_C = %g)" % (family, orc.GRAD_TOL_C), max(r))
        ll_ref, unit, kappa1 = ref["mode1"]
        assert kappa1 <= orc.MARGINAL_COND_MAX, (family, n, b, kappa1)
        assert beta1[b] == 0.0
        ratio = abs(ll1[b] - ll_ref) / unit
        print("family %d n %d draw %d rho %.3g: mode 0 %.3g, %.3g (cond1 %.3g); mode 1 %.3g units (cond1 %.3g)" % (
            family, n, b, ref["rho"], r[0], r[1], kappa, ratio, kappa1))
        _note("family%d/mode1 (of MARGINAL_TOL_C = %g)" % (family, orc.MARGINAL_TOL_C), ratio)
        assert ratio <= orc.MARGINAL_TOL_C, (family, n, b, ll1[b], ll_ref, ratio)


@pytest.mark.parametrize("family,n", CASES)
def test_predict_tables_exact(handle, family, n):
    from ccgp_amd import api
    x, y, rows, sites = make_case(family, n)
    try:
        _family(handle, family)
        (mean, var, beta, st), t = _timed(handle, lambda: handle.predict_batch(x[:, None], y, 2, rows, sites[:, None], SIGMA2))
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    _sweep(t)
    assert not np.asarray(st).any() and mean.shape == (2, 3) and var.shape == (2, 3)
    C = orc.PREDICT_TOL_C
    for b in range(2):
        parts, band, kappa = reference(family, n, b)["predict"]
        assert kappa <= KAPPA_MAX, (family, n, b, kappa)
        e_var = np.abs(var[b] - np.asarray(parts["var"], dtype=np.float64)) / band["var"]
        e_mean = np.abs(mean[b] - np.asarray(parts["mean"], dtype=np.float64)) / band["mean"]
        e_beta = abs(beta[b] - float(parts["beta"])) / band["beta"]
        print("family %d n %d draw %d cond1 %.3g rho %.3g rho_t %s: var %.3g mean %.3g beta %.3g (x band / C)" % (
            family, n, b, kappa, parts["rho"], np.array2string(parts["rho_t"], precision=3), e_var.max() * C, e_mean.max() * C, e_beta * C))
        for name, e in (("var", e_var.max()), ("mean", e_mean.max()), ("beta", e_beta)):
            _note("family%d/%s (of PREDICT_TOL_C = %g)" % (family, name, C), e * C)
        assert (e_var <= 1.0).all() and (e_mean <= 1.0).all() and e_beta <= 1.0, (family, n, b, e_var, e_mean, e_beta)


def test_zz_report_headroom():
    for k in sorted(MAX_RATIO):
        print("max ratio %-44s %.3g" % (k, MAX_RATIO[k]))
