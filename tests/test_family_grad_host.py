"""tests/family_grad_exact.py's references and bands, without a GPU: d corr / d theta of the Matern and spline families
(csrc/ccgp_internal.h matern_corr_grad, spline_corr_grad) restated in libm arithmetic.

  * the Matern rule lies inside its band for every nu of family_exact.NUS over family_exact.sweep_z, from the 9e-20 switch up;
    below the switch, where the kernel returns exactly 0, the true derivative is at most 2.1e-18 / theta;
  * the spline rule lies inside its band across both branches, the knots and beyond;
  * the closed-form gradient built in long double from these derivative tables equals central differences of the long-double
    likelihood built from family_exact.table at theta (1 +- 1e-4) to 1e-6 relative: the difference quotient's own truncation
    error (h^2 / 6 times the third logarithmic derivative), and a wrong sign or a missing factor is an error of order one;
  * the band rejects the derivative of matern_corr's two-term series at nu = 1.5, z = 1e-6 (off by a relative z = 1e-6).
"""
import math

import mpmath as mp
import numpy as np

import family_exact as fx
import family_grad_exact as gx
from oracle import ccgp_oracle as orc


def test_matern_rule_lies_inside_the_band_from_the_switch_up():
    worst = 0.0
    with mp.workdps(fx.DPS):
        for nu in fx.NUS:
            for z in fx.sweep_z(nu):
                z2 = float(z) * float(z)
                if not z2 > gx.SWITCH_Z2:
                    continue
                for theta in fx.SWEEP_THETAS:   # 0.0037: the factor behind exp() exceeds 1 where the value is subnormal
                    got = gx.matern_grad_rule(nu, z2, theta)
                    ref = gx.matern_dtheta_f(nu, mp.mpf(float(z)), mp.mpf(theta))
                    band = gx.matern_band(nu, mp.mpf(float(z)), ref)
                    ratio = float(abs(mp.mpf(got) - ref) / band)
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (nu, z, theta, got, float(ref), ratio)
    print("Matern derivative rule: largest |rule - ref| / band %.3g" % worst)


def test_below_the_switch_the_true_derivative_is_negligible():
    with mp.workdps(fx.DPS):
        for nu in fx.NUS:
            z = mp.sqrt(mp.mpf(gx.SWITCH_Z2))
            assert gx.matern_dtheta_f(nu, z, mp.mpf(1)) <= gx.BELOW_SWITCH, nu
            assert gx.matern_grad_rule(nu, gx.SWITCH_Z2, 0.5) == 0.0 and gx.matern_grad_rule(nu, 0.0, 0.5) == 0.0
    assert math.isnan(gx.matern_grad_rule(2.5, math.nan, 0.5)) and math.isnan(gx.spline_grad_rule(math.nan, 0.5))


def test_spline_rule_lies_inside_the_band():
    worst = 0.0
    for theta in (1.0, 0.3):
        hs = list(np.linspace(0.0, 1.2, 49) * theta)
        for knot in (theta / 2.0, theta):
            hs += [np.nextafter(knot, 0.0), knot, np.nextafter(knot, 2.0)]
        hs.append(theta * (1.0 + 8.0 * fx.EPS))
        for h in hs:
            ref, band, u = gx.spline_dtheta(theta, fx.frac(h))
            got = gx.spline_grad_rule((1.0 / (theta * theta)) * (float(h) * float(h)), theta)
            err = abs(fx.frac(got) - ref)
            assert err <= band, (theta, h, got, float(ref), float(band))
            if band > 0:
                worst = max(worst, float(err / band))
            if u >= 1 + 4 * fx.frac(fx.EPS):
                assert got == 0.0
    print("spline derivative rule: largest |rule - ref| / band %.3g" % worst)


def _case(family):
    rng = np.random.default_rng(40 + family)
    n = 8
    x = (np.arange(n) + rng.uniform(0.2, 0.8, n)) / n
    y = np.sin(9.0 * x) + 0.3 * np.cos(31.0 * x) + 0.3 * x
    row = np.array([0.75, 0.5, 2.4 / n, (2.9 if family == 1 else 3.6) / n])
    return x, y, row


def _components(family, nu, thetas, x):
    return [fx.table(1, nu, (1.0,), (thetas[0],), x, x).longdouble(),
            (fx.table(1, nu, (1.0,), (thetas[1],), x, x) if family == 1 else
             fx.table(2, nu, (0.0, 1.0), (thetas[0], thetas[1]), x, x, raw=True)).longdouble()]


def test_closed_form_gradient_equals_central_differences():
    orc.require_extended_precision()
    nu, s2, K, rel = 2.5, 1.3, 2, 1e-4
    for family in (1, 2):
        x, y, row = _case(family)
        X = x[:, None]

        def loglik(r):
            return orc.loglik_grad_parts(X, y, r, K, 1, s2, np.longdouble, Rc=_components(family, nu, r[K:], x))["loglik"]

        parts = orc.loglik_grad_parts(X, y, row, K, 1, s2, np.longdouble, Rc=_components(family, nu, row[K:], x))
        Dc = [gx.dtable(family, nu, row[K:], q, x, x).longdouble() for q in range(K)]
        grad, scale, _ = gx.family_grad_from_parts(parts, row, K, Dc, s2)
        for j in range(2 * K):
            up, dn = row.copy(), row.copy()
            up[j], dn[j] = row[j] * (1.0 + rel), row[j] * (1.0 - rel)
            fd = (loglik(up) - loglik(dn)) / np.longdouble(up[j] - dn[j])
            err = abs(float(fd - grad[j])) / abs(float(grad[j]))
            print("family %d column %d: closed form %.12g, central difference %.12g, relative difference %.3g" % (
                family, j, float(grad[j]), float(fd), err))
            assert err <= 1e-6, (family, j, float(grad[j]), float(fd))


def test_the_band_rejects_the_series_derivative():
    nu, z, theta = 1.5, 1e-6, 0.5
    with mp.workdps(fx.DPS):
        ref = gx.matern_dtheta_f(nu, mp.mpf(z), mp.mpf(theta))
        band = gx.matern_band(nu, mp.mpf(z), ref)
        wrong = gx.series_grad(nu, z * z, theta)
        right = gx.matern_grad_rule(nu, z * z, theta)
        assert abs(mp.mpf(right) - ref) <= band
        assert abs(mp.mpf(wrong) - ref) > 1e6 * band, (wrong, float(ref), float(band))
