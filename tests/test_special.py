"""Host-side quadrature nodes of likeli.hyperpars (HX:554-556): Halton base 2 and the
inverse-gamma quantile, checked against scipy (no GPU needed: these are host functions)."""
import numpy as np
import scipy.stats as sst

from ccgp_amd import api
from oracle import ccgp_oracle as orc


def test_halton_first_terms_and_oracle():
    u = api.halton_base2(1728)
    assert u[:7].tolist() == [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875]
    np.testing.assert_array_equal(u, orc.runif_halton(1728))
    assert len(set(u.tolist())) == 1728 and u.min() > 0 and u.max() < 1


def test_qigamma_matches_scipy_on_every_grid_shape():
    u = api.halton_base2(1728)
    for alpha in (3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 11.0):
        for beta in (1.0, 4.0, 28.0, 250.0):
            got = api.qigamma(u, alpha, beta)
            want = sst.invgamma.ppf(u, alpha, scale=beta)
            np.testing.assert_allclose(got, want, rtol=2e-13, atol=0)
            np.testing.assert_allclose(got, orc.qigamma(u, alpha, beta), rtol=2e-13)


def test_qigamma_tails_and_small_shape():
    # pscl::qigamma is 1/qgamma(1 - p, ...): the 1 - p is formed in double first (HX:555), so the
    # yardstick for tiny p is qgamma at that rounded argument, not invgamma.ppf(p).
    p = np.array([1e-12, 1e-6, 0.5, 1 - 1e-6, 1 - 1e-12])
    for alpha in (0.3, 1.0, 2.5, 50.0):
        want = 2.0 / sst.gamma.ppf(1.0 - p, alpha)
        np.testing.assert_allclose(api.qigamma(p, alpha, 2.0), want, rtol=1e-10)


MATERN_NUS = (1.0001, 1.01, 1.1, 1.5, 2.0, 2.5, 5.0, 7.3, 10.0)      # ccgp_set_kernel accepts 1 < nu <= 10


def matern_rule(nu, z2):
    """csrc/ccgp_internal.h matern_corr, statement by statement, in libm arithmetic; takes z^2 as the kernel does."""
    import math
    if not z2 > 9e-20:
        return 1.0 if z2 == z2 else z2
    if z2 <= 1e-10 and nu >= 1.5:
        return 1.0 - z2 / (4.0 * (nu - 1.0))
    z = math.sqrt(z2)
    hs = 0.15 / max(1.0, math.sqrt(z))
    s = 0.5
    for k in range(1, 6000):
        t = k * hs
        et = math.exp(t)
        c1 = 0.5 * (et + 1.0 / et) - 1.0
        g = 0.5 * (math.exp(nu * t - z * c1) + math.exp(-nu * t - z * c1))   # exponents formed first: no overflow
        s += g
        if g < 1e-17 * s and nu * t < z * c1:
            break
    norm = 1.0 / (math.gamma(nu) * 2.0 ** (nu - 1.0))
    return math.exp(nu * math.log(z) - z) * (hs * s * norm)


def test_matern_quadrature_rule_of_the_device_kernel():
    """ccgp_internal.h matern_corr: z^nu K_nu(z) / (Gamma(nu) 2^(nu-1)) by the trapezoidal rule on
    int_0^inf exp(-z cosh t) cosh(nu t) dt with step 0.15 / max(1, sqrt z), exactly 1 up to z = 3e-10 and the two-term
    series up to z = 1e-5 for nu >= 1.5.  The same rule in libm arithmetic against a 40-digit evaluation, for every nu
    of MATERN_NUS and z from 1e-9 to 740, both sides of every switch included: 5e-14 relative, plus 4 eps z beyond
    z = 200 (the conditioning of exp(-z)), plus two quanta where the value is subnormal.  The kernel itself is held
    to the same band by tests/test_gpu_family_corr_exact.py."""
    import math
    import mpmath as mp

    eps = 2.0 ** -52
    zs = np.concatenate([np.logspace(-9, math.log10(740.0), 56),
                         [3e-10 * (1 - 1e-9), 3e-10 * (1 + 1e-9), 1e-5 * (1 - 1e-9), 1e-5 * (1 + 1e-9), 1.0 - 1e-12, 1.0 + 1e-12,
                          0.3, 7.7, 33.3, 200.0, 300.0, 700.0, 740.0]])
    worst = 0.0
    assert matern_rule(2.5, 0.0) == 1.0 and math.isnan(matern_rule(2.5, float("nan")))
    with mp.workdps(40):
        for nu in MATERN_NUS:
            for z in zs:
                z2 = float(z) * float(z)
                zz = mp.sqrt(mp.mpf(z2))                                           # the rule sees z^2
                want = zz ** nu * mp.besselk(nu, zz) / (mp.gamma(nu) * mp.mpf(2) ** (mp.mpf(nu) - 1))
                band = (5e-14 + (4.0 * eps * float(zz) if zz > 200 else 0.0)) * want + (2 * mp.mpf(2) ** -1074 if want < 2.3e-308 else 0)
                err = abs(mp.mpf(matern_rule(nu, z2)) - want)
                worst = max(worst, float(err / band))
                assert err <= band, (nu, float(z), float(err / band))
    print("matern rule: largest |d| / band %.3g" % worst)
