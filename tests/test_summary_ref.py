"""The yardstick of the prediction summaries (tests/summary_ref.py) against mpmath at 50 digits, before any GPU run relies
on it; and the three C entry points in the Python binding."""
import mpmath as mp
import numpy as np
import pytest

import summary_ref as ref
from ccgp_amd import api

LEVELS = (1e-9, 0.025, 0.5, 0.975, 1.0 - 1e-9)

# S in {1, 2, 7}; the last two hold a component with sigma = 0
MIXTURES = {
    "S1": (np.array([0.3]), np.array([1.7])),
    "S2": (np.array([-1.0, 2.5]), np.array([0.5, 0.02])),
    "S7": (np.array([10.2, 9.7, 10.0, 11.5, 10.1, 9.9, 10.4]), np.array([0.3, 0.05, 1.2, 0.4, 0.01, 0.7, 0.25])),
    "S2_point": (np.array([1.0, 1.5]), np.array([0.0, 0.3])),
    "S7_point": (np.array([0.2, -0.7, 0.0, 1.5, 0.1, -0.1, 0.4]), np.array([0.3, 0.0, 1.2, 0.4, 0.01, 0.7, 0.25])),
}


def mp_tail(q, mu, sd, upper):
    """F(q) (upper False) or 1 - F(q) of the mixture at 50 digits; q, mu, sd are the doubles themselves."""
    mp.mp.dps = 50
    tot = mp.mpf(0)
    for m_, s_ in zip(mu, sd):
        d = mp.mpf(float(q)) - mp.mpf(float(m_))
        if s_ == 0.0:
            below = 1 if d >= 0 else 0
            tot += (1 - below) if upper else below
        else:
            z = d / mp.mpf(float(s_)) / mp.sqrt(2)
            tot += mp.erfc(z) / 2 if upper else mp.erfc(-z) / 2
    return tot / len(mu)


@pytest.mark.parametrize("name", sorted(MIXTURES))
def test_tails_and_density_against_mpmath(name):
    mu, sd = MIXTURES[name]
    mp.mp.dps = 50
    for q in np.concatenate([mu - 6.0 * np.maximum(sd, 0.1), mu + 0.37 * sd + 0.01, mu + 6.0 * np.maximum(sd, 0.1)]):
        # ndtr is a few ulp of its value; the rounding of z = (q - mu) / sd moves Phi by z^2 eps relative (z <= ~60 here
        # only where the term is negligible in the sum; the terms that carry a tail have z <= 7): 256 eps covers both
        for upper, got in ((False, ref.cdf(q, mu, sd)), (True, ref.sf(q, mu, sd))):
            want = mp_tail(q, mu, sd, upper)
            assert abs(mp.mpf(got) - want) <= 256 * ref.EPS * want + mp.mpf(10) ** -300, (name, q, upper, got, want)
        dens = sum(mp.exp(-((mp.mpf(float(q)) - mp.mpf(float(m_))) / mp.mpf(float(s_))) ** 2 / 2) /
                   (mp.mpf(float(s_)) * mp.sqrt(2 * mp.pi)) for m_, s_ in zip(mu, sd) if s_ > 0) / len(mu)
        assert abs(mp.mpf(ref.pdf(q, mu, sd)) - dens) <= 256 * ref.EPS * dens + mp.mpf(10) ** -300


@pytest.mark.parametrize("name", sorted(MIXTURES))
@pytest.mark.parametrize("p", LEVELS)
def test_quantile_against_mpmath(name, p):
    """q = inf{q : F(q) >= p}: at 50 digits F must not have reached p a few ulp below q and must have reached it a few
    ulp above, up to the reference's own relative error on the tail it works on (256 eps, as above)."""
    mu, sd = MIXTURES[name]
    q = ref.quantile(p, mu, sd)
    d = 4.0 * ref.ulp(q)
    upper = p > 0.5
    tgt = mp.mpf(1) - mp.mpf(p) if upper else mp.mpf(p)     # exact: p is a double
    slack = 256 * ref.EPS * tgt
    below, above = mp_tail(q - d, mu, sd, upper), mp_tail(q + d, mu, sd, upper)
    if upper:   # the survival function falls
        assert below >= tgt - slack and above <= tgt + slack, (name, p, q, below, above)
    else:
        assert below <= tgt + slack and above >= tgt - slack, (name, p, q, below, above)
    res, tol = ref.quantile_residual(q, p, mu, sd)
    assert res <= tol


def test_point_mass_quantile_is_the_point():
    mu, sd = np.array([2.5]), np.array([0.0])
    for p in LEVELS:
        assert ref.quantile(p, mu, sd) == 2.5
    assert ref.cdf(2.5, mu, sd) == 1.0 and ref.cdf(np.nextafter(2.5, 0.0), mu, sd) == 0.0


def test_summarize_definition():
    rng = np.random.default_rng(3)
    mean, var = rng.normal(size=(6, 2)), rng.uniform(-0.01, 1.0, size=(6, 2))
    status = np.array([0, 0, 1, 0, 0, 0])
    s = ref.summarize(mean, var, status, [0.5], y_at=[0.1, -0.2])
    ok = status == 0
    np.testing.assert_allclose(s["y_hat"], mean[ok].mean(axis=0), rtol=1e-15)
    v = np.maximum(var[ok], 0.0)
    np.testing.assert_allclose(s["pred_var"], v.mean(axis=0) + mean[ok].var(axis=0), rtol=1e-14)
    assert np.all((s["quant"] > 0) & (s["quant"] < 1)) and np.all((s["cdf_at"] > 0) & (s["cdf_at"] < 1))
    assert np.isnan(ref.summarize(mean, var, np.ones(6), [0.5])["quantiles"]).all()


def test_binding_declares_the_summary_entry_points():
    for name in ("ccgp_predict_summary", "ccgp_predict_summary_dev", "ccgp_summary_from_factorset"):
        assert name in api.SIGNATURES
        assert hasattr(api.lib(), name)
    assert callable(api.Handle.predict_summary) and callable(api.Handle.predict_summary_dev)
    assert callable(api.FactorSet.summary)
