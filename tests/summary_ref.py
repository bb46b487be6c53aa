"""Reference for the posterior-predictive summaries (ccgp_predict_summary): the definition, in numpy / scipy, from given
S x m tables.  Per site, over the draws with status == 0 (S' of them):

    sigma_s = sqrt(max(var_s, 0)),   F(q) = 1/S' sum_s Phi((q - mu_s) / sigma_s)   (sigma_s = 0: a step at mu_s)
    y_hat = mean(mu),  pred_var = mean(sigma^2) + mean((mu - y_hat)^2),  quant = 1 - F(y_hat),  cdf_at = F(y_at)
    q_p = inf{q : F(q) >= p}

Both tails go through erfc (scipy's ndtr does so): p <= 1/2 is solved on F, p > 1/2 on the survival function.
tests/test_summary_ref.py validates this file against mpmath at 50 digits.
"""
import numpy as np
from scipy.special import ndtr

EPS = np.finfo(np.float64).eps
_SQRT_2PI = np.sqrt(2.0 * np.pi)


def _z(q, mu, sd):
    """(q - mu) / sd with the step convention for sd = 0: +inf where q >= mu, -inf below."""
    pos = sd > 0.0
    d = q - mu
    z = np.where(d >= 0.0, np.inf, -np.inf)
    np.divide(d, sd, out=z, where=pos)
    return z


def cdf(q, mu, sd):
    return float(np.mean(ndtr(_z(q, mu, sd))))


def sf(q, mu, sd):
    return float(np.mean(ndtr(-_z(q, mu, sd))))


def pdf(q, mu, sd):
    pos = sd > 0.0
    z = (q - mu[pos]) / sd[pos]
    return float(np.sum(np.exp(-0.5 * z * z) / (sd[pos] * _SQRT_2PI)) / mu.size)


def _reached(q, p, mu, sd):
    """F(q) >= p, evaluated on the tail that keeps its digits."""
    return cdf(q, mu, sd) >= p if p <= 0.5 else sf(q, mu, sd) <= 1.0 - p


def quantile(p, mu, sd):
    """inf{q : F(q) >= p} to adjacent doubles: bracket from min / max of mu -+ 9 sd, widened geometrically, bisection."""
    lo, hi = float(np.min(mu - 9.0 * sd)), float(np.max(mu + 9.0 * sd))
    step = max(hi - lo, max(abs(lo), abs(hi)) * 2.0 ** -30, 1e-300)
    for _ in range(64):
        if not _reached(lo, p, mu, sd):
            break
        lo -= step
        step *= 4.0
    for _ in range(64):
        if _reached(hi, p, mu, sd):
            break
        hi += step
        step *= 4.0
    assert not _reached(lo, p, mu, sd) and _reached(hi, p, mu, sd)
    for _ in range(2200):
        mid = lo + 0.5 * (hi - lo)
        if not lo < mid < hi:
            break
        if _reached(mid, p, mu, sd):
            hi = mid
        else:
            lo = mid
    return hi


def ulp(x):
    return float(np.spacing(abs(x))) if x != 0.0 else float(np.finfo(np.float64).tiny)


def quantile_residual(q, p, mu, sd):
    """The acceptance criterion of a quantile q for level p, step CDFs included.  With delta = 4 ulp(q) and f the mixture
    density at q:   F(q - delta) - tol <= p <= F(q + delta) + tol,   tol = 64 eps + 4 ulp(q) f.
    Returns (residual, tol): residual = max(F(q - delta) - p, p - F(q + delta)), to be <= tol.  For p > 1/2 the same
    inequalities are evaluated on the survival function (identical in exact arithmetic, more digits in the reference)."""
    delta = 4.0 * ulp(q)
    tol = 64.0 * EPS + 4.0 * ulp(q) * pdf(q, mu, sd)
    if p <= 0.5:
        res = max(cdf(q - delta, mu, sd) - p, p - cdf(q + delta, mu, sd))
    else:
        res = max((1.0 - p) - sf(q - delta, mu, sd), sf(q + delta, mu, sd) - (1.0 - p))
    return res, tol


def summarize(mean, var, status, probs, y_at=None):
    """mean, var: [S, m]; status: [S].  Returns the dict of Handle.predict_summary (without beta)."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ok = np.asarray(status) == 0
    m = mean.shape[1]
    probs = np.ravel(np.asarray(probs, dtype=np.float64))
    out = dict(y_hat=np.full(m, np.nan), pred_var=np.full(m, np.nan), quant=np.full(m, np.nan),
               cdf_at=np.full(m, np.nan), quantiles=np.full((m, probs.size), np.nan))
    if not ok.any():
        return out
    for t in range(m):
        mu, v = mean[ok, t], np.maximum(var[ok, t], 0.0)
        sd = np.sqrt(v)
        y_hat = float(np.mean(mu))
        out["y_hat"][t] = y_hat
        out["pred_var"][t] = float(np.mean(v)) + float(np.mean((mu - y_hat) ** 2))
        out["quant"][t] = sf(y_hat, mu, sd)
        if y_at is not None:
            out["cdf_at"][t] = cdf(float(y_at[t]), mu, sd)
        for j, p in enumerate(probs):
            out["quantiles"][t, j] = quantile(float(p), mu, sd)
    return out
