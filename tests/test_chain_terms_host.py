"""The portable log-posterior terms (csrc/chain_terms.h, ccgp_chain_terms) against a 40-digit mpmath evaluation, without a GPU.
The chain kernel computes the parameter row, the log-Jacobian and the log-prior with an exp and a log built from exactly
rounded operations so that host and device agree in every bit; here the host side of that arithmetic is held to the true
values, output by output, for all four priors.

Bands (component-wise, first order, no condition number):
  * exp-derived row entries (p, theta1, theta2, (1 + lambda) theta): 2 ulp of the reference value -- a table value rounded
    once plus one fma rounding plus a reduction error below 1e-19 is about 1 ulp, doubled;
  * sums (ljac, lprior, 1 - p): 8 eps sum |summand|, the summands being the exact terms of the sum.
glibc's arithmetic -- logpost_terms of capi.hip restated in numpy -- runs on the same inputs; `pytest -s` prints both maxima as
fractions of the band (DESIGN.md records them)."""
import math

import mpmath as mp
import numpy as np
import pytest

from ccgp_amd import api

mp.mp.dps = 40
EPS = 2.0 ** -52
PRIORS = {"INVGAMMA": api.PRIOR_INVGAMMA, "GV": api.PRIOR_GV, "ISO": api.PRIOR_ISO, "ANI": api.PRIOR_ANI}
PARS = (7.0, 3.0, 3.0, 28.0)
TINY = 4.9406564584124654e-324


def inputs(q):
    rng = np.random.default_rng(20261020)
    t = rng.uniform(-40.0, 40.0, size=(400, q))
    edge = [0.0, TINY, -TINY, 1e-300, -1e-300, 40.0, -40.0, 1e-8, -1e-8, 0.5, -0.5]
    rows = [t]
    for j in range(q):
        for v in edge:
            r = rng.uniform(-3.0, 3.0, size=q)
            r[j] = v
            rows.append(r[None])
    return np.concatenate(rows)


def ulp(x):
    x = abs(float(x))
    return math.ulp(x) if x > 0.0 else TINY


def reference(prior, row, d):
    """Every output with its band: (name, value, band)."""
    psi1, psi2, phi = (mp.mpf(float(v)) for v in row[:3])
    th1, th2, en = mp.exp(psi1), mp.exp(psi2), mp.exp(-phi)
    p = 1 / (1 + en)
    out = [("p", p, 2 * ulp(p)), ("1-p", 1 - p, 8 * EPS * (1 + p))]
    lj_terms = [-phi, -2 * mp.log(1 + en), psi1, psi2]
    if prior == "ANI":
        zeta = mp.mpf(float(row[3]))
        lam = mp.exp(zeta)
        rates = [th1, th2, (1 + lam) * th1, (1 + lam) * th2]
        lj_terms.append(zeta)
        lp_terms = [-psi1, -psi1 * psi1 / 2, -psi2, -psi2 * psi2 / 2, -4 * zeta, -4 / lam]
    else:
        rates = [th1] * d + [th2] * d
        a1, b1, a2, b2 = {"INVGAMMA": PARS, "GV": (3, 1, 5, 75), "ISO": (3, 2, 5, 16)}[prior]
        lp_terms = [-(a1 + 1) * psi1, -b1 / th1, -(a2 + 1) * psi2, -b2 / th2]
    out += [("rate%d" % i, r, 2 * ulp(r)) for i, r in enumerate(rates)]
    out.append(("ljac", mp.fsum(lj_terms), 8 * EPS * float(mp.fsum(abs(v) for v in lj_terms))))
    out.append(("lprior", mp.fsum(lp_terms), 8 * EPS * float(mp.fsum(abs(v) for v in lp_terms))))
    return out


def glibc_terms(prior, T, d):
    """logpost_terms (capi.hip) in numpy: glibc's exp and log, the same order of operations."""
    psi1, psi2, phi = T[:, 0], T[:, 1], T[:, 2]
    with np.errstate(all="ignore"):
        th1, th2 = np.exp(psi1), np.exp(psi2)
        p = 1.0 / (1.0 + np.exp(-phi))
        lj = -phi - 2.0 * np.log(1.0 + np.exp(-phi)) + psi1 + psi2
        if prior == "ANI":
            zeta = T[:, 3]
            lam = np.exp(zeta)
            rates = [th1, th2, (1.0 + lam) * th1, (1.0 + lam) * th2]
            lj = lj + zeta
            lp = -psi1 - psi1 * psi1 / 2.0 - psi2 - psi2 * psi2 / 2.0 - 4.0 * zeta - 4.0 / lam
        else:
            rates = [th1] * d + [th2] * d
            a1, b1, a2, b2 = {"INVGAMMA": PARS, "GV": (3.0, 1.0, 5.0, 75.0), "ISO": (3.0, 2.0, 5.0, 16.0)}[prior]
            lp = -(a1 + 1.0) * psi1 - b1 / th1 - (a2 + 1.0) * psi2 - b2 / th2
    return np.column_stack([p, 1.0 - p] + rates), lj, lp


def worst(prior):
    """Largest |error| / band over the inputs for the portable terms and for glibc's: ({output: frac}, {output: frac})."""
    d = 2
    q = 4 if prior == "ANI" else 3
    T = inputs(q)
    rows, lj, lp = api.chain_terms(PRIORS[prior], d, T, PARS if prior == "INVGAMMA" else None)
    grows, glj, glp = glibc_terms(prior, T, d)
    mine, glibc = {}, {}
    for b, row in enumerate(T):
        ref = reference(prior, row, d)
        got = list(rows[b]) + [lj[b], lp[b]]
        gg = list(grows[b]) + [glj[b], glp[b]]
        assert len(ref) == len(got)
        for (name, val, band), g, g2 in zip(ref, got, gg):
            key = name[:4]
            mine[key] = max(mine.get(key, 0.0), float(abs(mp.mpf(float(g)) - val)) / band)
            glibc[key] = max(glibc.get(key, 0.0), float(abs(mp.mpf(float(g2)) - val)) / band)
    return mine, glibc


@pytest.mark.parametrize("prior", sorted(PRIORS))
def test_terms_within_bands(prior):
    mine, glibc = worst(prior)
    print(prior, "portable:", {k: round(v, 3) for k, v in mine.items()}, "glibc:", {k: round(v, 3) for k, v in glibc.items()})
    for k, v in mine.items():
        assert v <= 1.0, (prior, k, v)


def test_special_values():
    """NaN propagates, overflow gives +Inf, large negative arguments give 0; the sums follow IEEE arithmetic from there."""
    inf, nan = math.inf, math.nan
    T = np.array([[inf, 0.0, 0.0], [-inf, 0.0, 0.0], [nan, 0.0, 0.0], [0.0, 0.0, inf], [0.0, 0.0, -inf], [0.0, 0.0, nan],
                  [800.0, -800.0, 0.0], [0.0, 0.0, 0.0]])
    rows, lj, lp = api.chain_terms(api.PRIOR_GV, 1, T)
    assert rows[0, 2] == inf and rows[1, 2] == 0.0 and math.isnan(rows[2, 2])
    assert rows[3, 0] == 1.0 and rows[3, 1] == 0.0 and rows[4, 0] == 0.0 and rows[4, 1] == 1.0
    assert math.isnan(rows[5, 0]) and math.isnan(rows[5, 1]) and math.isnan(lj[5]) and math.isnan(lj[2]) and math.isnan(lp[2])
    assert rows[6, 2] == inf and rows[6, 3] == 0.0 and lp[6] == -inf
    assert rows[7, 0] == 0.5 and rows[7, 1] == 0.5 and rows[7, 2] == 1.0 and rows[7, 3] == 1.0
    assert lj[7] == -2.0 * math.log(2.0) and lp[7] == -76.0
    T4 = np.array([[0.0, 0.0, 0.0, inf], [0.0, 0.0, 0.0, -inf], [0.0, 0.0, 0.0, nan]])
    rows, lj, lp = api.chain_terms(api.PRIOR_ANI, 2, T4)
    assert rows[0, 4] == inf and lp[0] == -inf and rows[1, 4] == 1.0 and math.isnan(lp[1]) and math.isnan(rows[2, 4])   # +Inf - Inf


def test_refusals():
    L = api.lib()
    out = np.full(8, -7.0)
    t = np.zeros(3)
    p = api._p
    assert L.ccgp_chain_terms(9, 1, p(t), 1, None, p(out), p(out), p(out)) == -1
    assert L.ccgp_chain_terms(api.PRIOR_INVGAMMA, 1, p(t), 1, None, p(out), p(out), p(out)) == -1
    assert L.ccgp_chain_terms(api.PRIOR_ANI, 3, p(t), 1, None, p(out), p(out), p(out)) == -1
    assert L.ccgp_chain_terms(api.PRIOR_GV, 0, p(t), 1, None, p(out), p(out), p(out)) == -1
    assert L.ccgp_chain_terms(api.PRIOR_GV, 1, None, 1, None, p(out), p(out), p(out)) == -1
    assert (out == -7.0).all()
    assert L.ccgp_chain_terms(api.PRIOR_GV, 1, p(t), 0, None, p(out), p(out), p(out)) == 0
