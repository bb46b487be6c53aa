"""fit.Metro_device_sets' driver without a GPU: on_device=False with an analytic `logpost_sets_fn`.  What is held: a chain is
the plain sequential loop written here over the stream the contract names (blocks of u, then z; e = L z left to right; log u
by math.log), with the same bits whatever `seg` cuts it into and whether it runs alone or among others; the generator is left
exactly after ceil(proposals / block) blocks; and each of the three stops -- Geweke, N, max_proposals -- is reached."""
import math

import numpy as np
import pytest
from scipy.stats import norm

from ccgp_amd import fit

CENTRES = np.array([[0.3, -0.2, 0.1], [-0.4, 0.5, 0.0], [0.0, 0.1, -0.3]])
BLOCK = 32


def analytic(rows, set_of):
    """A Gaussian log-density per set, with a hole: rows whose first coordinate exceeds centre + 2.5 are not finite."""
    rows = np.atleast_2d(rows)
    c = CENTRES[np.asarray(set_of)]
    val = -0.5 * ((rows - c) ** 2 / np.array([0.5, 1.0, 2.0])).sum(axis=1)
    val = np.where(rows[:, 0] > c[:, 0] + 2.5, np.nan, val)
    return val, rows.sum(axis=1)


def estimate(c):
    return dict(mode=CENTRES[c].copy(), var=np.diag([0.5, 1.0, 2.0]) + 0.1, converged=True, value=0.0)


def sequential(c, seed, N, samp_size, batch_size, alpha, max_proposals):
    """The chain of set c as the contract states it, one proposal at a time."""
    rng = np.random.default_rng(seed)
    est = estimate(c)
    L = np.linalg.cholesky(math.sqrt(2.0) * est["var"])
    theta = est["mode"].copy()
    l = float(analytic(theta[None], [c])[0][0])
    samp, betas, k, pv, t = np.zeros((N, 3)), np.zeros(N), 0, 0.0, 0
    us, zs = None, None
    while k < N and pv < alpha and t < max_proposals:
        if t % BLOCK == 0:
            us, zs = rng.random(BLOCK), rng.standard_normal((BLOCK, 3))
        z = zs[t % BLOCK]
        e = np.array([L[0, 0] * z[0], L[1, 0] * z[0] + L[1, 1] * z[1], L[2, 0] * z[0] + L[2, 1] * z[1] + L[2, 2] * z[2]])
        logu = math.log(us[t % BLOCK])
        cand = theta + e
        val, beta = analytic(cand[None], [c])
        t += 1
        if math.isfinite(val[0]) and (val[0] - l) > logu:
            samp[k], betas[k] = cand, beta[0]
            theta, l, k = cand, float(val[0]), k + 1
            if k >= samp_size and k % batch_size == 0:
                try:
                    pv = float(2.0 * (1.0 - norm.cdf(abs(fit.geweke_z(samp[k - samp_size:k, 0])))))
                except Exception:
                    pv = 0.0
    return dict(sample=samp[k - samp_size:k], beta=betas[k - samp_size:k], accepted=k, proposals=t, geweke_p=pv,
                state=rng.bit_generator.state)


def run(cs, seeds, seg, **kw):
    rngs = [np.random.default_rng(s) for s in seeds]
    r = fit.Metro_device_sets(None, None, kw["N"], kw["samp_size"], kw["batch_size"], kw["alpha"], [None] * len(cs),
                              [1.0] * len(cs), [None] * len(cs), rngs=rngs, max_proposals=kw["max_proposals"],
                              laplace=[estimate(c) for c in cs], block=BLOCK, seg=seg, on_device=False,
                              logpost_sets_fn=lambda rows, set_of: analytic(rows, np.asarray(cs)[np.asarray(set_of)]))
    return r, [g.bit_generator.state for g in rngs]


# the Geweke stop (alpha small enough to be met at the first look), the N stop (alpha never met), the max_proposals stop
SETTINGS = {
    "geweke": dict(N=400, samp_size=40, batch_size=10, alpha=1e-12, max_proposals=5000),
    "N": dict(N=60, samp_size=40, batch_size=10, alpha=2.0, max_proposals=5000),
    "max_proposals": dict(N=400, samp_size=40, batch_size=10, alpha=2.0, max_proposals=170),
}


@pytest.fixture(scope="module")
def references():
    return {name: [sequential(c, 11 + c, **kw) for c in range(3)] for name, kw in SETTINGS.items()}


def same(ch, ref, state):
    assert ch["accepted"] == ref["accepted"] and ch["proposals"] == ref["proposals"] and ch["geweke_p"] == ref["geweke_p"]
    assert np.array_equal(ch["sample"], ref["sample"]) and np.array_equal(ch["beta"], ref["beta"])
    assert state == ref["state"]


@pytest.mark.parametrize("seg", [1, 7, 2048])
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_chain_is_the_sequential_loop(references, name, seg):
    kw, refs = SETTINGS[name], references[name]
    r, states = run([0, 1, 2], [11, 12, 13], seg, **kw)
    for c in range(3):
        same(r["chains"][c], refs[c], states[c])
    r1, st1 = run([1], [12], seg, **kw)   # alone
    same(r1["chains"][0], refs[1], st1[0])


@pytest.mark.parametrize("seg", [1, 7, 2048])
def test_every_stop_is_reached(seg):
    """The driver's own chains: each of the three stops is what ended them, and the generator stands after whole blocks."""
    got = {}
    for name, kw in SETTINGS.items():
        r, states = run([0], [11], seg, **kw)
        got[name] = ch = r["chains"][0]
        # the generator stands after whole blocks: ceil(proposals / block) of them
        rng = np.random.default_rng(11)
        for _ in range(-(-ch["proposals"] // BLOCK)):
            rng.random(BLOCK)
            rng.standard_normal((BLOCK, 3))
        assert rng.bit_generator.state == states[0], name
        assert ch["sample"].shape == (kw["samp_size"], 3)
    g, n, m = got["geweke"], got["N"], got["max_proposals"]
    kw = SETTINGS["geweke"]
    assert g["geweke_p"] >= kw["alpha"] and kw["samp_size"] <= g["accepted"] < kw["N"] and g["accepted"] % kw["batch_size"] == 0
    assert g["proposals"] < kw["max_proposals"]
    assert n["accepted"] == SETTINGS["N"]["N"] and n["proposals"] < SETTINGS["N"]["max_proposals"] and n["geweke_p"] < 2.0
    assert m["proposals"] == SETTINGS["max_proposals"]["max_proposals"] and m["accepted"] < SETTINGS["max_proposals"]["N"]


def test_metro_device_is_the_one_set_case(references):
    kw = SETTINGS["N"]
    rng = np.random.default_rng(12)
    ch = fit.Metro_device(None, None, kw["N"], kw["samp_size"], kw["batch_size"], kw["alpha"], None, 1.0, None, rng=rng,
                          max_proposals=kw["max_proposals"], laplace=estimate(1), block=BLOCK, seg=19,
                          logpost_fn=lambda rows: analytic(rows, np.ones(len(rows), dtype=int)))
    same(ch, references["N"][1], rng.bit_generator.state)
