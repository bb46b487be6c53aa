"""Cases for the device-chain tests (tests/test_gpu_chains.py): one shape per CHAIN instance of small_reg_kernel -- n = 2, 16,
17, 48, 50, 64, 65, 90, 128 and 32, 40, 80, 96, 100, 112, 120 are the general and the FULL instance (the exact multiples of 16)
of every NB = 1 .. 8 on the 16 x 16 grid -- over the four priors.  A case is a training set, a start state and T pre-drawn proposals (increments and log-uniforms).  The seeds and step
scales below were chosen on the CPU with the oracle's logpost (`python tests/chain_cases.py` prints each case's acceptances
and rejections under the oracle) so that every case has at least 5 of each; the GPU test asserts that from the device trace."""
import math

import numpy as np

from conftest import load_gv
from ccgp_amd import api

T = 60
PARS = (7.0, 3.0, 3.0, 28.0)   # the inverse-gamma prior's (a1, b1, a2, b2)
PRIOR_ID = {"HX": api.PRIOR_INVGAMMA, "GV": api.PRIOR_GV, "ISO": api.PRIOR_ISO, "ANI": api.PRIOR_ANI}
# (n, d, script, seed, step scale); d = 9 takes its points from the Ground-Vibrations training sets
CASES = [
    (2, 3, "ISO", 1, 0.8),
    (16, 3, "HX", 2, 0.5),
    (17, 2, "ANI", 3, 0.5),
    (48, 9, "GV", 4, 0.25),
    (50, 9, "GV", 5, 0.25),
    (64, 2, "ANI", 6, 0.4),
    (65, 3, "ISO", 7, 0.3),
    (90, 3, "HX", 8, 0.3),
    (128, 4, "GV", 9, 0.25),
    # the other variant (general / FULL) of every NB, and NB = 7: all 16 instances are launched
    (32, 3, "GV", 10, 0.4),
    (40, 2, "ANI", 11, 0.4),
    (80, 3, "ISO", 12, 0.3),
    (96, 4, "HX", 13, 0.3),
    (100, 3, "GV", 14, 0.3),
    (112, 4, "ISO", 15, 0.25),
    (120, 2, "ANI", 16, 0.3),
]


def training_set(n, d, seed):
    if d == 9:
        D, y = load_gv(50 if n <= 50 else 90, 1 + seed % 8)[:2]
        return D[:n].copy(), y[:n].copy()
    rng = np.random.default_rng(1000 + seed)
    D = rng.random((n, d))
    y = np.sin(3.0 * D).sum(axis=1) + 0.3 * np.cos(11.0 * D[:, 0]) + 0.05 * rng.standard_normal(n)
    return D, y


def make_case(n, d, script, seed, scale, t=T):
    D, y = training_set(n, d, seed)
    q = 4 if script == "ANI" else 3
    rng = np.random.default_rng(seed)
    theta0 = np.concatenate([[2.0, 3.5, 0.3], np.zeros(q - 3)]) if d != 9 else np.array([1.0, 1.0, 0.0])
    steps = scale * rng.standard_normal((t, q))
    logu = np.log(rng.random(t))
    return dict(D=D, y=y, s2=float(np.var(y, ddof=1)), script=script, prior=PRIOR_ID[script],
                pars=PARS if script == "HX" else None, theta0=theta0, steps=steps, logu=logu)


def walk(case, evaluate):
    """The chain of a case, one proposal at a time: evaluate(theta) -> (val, beta, status).  Returns the trace and the state."""
    theta = case["theta0"].copy()
    l, beta, _ = evaluate(theta)
    tr = dict(val=[], beta=[], status=[], accept=[], draws=[], l0=l, beta0=beta)
    for e, lu in zip(case["steps"], case["logu"]):
        cand = theta + e
        v, b, st = evaluate(cand)
        acc = bool(math.isfinite(v) and (v - l) > lu)
        tr["val"].append(v); tr["beta"].append(b); tr["status"].append(st); tr["accept"].append(int(acc))
        if acc:
            theta, l, beta = cand, v, b
            tr["draws"].append(cand)
    tr.update(theta=theta, l=l, beta_fin=beta)
    return tr


if __name__ == "__main__":
    from oracle import ccgp_oracle as orc

    for c in CASES:
        case = make_case(*c)

        def ev(theta, case=case):
            try:
                o = orc.logpost(case["D"], theta, case["y"], case["s2"], case["script"], case["pars"])
                return float(o["val"]), float(o["beta"]), 0
            except Exception:
                return math.nan, math.nan, 1
        tr = walk(case, ev)
        # the smallest L D L' pivot over the start and the proposals, in units of the device's failure threshold n eps
        piv, theta = [], case["theta0"].copy()
        for e, acc in zip(np.concatenate([np.zeros((1, theta.size)), case["steps"]]), [0] + tr["accept"]):
            cand = theta + e
            p, t1, t2 = 1.0 / (1.0 + math.exp(-cand[2])), math.exp(cand[0]), math.exp(cand[1])
            lam = math.exp(cand[3]) if cand.size == 4 else None
            r1 = np.array([t1, t2]) if lam is not None else np.full(case["D"].shape[1], t1)
            r2 = (1.0 + lam) * r1 if lam is not None else np.full(case["D"].shape[1], t2)
            d2 = (case["D"][:, None, :] - case["D"][None, :, :]) ** 2
            R = (p * p * np.exp(-(d2 * r1).sum(-1)) + (1 - p) ** 2 * np.exp(-(d2 * r2).sum(-1))) / (p * p + (1 - p) ** 2)
            try:
                piv.append(float(np.min(np.diag(np.linalg.cholesky(R)) ** 2)))
            except np.linalg.LinAlgError:
                piv.append(0.0)
            if acc:
                theta = cand
        print(c, "accepted", sum(tr["accept"]), "rejected", T - sum(tr["accept"]), "failed", sum(tr["status"]),
              "min pivot / (n eps) %.3g" % (min(piv) / (case["D"].shape[0] * 2.220446049250313e-16)))
