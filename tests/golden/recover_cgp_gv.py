#!/usr/bin/env python3
"""Recover the CGP fit that produced the `*.CGP` columns of the reference's only recorded output,
`Ground Vibrations Emulator/Results/Size 50 Results 1.txt` (written by GV:759-761).

compare.GP (GV:648-676) fills those columns from `CGP(D.train, y.train)` and `predict.CGP(cgp, D.test, PI = TRUE)`:
y.hat.CGP = Yp, LL.CGP = Y_low, UL.CGP = Y_up.  The fit's random Latin hypercube is not reproducible, its optimum is: the
objective var.MLE.DK (GV:102-133) is minimised over (lambda, Stand_theta[9], kappa, bw) in the box of GV:77-89, and at the
optimum most variables sit ON a bound, where optim leaves them exactly.  So

  1. fit the restatement (tests/cgp_ref.py behind cgp.CGP) from seeded starts;
  2. keep every variable that ended on a bound there, and solve least squares over the others against the 150 x 3 recorded
     numbers.

The residual is at rounding level (1e-12): the recovery is exact, which turns the recorded table into a deterministic
known-answer test for the whole of predict.CGP -- three correlation families, five reweighted solves, the variance ratio v,
the interval.

Run from the repo root:  python tests/golden/recover_cgp_gv.py   (CPU, about two minutes; writes
tests/golden/gv_cgp_recovered.json).  Inputs are the data fixtures under tests/golden/data/gv/.
"""
import json
import os
import sys

import numpy as np
from scipy.optimize import least_squares

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ccgp_amd  # noqa: E402,F401
from ccgp_amd import cgp  # noqa: E402
from ccgp_amd.tables import read_table  # noqa: E402
import cgp_ref  # noqa: E402


def recorded_cgp():
    names, res = read_table(os.path.join(HERE, "data", "gv", "results_50_1.txt"))
    col = {n: i for i, n in enumerate(names)}
    return res[:, :9], res[:, [col["y.hat.CGP"], col["LL.CGP"], col["UL.CGP"]]]


def device_row(ww, scales):
    """(lambda, Stand_theta, kappa, bw) -> (lambda, theta, alpha, bw) on the scale of the design itself (GV:164-165)."""
    p = scales.shape[0]
    th = ww[1:1 + p]
    return np.concatenate([[ww[0]], th / scales ** 2, (ww[1 + p] + th) / scales ** 2, [ww[2 + p]]])


def main():
    _, tr = read_table(os.path.join(HERE, "data", "gv", "train_50_1.txt"))
    D, y = tr[:, :9], tr[:, 9]
    Dt, rec = recorded_cgp()
    Xs, scales = cgp.standardise(D)

    est = cgp.CGP(cgp_ref.NumpyHandle(), D, y, rng=0)
    ww, lower, upper = est["par"].copy(), est["lower"], est["upper"]
    free = np.flatnonzero((ww > lower) & (ww < upper))
    print("fit: objective %.6f, free variables %s" % (est["objval"], free.tolist()))

    def table(x):
        w = ww.copy()
        w[free] = x
        out, _ = cgp_ref.predict(D, y, device_row(w, scales), Dt)
        return out[:, [0, 4, 5]]

    r = least_squares(lambda x: (table(x) - rec).ravel(), ww[free], bounds=(lower[free], upper[free]), x_scale=ww[free],
                      xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
    ww[free] = r.x
    resid = float(np.abs(table(r.x) - rec).max())
    objective = float(cgp_ref.state(Xs, y, cgp.rows_from_ww(ww)[0])["val"])
    out = {
        "source": "Ground Vibrations Emulator/Results/Size 50 Results 1.txt:2-151, columns y.hat.CGP, LL.CGP, UL.CGP; "
                  "Training Set Size 50 Sample 1",
        "model": "CGP GV:58-236: (lambda, Stand_theta[9], kappa, bw) in the box of GV:77-89; alpha = kappa + theta",
        "ww": ww.tolist(), "lower": lower.tolist(), "upper": upper.tolist(), "free": free.tolist(),
        "scales": scales.tolist(), "row": device_row(ww, scales).tolist(),
        "objective": objective, "fit_objective": est["objval"], "max_abs_resid": resid,
        "on_bounds": "; ".join("ww[%d] at its %s bound" % (i, "lower" if ww[i] == lower[i] else "upper")
                               for i in range(ww.shape[0]) if i not in free),
    }
    print(json.dumps(out, indent=1))
    assert resid < 1e-10
    with open(os.path.join(HERE, "gv_cgp_recovered.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
