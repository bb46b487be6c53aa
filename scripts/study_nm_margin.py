"""How far apart two correct Nelder-Mead searches stop: fit.laplace_sets (the lockstep search) against fit.laplace (scipy's)
on the 17 Ground-Vibrations training sets, on the CPU with the oracle's logpost as the evaluator, sigma2 = var(y) and the
reference's start (1, 1, 0) (GV:692).  Prints per set value(laplace) - value(laplace_sets), the largest positive gap, and
ten times it: the margin tests/test_sets_host.py allows (profiles/study.md).
    python scripts/study_nm_margin.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ccgp_amd  # noqa: E402,F401
from ccgp_amd import fit  # noqa: E402
from ccgp_amd.tables import read_table  # noqa: E402
from oracle import ccgp_oracle as orc  # noqa: E402


def gv_sets():
    for size, count in ((50, 9), (90, 8)):
        for i in range(1, count + 1):
            _, tr = read_table(os.path.join(ROOT, "tests", "golden", "data", "gv", "train_%d_%d.txt" % (size, i)))
            yield "%d_%d" % (size, i), tr[:, :9], tr[:, 9]


def main():
    gaps = []
    for name, D, y in gv_sets():
        s2 = float(np.var(y, ddof=1))

        def one(rows):
            return np.array([orc.logpost(D, r, y, s2, "GV")["val"] for r in np.atleast_2d(rows)])

        a = fit.laplace(one, np.array([1.0, 1.0, 0.0]))
        b = fit.laplace_sets(lambda rows, set_of: one(rows), np.array([[1.0, 1.0, 0.0]]))[0]
        gaps.append(a["value"] - b["value"])
        print("%-5s scipy %.12f (converged %s)  lockstep %.12f (converged %s, %d iterations)  gap %+.3e  |mode diff| %.2e" % (
            name, a["value"], a["converged"], b["value"], b["converged"], b["iterations"], gaps[-1],
            np.max(np.abs(a["mode"] - b["mode"]))))
    worst = max(max(gaps), 0.0)
    print("largest gap (scipy above lockstep): %.3e   margin = 10 x: %.3e   largest the other way: %.3e" % (
        worst, 10 * worst, max(-min(gaps), 0.0)))


if __name__ == "__main__":
    main()
