"""The ordinary-kriging MLE two ways, on the Ground-Vibrations set train_50_1 (n = 50, d = 9) and on Qian (n = 64, d = 4):
fit.ordinary_kriging_sigma2 (scipy L-BFGS-B, one start after another, three device calls per objective value) against
fit.ordinary_kriging_fit (ccgp_profile_batch: one factorisation per point, all starts in lockstep, one device call per
evaluator call).  Wall time, device calls and best log-likelihood of each.

Both routines run in ONE process on one device, interleaved (a, b, a, b, ...), after a warm-up pass of each; the wall
time is a host clock around calls that block until their results are on the host.  Reported: median and range over the
repeats.  Run from the repository root:  python scripts/kriging_fit_timing.py [--repeats 7] [--out profiles/kriging_fit_timing.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, '.')
import numpy as np
import ccgp_amd  # noqa: F401
from ccgp_amd import api, fit
from ccgp_amd.tables import read_table


class Counting:
    """The handle with its device calls counted (every method that reaches the C ABI's batched entry points)."""

    def __init__(self, h):
        self._h, self.calls = h, 0

    def __getattr__(self, name):
        attr = getattr(self._h, name)
        if name not in ("loglik_batch", "loglik_grad_batch", "profile_batch"):
            return attr

        def call(*a, **k):
            self.calls += 1
            return attr(*a, **k)
        return call


def datasets():
    _, tr = read_table('tests/golden/data/gv/train_50_1.txt')
    yield "gv_train_50_1", tr[:, :9], tr[:, 9]
    _, tr = read_table('tests/golden/data/qian_train.txt')
    yield "qian", tr[:, :4], tr[:, 4]


def run_old(h, D, y):
    c = Counting(h)
    t0 = time.perf_counter()
    s2, theta, beta = fit.ordinary_kriging_sigma2(c, D, y)
    dt = time.perf_counter() - t0
    ll = h.loglik_batch(D, y, 1, np.concatenate([[1.0], theta])[None], s2)[0][0]
    return dict(seconds=dt, device_calls=c.calls, loglik=float(ll), sigma2=float(s2))


def run_new(h, D, y):
    c = Counting(h)
    t0 = time.perf_counter()
    r = fit.ordinary_kriging_fit(c, D, y)
    dt = time.perf_counter() - t0
    return dict(seconds=dt, device_calls=c.calls, loglik=r["loglik"], sigma2=r["sigma2"], points=r["evaluations"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "kriging_fit_timing.json"))
    args = ap.parse_args()
    h = api.Handle(0)
    out = {}
    for name, D, y in datasets():
        run_old(h, D, y)        # warm-up: code objects, workspace, pinned buffers
        run_new(h, D, y)
        old, new = [], []
        for _ in range(args.repeats):
            old.append(run_old(h, D, y))
            new.append(run_new(h, D, y))
        to, tn = np.array([r["seconds"] for r in old]), np.array([r["seconds"] for r in new])
        out[name] = dict(
            n=int(D.shape[0]), d=int(D.shape[1]), repeats=args.repeats,
            ordinary_kriging_sigma2=dict(old[-1], seconds_median=float(np.median(to)), seconds_min=float(to.min()), seconds_max=float(to.max())),
            ordinary_kriging_fit=dict(new[-1], seconds_median=float(np.median(tn)), seconds_min=float(tn.min()), seconds_max=float(tn.max())),
            ratio_of_medians=float(np.median(to) / np.median(tn)))
        print("%s: sigma2 routine %.1f ms [%.1f, %.1f], %d device calls, log-lik %.4f | lockstep fit %.1f ms [%.1f, %.1f], %d device calls "
              "(%d points), log-lik %.4f | ratio of medians %.1f" % (
                  name, 1e3 * np.median(to), 1e3 * to.min(), 1e3 * to.max(), old[-1]["device_calls"], old[-1]["loglik"],
                  1e3 * np.median(tn), 1e3 * tn.min(), 1e3 * tn.max(), new[-1]["device_calls"], new[-1]["points"], new[-1]["loglik"],
                  np.median(to) / np.median(tn)))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
