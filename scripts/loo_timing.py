"""Leave-one-out cross-validation of the Combined GP, timed: one ccgp_loo_batch call and one ccgp_loo_summary call against
today's way on the same box -- n calls of ccgp_predict_batch, each on the n - 1 other points and the one held-out site -- and
against one ccgp_loglik_batch of the same draws as the floor (one factorisation per draw and nothing else).

Sets: Ground-Vibrations train_50_1 (n = 50, d = 9, S = 1000 draws), Qian (n = 64, d = 4, S = 1000) and a synthetic design of
n = 2048 points (d = 3, S = 8) on the blocked sweep.  At n = 2048 the n-call route is timed on --folds of its folds (default
16) and scaled to n; everywhere else every fold runs.

Wall time is a host clock around calls that block until their results are on the host: median and range over the repeats
after one warm-up call.  Beside it the device time of the launch groups (ccgp_get_timing) of the loo call, of the likelihood
call and of the gradient call, whose instance carries the same identity rows: what the epilogue costs on top of the
factorisation it follows.
Run from the repository root:  python scripts/loo_timing.py [--repeats 5] [--folds 16] [--out profiles/loo_timing.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import ccgp_amd  # noqa: F401
from ccgp_amd import api
from ccgp_amd.tables import read_table


def iso_rows(S, d, seed, t1, t2):
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([[p, 1.0 - p], np.full(d, a), np.full(d, b)])
                     for p, a, b in zip(rng.uniform(0.6, 0.95, S), rng.uniform(*t1, S), rng.uniform(*t2, S))])


def datasets():
    _, tr = read_table('tests/golden/data/gv/train_50_1.txt')
    yield "gv_train_50_1", tr[:, :9], tr[:, 9], iso_rows(1000, 9, 1, (0.03, 0.15), (0.8, 3.0)), 0
    _, tr = read_table('tests/golden/data/qian_train.txt')
    yield "qian", tr[:, :4], tr[:, 4], iso_rows(1000, 4, 2, (0.15, 1.0), (10.0, 60.0)), 0
    rng = np.random.default_rng(3)
    n, d = 2048, 3
    X = np.stack([(rng.permutation(n) + rng.random(n)) / n for _ in range(d)], axis=1)
    y = np.sin(2 * np.pi * X).sum(axis=1)
    yield "synthetic_2048", X, y, iso_rows(8, d, 4, (20.0, 60.0), (300.0, 900.0)), 1


def clock(fn, repeats):
    fn()                                # warm-up: code objects, workspace, pinned buffers
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return out, dict(median=float(np.median(secs)), min=float(min(secs)), max=float(max(secs)), repeats=repeats)


def device_ms(h, fn):
    h.enable_timing(True)
    try:
        fn()
        t = h.get_timing()
    finally:
        h.enable_timing(False)
    return {k: [round(v[0], 4), int(v[1])] for k, v in t.items() if v[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--folds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "loo_timing.json"))
    args = ap.parse_args()
    h = api.Handle(0)
    out = {}
    probs = (0.025, 0.975)
    for name, X, y, rows, sample_folds in datasets():
        n, d = X.shape
        S, s2 = len(rows), float(np.var(y, ddof=1))
        rec = out[name] = dict(n=n, d=d, S=S)
        (mean, var, _, _, st), rec["loo_batch"] = clock(lambda: h.loo_batch(X, y, 2, rows, s2), args.repeats)
        res, rec["loo_summary"] = clock(lambda: h.loo_summary(X, y, 2, rows, s2, probs), args.repeats)
        _, rec["loglik_batch"] = clock(lambda: h.loglik_batch(X, y, 2, rows, s2), args.repeats)
        rec["failed_draws"] = int((st != 0).sum())
        folds = list(range(n)) if not sample_folds else list(np.linspace(0, n - 1, args.folds).astype(int))
        keep = [np.arange(n) != i for i in folds]
        Xs, ys = [np.asfortranarray(X[k]) for k in keep], [y[k].copy() for k in keep]

        def n_calls():
            return [h.predict_batch(Xs[j], ys[j], 2, rows, X[i:i + 1], s2) for j, i in enumerate(folds)]

        tabs, t = clock(n_calls, 1 if sample_folds else min(args.repeats, 3))
        scale = n / len(folds)
        rec["n_predict_calls"] = dict(t, folds_timed=len(folds), median_scaled_to_n=t["median"] * scale)
        # the two routes agree: largest difference over the timed folds relative to the spread of y
        ok = st == 0
        dm = max(float(np.nanmax(np.abs(tab[0][ok, 0] - mean[ok, i]))) for tab, i in zip(tabs, folds))
        dv = max(float(np.nanmax(np.abs(tab[1][ok, 0] - var[ok, i]))) for tab, i in zip(tabs, folds))
        rec["max_abs_diff_vs_n_calls"] = dict(mean=dm, var=dv, y_sd=float(np.sqrt(s2)), sigma2=s2)
        rec["device_ms"] = dict(loo_batch=device_ms(h, lambda: h.loo_batch(X, y, 2, rows, s2)),
                                loglik_batch=device_ms(h, lambda: h.loglik_batch(X, y, 2, rows, s2)),
                                loglik_grad_batch=device_ms(h, lambda: h.loglik_grad_batch(X, y, 2, rows, s2)))
        y_hat = res["y_hat"]
        rec["loo_rmspe"] = float(np.sqrt(np.mean((y - y_hat) ** 2)))
        rec["loo_coverage_95"] = float(np.mean((y >= res["quantiles"][:, 0]) & (y <= res["quantiles"][:, 1])))
        rec["speedup_vs_n_calls"] = rec["n_predict_calls"]["median_scaled_to_n"] / rec["loo_batch"]["median"]
        rec["loo_over_loglik"] = rec["loo_batch"]["median"] / rec["loglik_batch"]["median"]
        print(name, json.dumps(rec))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
