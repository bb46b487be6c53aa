"""The single-GP comparator's prediction (ccgp_krige_predict_batch), call by call, on the Ground-Vibrations set train_50_1
(n = 50, d = 9, its 150 test sites) and on Qian (n = 64, d = 4, its 14 test sites): the median wall time of

  krige_B1     krige_predict_batch, one model, form PLUGIN
  krige_B8     the same call with 8 models (the starts of a fit)
  host_inverse what the same columns cost before the call existed: corr_matrix + corr_cross on the device and the numpy
               inverse of tests/test_reference_pins_gpu.py
  fit_predict  fit.ordinary_kriging_fit, then the prediction, end to end

Wall time is a host clock around calls that block until their results are on the host; these calls are latency-bound.  Each
figure is the median (with min and max) over the repeats after warm-up calls.
Run from the repository root:  python scripts/single_gp_timing.py [--repeats 200] [--fit-repeats 5] [--out profiles/single_gp_timing.json]"""
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


def datasets():
    _, tr = read_table('tests/golden/data/gv/train_50_1.txt')
    _, te = read_table('tests/golden/data/gv/test_50_1.txt')
    yield "gv_train_50_1", tr[:, :9], tr[:, 9], te[:, :9]
    _, tr = read_table('tests/golden/data/qian_train.txt')
    _, te = read_table('tests/golden/data/qian_test.txt')
    yield "qian", tr[:, :4], tr[:, 4], te[:, :4]


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--fit-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "single_gp_timing.json"))
    args = ap.parse_args()
    h = api.Handle(0)
    out = {}
    for name, D, y, Dt in datasets():
        n, d = D.shape
        est = fit.ordinary_kriging_fit(h, D, y)
        row = np.concatenate([[1.0], est["theta"]])[None]
        rows8 = np.repeat(row, 8, axis=0)
        rows8[:, 1:] *= (1.0 + 0.05 * np.arange(8))[:, None]
        s2 = np.array([est["sigma2"]])

        def host_inverse():
            R = h.corr_matrix(D, est["theta"])
            r = h.corr_cross(Dt, D, est["theta"])
            R_inv = np.linalg.inv(R)
            q = np.einsum("ti,ij,tj->t", r, R_inv, r)
            v1 = R_inv.sum(axis=0)
            beta = float(v1 @ y) / float(v1.sum())
            return beta + r @ (R_inv @ (y - beta)), est["sigma2"] * (1.0 - q)

        def fit_predict():
            e = fit.ordinary_kriging_fit(h, D, y)
            return h.krige_predict_batch(D, y, 1, np.concatenate([[1.0], e["theta"]])[None], [e["sigma2"]], Dt, api.VAR_PLUGIN)

        rec = dict(n=int(n), d=int(d), sites=int(Dt.shape[0]), seconds=dict(
            krige_B1=timed(lambda: h.krige_predict_batch(D, y, 1, row, s2, Dt, api.VAR_PLUGIN), args.repeats),
            krige_B8=timed(lambda: h.krige_predict_batch(D, y, 1, rows8, np.repeat(s2, 8), Dt, api.VAR_PLUGIN), args.repeats),
            host_inverse=timed(host_inverse, args.repeats),
            fit_predict=timed(fit_predict, args.fit_repeats, warmup=1)))
        # the two ways to the same columns agree (the host inverse carries cond(R) eps)
        mean, var, _, _, st = h.krige_predict_batch(D, y, 1, row, s2, Dt, api.VAR_PLUGIN)
        hm, hv = host_inverse()
        rec["max_abs_diff_mean"] = float(np.abs(mean[0] - hm).max())
        rec["max_abs_diff_var"] = float(np.abs(var[0] - hv).max())
        rec["status"] = int(st[0])
        out[name] = rec
        print(name, json.dumps(rec))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
