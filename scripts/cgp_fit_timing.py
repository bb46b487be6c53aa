"""The CGP comparator's fit (ccgp_amd.cgp.CGP) step by step, on the Ground-Vibrations set train_50_1 (n = 50, d = 9) and on
Qian (n = 64, d = 4): device calls, parameter rows evaluated, and the wall time of the candidate call (505 rows), of the
lockstep refinement, of the jackknife call (n rows) and of predict.CGP at 150 sites -- through the device handle, and the
same steps through the fp64 numpy restatement (tests/cgp_ref.NumpyHandle) on the host.

Wall time is a host clock around calls that block until their results are on the host.  The device figures are the median
and range over the repeats after one warm-up fit; the host restatement runs once.  The two halves can run on different
machines: each run merges its half into the output file.
Run from the repository root:  python scripts/cgp_fit_timing.py [--what device|host|both] [--repeats 5] [--out profiles/cgp_fit_timing.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import ccgp_amd  # noqa: F401
from ccgp_amd import cgp
from ccgp_amd.tables import read_table


def datasets():
    _, tr = read_table('tests/golden/data/gv/train_50_1.txt')
    _, te = read_table('tests/golden/data/gv/test_50_1.txt')
    yield "gv_train_50_1", tr[:, :9], tr[:, 9], te[:150, :9]
    _, tr = read_table('tests/golden/data/qian_train.txt')
    D = tr[:, :4]
    yield "qian", D, tr[:, 4], D.min(0) + np.random.default_rng(0).random((150, 4)) * (D.max(0) - D.min(0))


def one_fit(h, D, y, Dt):
    est = cgp.CGP(h, D, y, rng=0)
    t0 = time.perf_counter()
    cgp.predict_CGP(h, est, Dt, PI=True)
    sec = dict(est["seconds"], predict_150=time.perf_counter() - t0)
    return dict(seconds=sec, device_calls=est["calls"], refinement_calls=est["refinement_calls"], evaluations=est["evaluations"],
                objval=est["objval"], rmscv=est["rmscv"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=("device", "host", "both"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "cgp_fit_timing.json"))
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    h = None
    if args.what in ("device", "both"):
        from ccgp_amd import api
        h = api.Handle(0)
    for name, D, y, Dt in datasets():
        rec = out.setdefault(name, {})
        rec.update(n=int(D.shape[0]), d=int(D.shape[1]))
        if h is not None:
            one_fit(h, D, y, Dt)        # warm-up: code objects, workspace, pinned buffers
            runs = [one_fit(h, D, y, Dt) for _ in range(args.repeats)]
            dev = dict(runs[-1], repeats=args.repeats, seconds={
                k: dict(median=float(np.median([r["seconds"][k] for r in runs])), min=float(min(r["seconds"][k] for r in runs)),
                        max=float(max(r["seconds"][k] for r in runs))) for k in runs[-1]["seconds"]})
            rec["device"] = dev
            print(name, "device:", json.dumps(dev))
        if args.what in ("host", "both"):
            import cgp_ref
            rec["host_numpy"] = one_fit(cgp_ref.NumpyHandle(), D, y, Dt)
            print(name, "host:", json.dumps(rec["host_numpy"]))
    if h is not None:
        h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
