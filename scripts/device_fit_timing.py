"""The ordinary-kriging (sigma2 / single-GP) fits of the Ground-Vibrations study two ways, timed: fit.ordinary_kriging_fit_sets
(one device call per lockstep step for all the starts of a group, the host taking every L-BFGS step in numpy) against
fit.ordinary_kriging_fit_device_sets (the starts resident on the device, one launch per `seg` evaluations).  Sets are those
of scripts/study_timing.py: the nine size-50 and eight size-90 sets, eight starts each, seed 0.  The two arms run the same
method from the same starts; they differ in the exp behind theta = exp(log theta) (numpy's against the portable one), so the
evaluation counts may differ by a few and the figures to compare are the seconds of the whole fit and the time per evaluation.

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  Per arm: seconds, device calls (the groups' calls: what the device saw) and evaluations of every run, the
median and the range; for the device arm also microseconds per evaluation of a start -- the single-workgroup latency of the
profiled-gradient instance with the step behind it: seconds of the launches over the evaluations of the LONGEST start of each
launch, which is what the launch waits for -- and per evaluation overall.
Run from the repository root:  python scripts/device_fit_timing.py [--runs 3] [--out profiles/device_fits_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seg", type=int, default=512)
    ap.add_argument("--out", default=os.path.join("profiles", "device_fits_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, fit
    from ccgp_amd.tables import read_table

    groups = []
    for size, count in ((50, 9), (90, 8)):
        sets = []
        for i in range(1, count + 1):
            _, tr = read_table("tests/golden/data/gv/train_%d_%d.txt" % (size, i))
            sets.append((tr[:, :9], tr[:, 9]))
        groups.append(sets)
    h = api.Handle(0)

    class Counting:
        """The handle with its fit calls counted and the device launches timed."""

        def __init__(self):
            self.calls, self.launch_seconds, self.critical = 0, 0.0, 0

        def profile_batch_sets(self, *a, **k):
            self.calls += 1
            return h.profile_batch_sets(*a, **k)

        def profile_fit_eval_sets(self, *a, **k):
            self.calls += 1
            return h.profile_fit_eval_sets(*a, **k)

        def profile_fit_sets(self, *a, **k):
            self.calls += 1
            t0 = time.perf_counter()
            r = h.profile_fit_sets(*a, **k)
            self.launch_seconds += time.perf_counter() - t0
            self.critical += int(r["evals"].max())
            return r

    def arm(which):
        c = Counting()
        t0 = time.perf_counter()
        evaluations, ll = 0, []
        for sets in groups:
            Ds, ys = [s[0] for s in sets], [s[1] for s in sets]
            if which == "lockstep":
                fits = fit.ordinary_kriging_fit_sets(c, Ds, ys)
            else:
                fits = fit.ordinary_kriging_fit_device_sets(c, Ds, ys, seg=args.seg)
            evaluations += sum(f["evaluations"] for f in fits)
            ll += [f["loglik"] for f in fits]
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, calls=c.calls, evaluations=evaluations, us_per_evaluation=1e6 * secs / evaluations, loglik=ll)
        if which == "device":
            out.update(launch_seconds=c.launch_seconds, critical_evaluations=c.critical,
                       us_per_start_evaluation=1e6 * c.launch_seconds / c.critical)
        return out

    arms = ("lockstep", "device")
    for a in arms:
        arm(a)   # warm-up: code objects, staging and pinned buffers
    out = dict(seg=args.seg, starts=8, sets=[[len(g), g[0][0].shape[0]] for g in groups], runs={a: [] for a in arms})
    for run in range(args.runs):
        for a in arms:
            out["runs"][a].append(arm(a))
            print(a, "run", run, json.dumps({k: v for k, v in out["runs"][a][-1].items() if k != "loglik"}), flush=True)
    out["summary"] = {}
    for a in arms:
        keys = [k for k in out["runs"][a][0] if k != "loglik"]
        out["summary"][a] = {k: dict(median=float(np.median([r[k] for r in out["runs"][a]])),
                                     min=float(min(r[k] for r in out["runs"][a])), max=float(max(r[k] for r in out["runs"][a])))
                             for k in keys}
    lo, dv = out["summary"]["lockstep"]["seconds"], out["summary"]["device"]["seconds"]
    out["summary"]["ratio_seconds"] = lo["median"] / dv["median"]
    # the condition: the device arm's median below the lockstep arm's, the two ranges disjoint
    out["summary"]["separated"] = bool(dv["median"] < lo["median"] and dv["max"] < lo["min"])
    out["summary"]["max_abs_loglik_difference"] = float(np.max(np.abs(np.array(out["runs"]["lockstep"][0]["loglik"]) -
                                                                     np.array(out["runs"]["device"][0]["loglik"]))))
    print(json.dumps(out["summary"], indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
