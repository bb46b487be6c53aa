"""The Laplace stage of the Ground-Vibrations study two ways, timed: fit.laplace_sets over the twin evaluator
ccgp_chain_logpost_sets (what fit.study(device_chains=True) does: one device call per iteration with the four trial points of
every unfinished set, the host taking every Nelder-Mead step in numpy) against fit.laplace_device_sets (the searches resident
on the device, one launch per `seg` evaluations, then the Hessian's points as one call).  Sets are those of
scripts/study_timing.py: the nine size-50 and eight size-90 sets, from the reference's start (1, 1, 0) (GV:692), sigma2 per
set from the ordinary-kriging fit (computed once, outside the clock).

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  The script asserts that both arms return the same 17 modes and covariances (and every other key of
laplace_sets' dict) bit for bit.  Per arm: seconds and device calls of every run, the median and the range; for the device
arm also microseconds per evaluation of one search -- the single-workgroup latency of the chain instance with the step behind
it: seconds of the launches over the evaluations of the LONGEST search of each launch, which is what the launch waits for.
The condition: the device arm's slowest run below the lockstep arm's fastest.
Run from the repository root:  python scripts/device_laplace_timing.py [--runs 3] [--out profiles/device_laplace_timing.json]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seg", type=int, default=512)
    ap.add_argument("--out", default=os.path.join("profiles", "device_laplace_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table

    h = api.Handle(0)
    groups = []
    for size, count in ((50, 9), (90, 8)):
        sets = []
        for i in range(1, count + 1):
            _, tr = read_table("tests/golden/data/gv/train_%d_%d.txt" % (size, i))
            sets.append((tr[:, :9], tr[:, 9]))
        s2 = [f["sigma2"] for f in fit.ordinary_kriging_fit_device_sets(h, [s[0] for s in sets], [s[1] for s in sets])]
        groups.append((sets, s2))
    start = np.array([1.0, 1.0, 0.0])

    class Counting:
        """The handle with the Laplace stage's calls counted and the device launches timed."""

        def __init__(self):
            self.calls, self.launch_seconds, self.critical, self.launches = 0, 0.0, 0, 0

        def chain_logpost_sets(self, *a, **k):
            self.calls += 1
            return h.chain_logpost_sets(*a, **k)

        def laplace_search_sets(self, *a, **k):
            self.calls += 1
            self.launches += 1
            t0 = time.perf_counter()
            r = h.laplace_search_sets(*a, **k)
            self.launch_seconds += time.perf_counter() - t0
            self.critical += int(r["evals"].max())
            return r

    base = CombinedGP("GV", handle=h)

    def arm(which):
        c = Counting()
        gp = types.SimpleNamespace(h=c, cfg=base.cfg, script=base.script)
        t0 = time.perf_counter()
        ests = []
        for sets, s2 in groups:
            Ds, ys = [s[0] for s in sets], [s[1] for s in sets]
            starts = np.tile(start, (len(sets), 1))
            if which == "lockstep":
                fn = fit._twin_sets_evaluator(gp, Ds, ys, s2, None, None)
                ests += fit.laplace_sets(lambda rows, set_of: fn(rows, set_of)[0], starts)
            else:
                ests += fit.laplace_device_sets(gp, Ds, ys, s2, starts, seg=args.seg)
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, calls=c.calls, iterations=sum(e["iterations"] for e in ests),
                   charged=sum(e["evaluations"] for e in ests))
        if which == "device":
            out.update(launches=c.launches, launch_seconds=c.launch_seconds, fed=sum(e["fed"] for e in ests),
                       critical_evaluations=c.critical, us_per_search_evaluation=1e6 * c.launch_seconds / c.critical)
        return out, ests

    arms = ("lockstep", "device")
    for a in arms:
        arm(a)   # warm-up: code objects, staging and pinned buffers
    out = dict(seg=args.seg, start=start.tolist(), sets=[[len(g[0]), g[0][0][0].shape[0]] for g in groups],
               runs={a: [] for a in arms})
    for run in range(args.runs):
        got = {}
        for a in arms:
            r, got[a] = arm(a)
            out["runs"][a].append(r)
            print(a, "run", run, json.dumps(r), flush=True)
        for lo, dv in zip(got["lockstep"], got["device"]):   # the same 17 estimates, bit for bit
            for k in lo:
                assert np.asarray(lo[k], dtype=np.float64).tobytes() == np.asarray(dv[k], dtype=np.float64).tobytes(), k
    out["converged"] = [bool(e["converged"]) for e in got["device"]]
    out["iterations_per_set"] = [int(e["iterations"]) for e in got["device"]]
    out["fed_per_set"] = [int(e["fed"]) for e in got["device"]]
    out["summary"] = {}
    for a in arms:
        out["summary"][a] = {k: dict(median=float(np.median([r[k] for r in out["runs"][a]])),
                                     min=float(min(r[k] for r in out["runs"][a])), max=float(max(r[k] for r in out["runs"][a])))
                             for k in out["runs"][a][0]}
    lo, dv = out["summary"]["lockstep"]["seconds"], out["summary"]["device"]["seconds"]
    out["summary"]["ratio_seconds"] = lo["median"] / dv["median"]
    # the condition: the device arm's slowest run below the lockstep arm's fastest
    out["summary"]["separated"] = bool(dv["max"] < lo["min"])
    out["summary"]["same_bits"] = True
    print(json.dumps(out["summary"], indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
