"""The two maximum-entropy design searches of the batch-sequential script two ways, timed: the host-lockstep arm (the default:
one device call per lockstep step for all running starts, the host taking every quasi-Newton step in numpy) against the device
arm (on_device=True: the starts resident on the device, one launch per `seg` evaluations).  The searches are
Entropy_optim(14, 2, prior medians, 20 starts, rng 0) and Batch_Entropy_optim(Initial ME Design, 7, 2, prior medians, 25 starts
from make_starts(25, 7, 2, 0)).  The two arms compute the same result, bit for bit in every key but device_calls: that is
asserted after every pair of runs.

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  Per search and arm: seconds and device calls of every run, the median and the range; for the device arm also
the evaluations of the longest start -- what the launch waits for -- and microseconds per evaluation of that start: seconds of
the launches over those evaluations, the single-workgroup latency of the design-gradient instance with the step behind it.
The condition: the device arm's slowest run below the lockstep arm's fastest, for both searches.
Run from the repository root:  python scripts/device_design_timing.py [--runs 3] [--out profiles/device_design.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "device_design.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, design
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table

    prior = (0.5, 1.0, 4.0)   # p.prior, theta1.prior, theta2.prior (BSQ:981-983)
    _, D0 = read_table("tests/golden/data/bsq/initial_me_design.txt")
    S2 = design.make_starts(25, 7, 2, 0)
    h = api.Handle(0)

    class Timed:
        """The handle with the device launches of the search timed."""

        def __init__(self):
            self.launch_seconds, self.critical, self.launches = 0.0, 0, 0

        def __getattr__(self, name):
            return getattr(h, name)

        def design_fit(self, *a, **k):
            t0 = time.perf_counter()
            r = h.design_fit(*a, **k)
            self.launch_seconds += time.perf_counter() - t0
            self.critical += int(r["evals"].max())
            self.launches += 1
            return r

    def search(which, on_device):
        c = Timed()
        gp = CombinedGP("BSQ", handle=c)
        t0 = time.perf_counter()
        if which == "first":
            r = gp.Entropy_optim(14, 2, *prior, 20, rng=0, on_device=on_device)
        else:
            r = gp.Batch_Entropy_optim(D0, 7, 2, *prior, 25, starts=S2, on_device=on_device)
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, device_calls=int(r["device_calls"]), iterations=int(r["iterations"].sum()))
        if on_device:
            out.update(launches=c.launches, launch_seconds=c.launch_seconds, critical_evaluations=c.critical,
                       us_per_start_evaluation=1e6 * c.launch_seconds / max(c.critical, 1))
        return out, r

    def same(a, b):
        return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "device_calls")

    searches, arms = ("first", "second"), (("lockstep", False), ("device", True))
    for s in searches:
        for _, dev in arms:
            search(s, dev)   # warm-up: code objects, staging and pinned buffers
    out = dict(starts=dict(first=20, second=25), runs={s: {a: [] for a, _ in arms} for s in searches})
    for run in range(args.runs):
        for s in searches:
            res = {}
            for a, dev in arms:
                fig, res[a] = search(s, dev)
                out["runs"][s][a].append(fig)
                print(s, a, "run", run, json.dumps(fig), flush=True)
            assert same(res["lockstep"], res["device"]), "the two arms disagree on the %s search" % s
    out["summary"] = {}
    for s in searches:
        sm = {}
        for a, _ in arms:
            runs = out["runs"][s][a]
            sm[a] = {k: dict(median=float(np.median([r[k] for r in runs])), min=float(min(r[k] for r in runs)),
                             max=float(max(r[k] for r in runs))) for k in runs[0]}
        lo, dv = sm["lockstep"]["seconds"], sm["device"]["seconds"]
        sm["ratio_seconds"] = lo["median"] / dv["median"]
        sm["separated"] = bool(dv["max"] < lo["min"])   # the condition
        out["summary"][s] = sm
    out["summary"]["condition_met"] = bool(all(out["summary"][s]["separated"] for s in searches))
    print(json.dumps(out["summary"], indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
