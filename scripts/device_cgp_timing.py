"""The CGP comparator of the Ground-Vibrations study two ways, timed: cgp.CGP_sets with the refinement in lockstep on the host
(one device call per evaluation for all the running starts of a group, numpy forming the points, the clipped differences and
every L-BFGS step) against on_device=True (the starts resident on the device, two launches per evaluation, the host looking
every `look` rounds).  Sets are those of scripts/study_timing.py: the nine size-50 and eight size-90 sets, five starts each,
seed 0.  Both arms compute the same fits bit for bit -- the script asserts it on every field but calls, refinement_calls and
seconds -- so the figures to compare are the seconds of the refinement.

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  Per arm: seconds of the whole fit and of its refinement, device calls and refinement calls of every run, the
median and the range; for the device arm also the rounds (evaluations of the longest start of each call, which is what the
call waits for), microseconds per round, and the refinement's time outside ccgp_cgp_fit_sets.  The same for one set
(train_50_1) through cgp.CGP.
Run from the repository root:  python scripts/device_cgp_timing.py [--runs 3] [--look 16] [--out profiles/device_cgp.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

SKIP = ("calls", "refinement_calls", "seconds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--look", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "device_cgp.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, cgp
    from ccgp_amd.tables import read_table

    groups = []
    for size, count in ((50, 9), (90, 8)):
        sets = []
        for i in range(1, count + 1):
            _, tr = read_table("tests/golden/data/gv/train_%d_%d.txt" % (size, i))
            sets.append((tr[:, :9], tr[:, 9]))
        groups.append(sets)
    h = api.Handle(0)

    class Timed:
        """The handle with the calls of ccgp_cgp_fit_sets timed and their rounds counted."""

        def __init__(self):
            self.launch_seconds, self.rounds, self.fit_calls = 0.0, 0, 0

        def __getattr__(self, name):
            return getattr(h, name)

        def cgp_fit_sets(self, *a, **k):
            t0 = time.perf_counter()
            r = h.cgp_fit_sets(*a, **k)
            self.launch_seconds += time.perf_counter() - t0
            self.rounds += int(r["evals"].max())
            self.fit_calls += 1
            return r

    def same(got, want):
        for k in want:
            if k not in SKIP:
                a, b = np.asarray(got[k]), np.asarray(want[k])
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), k

    def arm(which, problems):
        """problems: lists of (X, y) of one shape each; a list of one set goes through cgp.CGP."""
        c = Timed()
        t0 = time.perf_counter()
        fits, refinement, calls, ref_calls = [], 0.0, 0, 0
        for sets in problems:
            if len(sets) == 1:
                ests = [cgp.CGP(c, sets[0][0], sets[0][1], on_device=which == "device", look=args.look)]
            else:
                ests = cgp.CGP_sets(c, [s[0] for s in sets], [s[1] for s in sets], on_device=which == "device", look=args.look)
            fits += ests
            refinement += ests[0]["seconds"]["refinement"]
            calls += ests[0]["calls"]
            ref_calls += ests[0]["refinement_calls"]
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, refinement_seconds=refinement, calls=calls, refinement_calls=ref_calls)
        if which == "device":
            out.update(launch_seconds=c.launch_seconds, rounds=c.rounds, us_per_round=1e6 * c.launch_seconds / c.rounds,
                       outside_launch_seconds=refinement - c.launch_seconds)
        else:
            out.update(us_per_refinement_call=1e6 * refinement / ref_calls)
        return out, fits

    arms = ("lockstep", "device")
    out = dict(look=args.look, starts=5, sets=[[len(g), g[0][0].shape[0]] for g in groups])
    for label, problems in (("study", groups), ("train_50_1", [groups[0][:1]])):
        ref = None
        for a in arms:   # warm-up: code objects, staging and pinned buffers; and the two arms return the same fits
            _, fits = arm(a, problems)
            if ref is None:
                ref = fits
            for g, w in zip(fits, ref):
                same(g, w)
        runs = {a: [] for a in arms}
        for run in range(args.runs):
            for a in arms:
                r, fits = arm(a, problems)
                for g, w in zip(fits, ref):
                    same(g, w)
                runs[a].append(r)
                print(label, a, "run", run, json.dumps(r), flush=True)
        summary = {}
        for a in arms:
            summary[a] = {k: dict(median=float(np.median([r[k] for r in runs[a]])), min=float(min(r[k] for r in runs[a])),
                                  max=float(max(r[k] for r in runs[a]))) for k in runs[a][0]}
        lo, dv = summary["lockstep"]["refinement_seconds"], summary["device"]["refinement_seconds"]
        summary["ratio_refinement_seconds"] = lo["median"] / dv["median"]
        # the condition: the device arm's slowest refinement below the lockstep arm's fastest
        summary["separated"] = bool(dv["max"] < lo["min"])
        summary["same_fits"] = True
        out[label] = dict(runs=runs, summary=summary)
        print(label, json.dumps(summary, indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
