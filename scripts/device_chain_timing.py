"""The Metro part of the Ground-Vibrations study two ways, timed: fit.Metro_sets (one device call per step for all the chains
of a group, the host drawing and deciding every proposal) against fit.Metro_device_sets (the chains resident on the device,
one launch per segment).  Sets and settings are those of scripts/study_timing.py: the nine size-50 and eight size-90 sets,
N.max 5000, samp.size 1000, alpha.geweke 0.5, batch.size 20, start (1, 1, 0), sigma2 = var(y), one generator per set seeded
with the set's number.  The Laplace estimates are computed once (fit.laplace_sets on the lockstep evaluator) and handed to
both arms, so the arms differ in the chains alone.  The two arms run DIFFERENT chains (each has its stream contract) of the
same law, so proposals differ and the figure to compare is the time per proposal.

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  Per arm: seconds, device calls, proposals and microseconds per proposal of every run, the median and the
range.  Run from the repository root:  python scripts/device_chain_timing.py [--runs 3] [--out profiles/device_chains_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

SETTINGS = dict(N=5000, samp_size=1000, batch_size=20, alpha=0.5)
START = np.array([1.0, 1.0, 0.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seg", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join("profiles", "device_chains_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table

    groups = []
    for size, count in ((50, 9), (90, 8)):
        sets = []
        for i in range(1, count + 1):
            _, tr = read_table("tests/golden/data/gv/train_%d_%d.txt" % (size, i))
            sets.append((tr[:, :9], tr[:, 9]))
        groups.append(sets)
    h = api.Handle(0)
    gp = CombinedGP("GV", handle=h)
    prepared = []
    seed = 0
    for sets in groups:
        Ds, ys = [s[0] for s in sets], [s[1] for s in sets]
        s2 = [float(np.var(y, ddof=1)) for y in ys]
        fn = fit._device_sets_evaluator(gp, Ds, ys, s2, None, None)
        ests = fit.laplace_sets(lambda rows, set_of: fn(rows, set_of)[0], np.tile(START, (len(sets), 1)))
        prepared.append((Ds, ys, s2, ests, [seed + i + 1 for i in range(len(sets))]))
        seed += len(sets)

    def arm(which):
        t0 = time.perf_counter()
        calls = proposals = accepted = 0
        for Ds, ys, s2, ests, seeds in prepared:
            if which == "lockstep":
                r = fit.Metro_sets(gp, None, SETTINGS["N"], SETTINGS["samp_size"], SETTINGS["batch_size"], SETTINGS["alpha"], Ds, s2,
                                   ys, rngs=seeds, laplace=ests)
            else:
                r = fit.Metro_device_sets(gp, None, SETTINGS["N"], SETTINGS["samp_size"], SETTINGS["batch_size"], SETTINGS["alpha"],
                                          Ds, s2, ys, rngs=seeds, laplace=ests, seg=args.seg)
            calls += r["device_batches"] + 1
            proposals += sum(c["proposals"] for c in r["chains"])
            accepted += sum(c["accepted"] for c in r["chains"])
        secs = time.perf_counter() - t0
        return dict(seconds=secs, calls=calls, proposals=proposals, accepted=accepted, us_per_proposal=1e6 * secs / proposals)

    arms = ("lockstep", "device")
    for a in arms:
        arm(a)   # warm-up: code objects, staging and pinned buffers
    out = dict(settings=SETTINGS, seg=args.seg, sets=[[len(g), g[0][0].shape[0]] for g in groups], runs={a: [] for a in arms})
    for run in range(args.runs):
        for a in arms:
            out["runs"][a].append(arm(a))
            print(a, "run", run, json.dumps(out["runs"][a][-1]), flush=True)
    out["summary"] = {}
    for a in arms:
        out["summary"][a] = {k: dict(median=float(np.median([r[k] for r in out["runs"][a]])),
                                     min=float(min(r[k] for r in out["runs"][a])), max=float(max(r[k] for r in out["runs"][a])))
                             for k in ("seconds", "calls", "proposals", "us_per_proposal")}
    lo, dv = out["summary"]["lockstep"]["us_per_proposal"], out["summary"]["device"]["us_per_proposal"]
    out["summary"]["ratio_us_per_proposal"] = lo["median"] / dv["median"]
    # the condition: the device arm lies below the lockstep arm by more than the two arms' ranges
    out["summary"]["separated"] = bool(lo["median"] - dv["median"] > (lo["max"] - lo["min"]) + (dv["max"] - dv["min"]))
    print(json.dumps(out["summary"], indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
