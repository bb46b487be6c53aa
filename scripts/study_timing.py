"""The Ground-Vibrations simulation study two ways, timed: fit.study (the sets of one shape fitted in lockstep, one device call
per step for all their chains) against the loop a user writes without it (per set: ordinary_kriging_fit, fit.factors_frame,
compare_GP(exact=True)).  Sets: the nine size-50 and eight size-90 train / test pairs under tests/golden/data/gv; settings:
the reference's (GV:691-697: start (1, 1, 0), N.max 5000, samp.size = net.samp.size 1000, alpha.geweke 0.5, batch.size 20,
alpha 0.05); one generator per set, seeded with the set's number in both arms, at speculate 0 and 3.

Per arm and run: wall time (host clock around blocking calls) and device calls of the four parts -- sigma2 (the per-set
ordinary-kriging fits), laplace, metro, predict.  The arms alternate, --runs times each (default 3) after one untimed warm-up
call per entry point; the record holds every run and the median.  The sequential arm's Laplace stage is timed by wrapping
fit.laplace, its calls are counted at the evaluator.  --arm sequential --root <tree> runs that arm alone on another build of
the package (it touches no code of the lockstep path), e.g. a build of the parent commit.
Run from the repository root:  python scripts/study_timing.py [--runs 3] [--out profiles/study_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

SETTINGS = dict(N=5000, samp_size=1000, batch_size=20, alpha_geweke=0.5, net_samp_size=1000, alpha=0.05)
START = np.array([1.0, 1.0, 0.0])


def gv_sets(read_table):
    out = []
    for size, count in ((50, 9), (90, 8)):
        for i in range(1, count + 1):
            _, tr = read_table('tests/golden/data/gv/train_%d_%d.txt' % (size, i))
            _, te = read_table('tests/golden/data/gv/test_%d_%d.txt' % (size, i))
            out.append((tr[:, :9], tr[:, 9], te[:, :9], te[:, 9]))
    return out


def sequential(fit, gp, sets, speculate):
    secs = dict(sigma2=0.0, laplace=0.0, metro=0.0, predict=0.0)
    calls = dict(sigma2=0, laplace=0, metro=0, predict=0)
    inner = fit.laplace
    state = dict(in_laplace=False)

    def timed_laplace(fn_batch, start, *a, **k):
        def counted(rows):
            calls["laplace"] += 1
            return fn_batch(rows)
        t0 = time.perf_counter()
        est = inner(counted, start, *a, **k)
        state["laplace_s"] = time.perf_counter() - t0
        return est

    fit.laplace = timed_laplace
    summaries = []
    try:
        for i, (D, y, Dt, yt) in enumerate(sets):
            t0 = time.perf_counter()
            okf = fit.ordinary_kriging_fit(gp.h, D, y)
            secs["sigma2"] += time.perf_counter() - t0
            calls["sigma2"] += okf["calls"]
            t0 = time.perf_counter()
            ff = fit.factors_frame(gp, START, SETTINGS["N"], SETTINGS["samp_size"], SETTINGS["batch_size"],
                                   SETTINGS["alpha_geweke"], D, okf["sigma2"], y, SETTINGS["net_samp_size"],
                                   rng=np.random.default_rng(i + 1), speculate=speculate)
            both = time.perf_counter() - t0
            secs["laplace"] += state["laplace_s"]
            secs["metro"] += both - state["laplace_s"]
            calls["metro"] += ff["chain"]["device_batches"] + 1
            t0 = time.perf_counter()
            table = fit.compare_GP(gp, Dt, SETTINGS["alpha"], yt, ff["draws"], D, okf["sigma2"], y, exact=True)
            secs["predict"] += time.perf_counter() - t0
            calls["predict"] += 1
            summaries.append(fit.comparison_summary(table))
    finally:
        fit.laplace = inner
    return dict(seconds=secs, calls=calls, total=sum(secs.values()), rmspe=[s["rmspe"] for s in summaries])


def lockstep(fit, gp, sets, speculate):
    t0 = time.perf_counter()
    r = fit.study(gp, sets, SETTINGS["alpha"], SETTINGS["N"], SETTINGS["samp_size"], SETTINGS["batch_size"],
                  SETTINGS["alpha_geweke"], net_samp_size=SETTINGS["net_samp_size"], start=START,
                  rngs=[i + 1 for i in range(len(sets))], speculate=speculate)
    wall = time.perf_counter() - t0
    return dict(seconds=r["seconds"], calls=r["calls"], total=sum(r["seconds"].values()), wall=wall,
                rmspe=[s["rmspe"] for s in r["summaries"]], pooled=r["pooled"],
                proposals=[c["proposals"] for c in r["chains"]], accepted=[c["accepted"] for c in r["chains"]])


def median_of(runs):
    out = dict(total=float(np.median([r["total"] for r in runs])))
    for part in ("sigma2", "laplace", "metro", "predict"):
        out[part] = float(np.median([r["seconds"][part] for r in runs]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arm", choices=("both", "sequential"), default="both")
    ap.add_argument("--root", default=".")
    ap.add_argument("--speculate", type=int, nargs="*", default=[0, 3])
    ap.add_argument("--out", default=os.path.join("profiles", "study_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table

    sets = gv_sets(read_table)
    h = api.Handle(0)
    gp = CombinedGP("GV", handle=h)
    # warm-up: code objects, staging and pinned buffers of every entry point the arms use
    D, y, Dt, yt = sets[0]
    s2 = fit.ordinary_kriging_fit(h, D, y, starts=2)["sigma2"]
    fit.logpost_batch(gp, D, START[None], y, s2)
    fit.compare_GP(gp, Dt, 0.05, yt, fit.transformed_to_draws(np.tile(START, (4, 1))), D, s2, y, exact=True)
    if args.arm == "both":
        gp.logpost_sets(np.stack([D, D]), np.tile(START, (3, 1)), np.stack([y, y]), [s2, s2], [0, 1, 0])
    out = dict(settings=SETTINGS, sets=[list(s[0].shape) for s in sets], package=os.path.abspath(args.root))
    for m in args.speculate:
        rec = out["speculate_%d" % m] = dict(sequential=[], lockstep=[])
        for run in range(args.runs):
            rec["sequential"].append(sequential(fit, gp, sets, m))
            print("speculate %d run %d sequential" % (m, run), json.dumps(rec["sequential"][-1]), flush=True)
            if args.arm == "both":
                rec["lockstep"].append(lockstep(fit, gp, sets, m))
                print("speculate %d run %d lockstep  " % (m, run), json.dumps(rec["lockstep"][-1]), flush=True)
        rec["median"] = dict(sequential=median_of(rec["sequential"]))
        if args.arm == "both":
            rec["median"]["lockstep"] = median_of(rec["lockstep"])
            rec["median"]["speedup_total"] = rec["median"]["sequential"]["total"] / rec["median"]["lockstep"]["total"]
            fitted = ("laplace", "metro")
            rec["median"]["speedup_fit"] = sum(rec["median"]["sequential"][p] for p in fitted) / \
                sum(rec["median"]["lockstep"][p] for p in fitted)
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
