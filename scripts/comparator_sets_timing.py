"""The Ground-Vibrations simulation study with all three models of compare.GP's table -- fit.study(cgp=True, single=True) -- two
ways, timed: the comparator fits per set (lockstep_fits=False: ordinary_kriging_fit for sigma2, the same fit again and cgp.CGP
inside compare_GP) against the comparator fits in lockstep across the sets of a shape (lockstep_fits=True:
ordinary_kriging_fit_sets, cgp.CGP_sets).  Sets and settings: those of scripts/study_timing.py (the nine size-50 and eight
size-90 pairs under tests/golden/data/gv; GV:691-697), one generator per set seeded with the set's number, speculate 0.

Per arm and run: wall time (host clock around blocking calls) and device calls of the six parts -- sigma2, single, cgp,
laplace, metro, predict.  In the per-set arm the single and cgp fits happen inside compare_GP; they are timed here by wrapping
fit.ordinary_kriging_fit and cgp.CGP, `single` is what the wrapped fit took beyond the sigma2 part, and `predict` is reported
without them.  The arms alternate, --runs times each (default 3) after one untimed warm-up of every entry point; the record
holds every run, the median and the range.  Both arms must produce the same 17 tables: asserted here, column by column, bit
for bit.  The condition of the work -- sigma2 + single + cgp of the lockstep arm below the per-set arm's -- is asserted on the
medians.  --arm per_set --root <tree> runs the per-set arm alone on another build of the package, e.g. the parent commit's (a
tree without lockstep_fits runs fit.study as it is there); the record's `package` is "this tree" without --root and --label's
text with it (e.g. --label "a build of the parent commit (--root)"), never a path.  --bench <file> ...: records of
`python bench.py` runs to store beside the timings (the headline on parent and new build, run alternately by the caller).
Run from the repository root:  python scripts/comparator_sets_timing.py [--runs 3] [--out profiles/comparator_sets_timing.json]"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

from study_timing import SETTINGS, START, gv_sets

PARTS = ("sigma2", "single", "cgp", "laplace", "metro", "predict")
COMPARATORS = ("sigma2", "single", "cgp")


def run_study(fit, cgp, gp, sets, lockstep_fits):
    """One study -> (record, tables).  lockstep_fits None: a tree whose fit.study has no such keyword."""
    took = dict(okf=0.0, cgp=0.0)
    inner_okf, inner_cgp = fit.ordinary_kriging_fit, cgp.CGP

    def timed(key, fn):
        def wrapped(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                took[key] += time.perf_counter() - t0
        return wrapped

    fit.ordinary_kriging_fit, cgp.CGP = timed("okf", inner_okf), timed("cgp", inner_cgp)
    kw = {} if lockstep_fits is None else dict(lockstep_fits=lockstep_fits)
    try:
        t0 = time.perf_counter()
        r = fit.study(gp, sets, SETTINGS["alpha"], SETTINGS["N"], SETTINGS["samp_size"], SETTINGS["batch_size"],
                      SETTINGS["alpha_geweke"], net_samp_size=SETTINGS["net_samp_size"], start=START,
                      rngs=[i + 1 for i in range(len(sets))], cgp=True, single=True, **kw)
        wall = time.perf_counter() - t0
    finally:
        fit.ordinary_kriging_fit, cgp.CGP = inner_okf, inner_cgp
    secs = {p: float(r["seconds"].get(p, 0.0)) for p in PARTS}
    calls = {p: int(r["calls"].get(p, 0)) for p in PARTS}
    if not lockstep_fits:   # the fits compare_GP made: out of predict, into their own parts
        secs["single"] = took["okf"] - secs["sigma2"]
        secs["cgp"] = took["cgp"]
        secs["predict"] -= secs["single"] + secs["cgp"]
        if not calls["single"]:
            calls["single"] = sum(int(t["single"]["calls"]) for t in r["tables"])
            calls["cgp"] = sum(int(t["CGP"]["calls"]) for t in r["tables"])
    rec = dict(seconds=secs, calls=calls, total=sum(secs.values()), wall=wall, comparators=sum(secs[p] for p in COMPARATORS),
               rmspe=[s["rmspe"] for s in r["summaries"]], rmspe_CGP=[s["rmspe_CGP"] for s in r["summaries"]],
               rmspe_single=[s["rmspe_single"] for s in r["summaries"]])
    return rec, r["tables"]


def same_tables(a, b):
    assert len(a) == len(b) == 17
    for ta, tb in zip(a, b):
        cols = [k for k, v in ta.items() if isinstance(v, np.ndarray)]
        assert cols and sorted(cols) == sorted(k for k, v in tb.items() if isinstance(v, np.ndarray))
        for k in cols:
            np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
        for k in ("theta", "sigma2", "beta", "loglik"):
            np.testing.assert_array_equal(ta["single"][k], tb["single"][k], err_msg="single " + k)
        for k in ("par", "theta", "alpha", "Yp_jackknife", "temp_matrix"):
            np.testing.assert_array_equal(ta["CGP"][k], tb["CGP"][k], err_msg="CGP " + k)


def summary_of(runs):
    out = {}
    for key in ("total", "wall", "comparators"):
        v = [r[key] for r in runs]
        out[key] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    for p in PARTS:
        v = [r["seconds"][p] for r in runs]
        out[p] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), calls=runs[0]["calls"][p])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arm", choices=("both", "per_set"), default="both")
    ap.add_argument("--root", default=".")
    ap.add_argument("--label", default=None, help="what the record calls the build it ran (never a path)")
    ap.add_argument("--bench", nargs="*", default=[], help="label=path of bench.py result lines to store in the record")
    ap.add_argument("--merge", nargs="*", default=[], help="label=path of records of other runs of this script to store")
    ap.add_argument("--out", default=os.path.join("profiles", "comparator_sets_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, cgp, fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table

    has_kw = "lockstep_fits" in inspect.signature(fit.study).parameters
    if args.arm == "both" and not has_kw:
        raise SystemExit("this tree's fit.study has no lockstep_fits: run it with --arm per_set")
    sets = gv_sets(read_table)
    h = api.Handle(0)
    gp = CombinedGP("GV", handle=h)
    # warm-up: code objects, staging and pinned buffers of every entry point the arms use
    D, y, Dt, yt = sets[0]
    s2 = fit.ordinary_kriging_fit(h, D, y, starts=2)["sigma2"]
    fit.logpost_batch(gp, D, START[None], y, s2)
    gp.logpost_sets(np.stack([D, D]), np.tile(START, (3, 1)), np.stack([y, y]), [s2, s2], [0, 1, 0])
    fit.compare_GP(gp, Dt, 0.05, yt, fit.transformed_to_draws(np.tile(START, (4, 1))), D, s2, y, exact=True, cgp=True, single=True)
    if args.arm == "both":
        two = [sets[0][:2], sets[1][:2]]
        fit.ordinary_kriging_fit_sets(h, [s[0] for s in two], [s[1] for s in two], starts=2)
        cgp.CGP_sets(h, [s[0] for s in two], [s[1] for s in two])
    # the record names the build by a label, not by where the tree lies: the same on every machine
    label = args.label or ("this tree" if args.root == "." else "another build (--root)")
    out = dict(settings=SETTINGS, sets=[list(s[0].shape) for s in sets], package=label,
               study="fit.study(cgp=True, single=True), speculate 0", per_set=[], lockstep=[])
    ref = None
    for run in range(args.runs):
        rec, tables = run_study(fit, cgp, gp, sets, False if has_kw else None)
        out["per_set"].append(rec)
        print("run %d per_set " % run, json.dumps(rec), flush=True)
        if ref is None:
            ref = tables
        else:
            same_tables(tables, ref)
        if args.arm == "both":
            rec, tables = run_study(fit, cgp, gp, sets, True)
            out["lockstep"].append(rec)
            print("run %d lockstep" % run, json.dumps(rec), flush=True)
            same_tables(tables, ref)   # both arms, every run: the same 17 tables
    h.close()
    out["summary"] = dict(per_set=summary_of(out["per_set"]))
    if args.arm == "both":
        out["summary"]["lockstep"] = summary_of(out["lockstep"])
        a, b = out["summary"]["per_set"], out["summary"]["lockstep"]
        out["summary"]["comparators_ratio"] = a["comparators"]["median"] / b["comparators"]["median"]
        out["summary"]["total_ratio"] = a["total"]["median"] / b["total"]["median"]
        out["tables_identical"] = True
    else:
        del out["lockstep"]
    for item in args.merge:
        label, path = item.split("=", 1)
        with open(path) as fh:
            out[label] = json.load(fh)
    for item in args.bench:
        label, path = item.split("=", 1)
        with open(path) as fh:
            out.setdefault("bench", {})[label] = [json.loads(line) for line in fh if line.strip().startswith("{")]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if args.arm == "both":
        print("comparators (sigma2 + single + cgp): per set %.3f s, lockstep %.3f s, ratio %.2f" % (
            a["comparators"]["median"], b["comparators"]["median"], out["summary"]["comparators_ratio"]))
        assert b["comparators"]["median"] < a["comparators"]["median"], "the lockstep comparator fits are not faster"


if __name__ == "__main__":
    main()
