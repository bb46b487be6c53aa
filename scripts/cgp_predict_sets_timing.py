"""The CGP columns of the Ground-Vibrations study's tables two ways, timed: cgp.predict_CGP per set (one ccgp_cgp_predict call
each: the set, its model and its test sites go up, the state launch and the site launch run for one row, the table comes
back) against cgp.predict_CGP_sets (one ccgp_cgp_predict_sets call per group of one shape: one state launch for all the
group's rows, one site launch over rows x sites).  Sets are those of scripts/study_timing.py: the nine size-50 and eight
size-90 sets with their own 150 test sites each; the models are fitted once (cgp.CGP_sets, five starts, seed 0, refinement on
the device) and given to both arms.  Both arms return the same dicts bit for bit -- the script asserts it after every run --
so the figures to compare are the seconds.

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  Then, once per arm with the handle's event timing on, the kernel time of the same work (state and site
launches, CCGP_T_FUSED) and what remains of the wall time: staging, copies, synchronisation and the host.
Run from the repository root:  python scripts/cgp_predict_sets_timing.py [--runs 3] [--out profiles/cgp_predict_sets.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "cgp_predict_sets.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, cgp
    from ccgp_amd.tables import read_table

    h = api.Handle(0)
    ests, news = [], []
    for size, count in ((50, 9), (90, 8)):
        Ds, ys = [], []
        for i in range(1, count + 1):
            _, tr = read_table("tests/golden/data/gv/train_%d_%d.txt" % (size, i))
            _, te = read_table("tests/golden/data/gv/test_%d_%d.txt" % (size, i))
            Ds.append(tr[:, :9])
            ys.append(tr[:, 9])
            news.append(te[:, :9])
        ests += cgp.CGP_sets(h, Ds, ys, on_device=True)

    def per_set():
        return [cgp.predict_CGP(h, e, u, PI=True) for e, u in zip(ests, news)]

    def lockstep():
        return cgp.predict_CGP_sets(h, ests, news, PI=True)

    arms = dict(per_set=per_set, lockstep=lockstep)

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w)
            for k in w:
                assert np.asarray(g[k]).tobytes() == np.asarray(w[k]).tobytes(), k

    ref = per_set()          # warm-up of both arms: code objects, staging and pinned buffers
    same(lockstep(), ref)
    runs = {a: [] for a in arms}
    for run in range(args.runs):
        for a, fn in arms.items():
            t0 = time.perf_counter()
            got = fn()
            runs[a].append(time.perf_counter() - t0)
            same(got, ref)
            print(a, "run", run, "%.6f s" % runs[a][-1], flush=True)
    division = {}
    for a, fn in arms.items():
        h.enable_timing(True)
        try:
            t0 = time.perf_counter()
            got = fn()
            wall = time.perf_counter() - t0
            ms, sections = h.get_timing()["fused"]
        finally:
            h.enable_timing(False)
        same(got, ref)
        division[a] = dict(wall_seconds_with_events=wall, kernel_seconds=ms / 1e3, timed_sections=sections,
                           outside_kernels_seconds=float(np.median(runs[a])) - ms / 1e3)
    summary = {a: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for a, v in runs.items()}
    summary["ratio"] = summary["per_set"]["median"] / summary["lockstep"]["median"]
    # the condition: the lockstep arm's slowest run below the per-set arm's fastest
    summary["separated"] = bool(summary["lockstep"]["max"] < summary["per_set"]["min"])
    summary["same_tables"] = True
    out = dict(sets=[[9, 50], [8, 90]], sites=150, device_calls=dict(per_set=len(ests), lockstep=2), runs=runs, summary=summary,
               division=division)
    print(json.dumps(dict(summary=summary, division=division), indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
