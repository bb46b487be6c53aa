"""The prediction stage of the Ground-Vibrations study two ways, timed: fit.compare_GP per set (per set one
ccgp_predict_summary, one ccgp_krige_predict_batch and one ccgp_cgp_predict call) against fit.compare_GP_sets (per shape one
ccgp_predict_summary_sets, one ccgp_krige_predict_batch_sets and one ccgp_cgp_predict_sets call); and, separately, the Combined
GP alone: Handle.predict_summary per set against Handle.predict_summary_sets.  Sets are those of scripts/study_timing.py: the
nine size-50 and eight size-90 sets with their own 150 test sites, --draws (1000) draws each in the range the chains visit;
the single-GP and CGP models are fitted once and given to both arms.  Both arms return the same tables bit for bit -- the
script asserts it after every run -- so the figures to compare are the seconds.

The arms alternate in one process, --runs times each (default 3) after one untimed warm-up each, the host clock around the
blocking calls.  Then, once per arm with the handle's event timing on, the kernel time of the same work and what remains of
the wall time: staging, copies, synchronisation and the host.
Run from the repository root:  python scripts/predict_sets_timing.py [--runs 3] [--draws 1000] [--out profiles/predict_sets.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("profiles", "predict_sets.json"))
    args = ap.parse_args()
    sys.path.insert(0, ".")
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, cgp, fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table

    h = api.Handle(0)
    gp = CombinedGP("GV", handle=h)
    rng = np.random.default_rng(0)
    sets, krige, cgps = [], [], []
    for size, count in ((50, 9), (90, 8)):
        group = []
        for i in range(1, count + 1):
            _, tr = read_table("tests/golden/data/gv/train_%d_%d.txt" % (size, i))
            _, te = read_table("tests/golden/data/gv/test_%d_%d.txt" % (size, i))
            group.append((tr[:, :9], tr[:, 9], te[:, :9], te[:, 9]))
        krige += fit.ordinary_kriging_fit_sets(h, [s[0] for s in group], [s[1] for s in group])
        cgps += cgp.CGP_sets(h, [s[0] for s in group], [s[1] for s in group], on_device=True)
        sets += group
    C, S = len(sets), args.draws
    draws = [np.column_stack([rng.uniform(0.2, 0.8, S), rng.uniform(0.03, 0.15, S), rng.uniform(0.8, 3.0, S)]) for _ in sets]
    s2 = [k["sigma2"] for k in krige]
    cg, sg = [dict(est=e) for e in cgps], [dict(est=e) for e in krige]
    Dt, yt, D, y = [s[2] for s in sets], [s[3] for s in sets], [s[0] for s in sets], [s[1] for s in sets]
    params = [gp.draws_to_params(D[i], draws[i]) for i in range(C)]
    probs = (0.025, 0.975)
    shapes = sorted({d.shape for d in D}, reverse=True)

    def tables_per_set():
        return [fit.compare_GP(gp, Dt[i], 0.05, yt[i], draws[i], D[i], s2[i], y[i], exact=True, cgp=cg[i], single=sg[i])
                for i in range(C)]

    def tables_lockstep():
        return fit.compare_GP_sets(gp, Dt, 0.05, yt, draws, D, s2, y, cgp=cg, single=sg)

    def summary_per_set():
        return [h.predict_summary(D[i], y[i], 2, params[i], Dt[i], s2[i], probs) for i in range(C)]

    def summary_lockstep():
        out = [None] * C
        for shp in shapes:
            idx = [i for i in range(C) if D[i].shape == shp]
            res = h.predict_summary_sets(np.stack([D[i] for i in idx]), np.stack([y[i] for i in idx]), [s2[i] for i in idx], 2,
                                         np.concatenate([params[i] for i in idx]), np.repeat(np.arange(len(idx)), S),
                                         np.stack([Dt[i] for i in idx]), probs)
            for i, r in zip(idx, res):
                out[i] = r
        return out

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w)
            for k, v in w.items():
                if isinstance(v, np.ndarray):
                    assert np.asarray(g[k]).tobytes() == v.tobytes(), k

    out = dict(sets=[[9, 50], [8, 90]], sites=150, draws=S)
    for label, arms in (("compare_GP", dict(per_set=tables_per_set, lockstep=tables_lockstep)),
                        ("predict_summary", dict(per_set=summary_per_set, lockstep=summary_lockstep))):
        ref = arms["per_set"]()          # warm-up of both arms
        same(arms["lockstep"](), ref)
        runs = {a: [] for a in arms}
        for run in range(args.runs):
            for a, fn in arms.items():
                t0 = time.perf_counter()
                got = fn()
                runs[a].append(time.perf_counter() - t0)
                same(got, ref)
                print(label, a, "run", run, "%.6f s" % runs[a][-1], flush=True)
        division = {}
        for a, fn in arms.items():
            h.enable_timing(True)
            try:
                got = fn()
                t = h.get_timing()
            finally:
                h.enable_timing(False)
            same(got, ref)
            kernel = sum(v[0] for v in t.values()) / 1e3
            division[a] = dict(kernel_seconds=kernel, timed_sections=int(sum(v[1] for v in t.values())),
                               outside_kernels_seconds=float(np.median(runs[a])) - kernel)
        summary = {a: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for a, v in runs.items()}
        summary["ratio"] = summary["per_set"]["median"] / summary["lockstep"]["median"]
        # the condition: the lockstep arm's slowest run below the per-set arm's fastest
        summary["separated"] = bool(summary["lockstep"]["max"] < summary["per_set"]["min"])
        summary["same_tables"] = True
        out[label] = dict(runs=runs, summary=summary, division=division)
        print(label, json.dumps(dict(summary=summary, division=division), indent=1))
    h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
