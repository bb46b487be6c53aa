"""What the 1-D scripts do after the chain, timed with CCGP_OPT_FAMILY_FUSED_PREDICT off (a build of the parent commit, which
has no such option: the blocked sweep) and on (this build) -- profiles/family_fused_predict.md.

D1's shape: n = 8, Matern nu = 5, K = 2, 2500 posterior draws, 50 test sites; seeded Latin-hypercube designs on [0, 1] with
responses sin(10 x) (scripts/family_fused_timing.designs), draws with p in (0.3, 0.7) and theta in (0.2, 0.4), sigma2 = 1.
Timed, per run:
  predict_summary    ccgp_predict_summary, 2500 draws x 50 sites (compare.GP / prediction, D1:825-844)
  loo_summary        ccgp_loo_summary, 2500 draws
  prediction_single  ccgp_krige_predict_batch with K = 1, one model, 50 sites (prediction.single, D1:548-567)
  loop8, loop201     ccgp_predict_summary once per design over 8 and over 201 designs
  arm A  the parent build (--parent <tree>): every call on the blocked sweep;
  arm B  this build with the option on.
Each run is a process of its own: an untimed warm-up of every entry point used, then the host clock around the blocking
calls -- the median of --reps calls for the three single calls, one pass for the loops.  The arms alternate, --runs times each.
The condition: arm B's slowest run below arm A's fastest, for predict_summary and for loo_summary.
--arm share: arm B's predict_summary --reps times and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats) that
gives site_corr_family_kernel's share of the call.
Run from the repository root:  python scripts/family_fused_predict_timing.py --parent <parent tree> [--out <json>]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

NU = 5.0
SHAPE = dict(n=8, nu=NU, K=2, draws=2500, sites=50)
LEVELS = (0.025, 0.975)


def designs(C, n=8):
    out = []
    for c in range(C):
        rng = np.random.default_rng(1000 + c)
        x = (rng.permutation(n) + rng.random(n)) / n
        out.append((x[:, None], np.sin(10.0 * x)))
    return out


def inputs():
    rng = np.random.default_rng(7)
    S = SHAPE["draws"]
    p = rng.uniform(0.3, 0.7, S)
    P = np.column_stack([p, 1.0 - p, rng.uniform(0.2, 0.4, S), rng.uniform(0.2, 0.4, S)])
    return P, np.linspace(0.0, 1.0, SHAPE["sites"])[:, None]


def run_arm(arm, root, reps):
    sys.path.insert(0, root)
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api

    h = api.Handle(0)
    P, Xt = inputs()
    sets = designs(201)
    X, y = sets[0]
    one = np.array([[1.0, 0.3]])
    h.set_kernel(api.KERNEL_MATERN, NU)
    if arm != "A":
        h.set_option(api.OPT_FAMILY_FUSED_PREDICT, 1)

    calls = dict(predict_summary=lambda D=X, r=y: h.predict_summary(D, r, 2, P, Xt, 1.0, LEVELS),
                 loo_summary=lambda: h.loo_summary(X, y, 2, P, 1.0, LEVELS),
                 prediction_single=lambda: h.krige_predict_batch(X, y, 1, one, None, Xt, api.VAR_UNBIASED))

    def timed(fn):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return dict(median_us=1e6 * float(np.median(t)), min_us=1e6 * min(t), max_us=1e6 * max(t))

    try:
        for fn in calls.values():                       # warm-up: code objects, workspace, staging and pinned buffers
            fn()
            fn()
        if arm == "share":
            out = dict(arm=arm, predict_summary=timed(calls["predict_summary"]))
        else:
            h.enable_timing(True)
            r = calls["predict_summary"]()
            tiers = {k: v[1] for k, v in h.get_timing().items()}
            h.enable_timing(False)
            out = dict(arm=arm, package=os.path.abspath(root), tiers=tiers, failed=int(r["n_failed"]))
            for name, fn in calls.items():
                out[name] = timed(fn)
            for C in (8, 201):
                t0 = time.perf_counter()
                for D, resp in sets[:C]:
                    calls["predict_summary"](D, resp)
                out["loop%d_seconds" % C] = time.perf_counter() - t0
    finally:
        if arm != "A":
            h.set_option(api.OPT_FAMILY_FUSED_PREDICT, 0)
        h.set_kernel(api.KERNEL_GAUSS, 0.0)
        h.close()
    return out


def child(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(extra), r.returncode, (r.stdout + r.stderr)[-2000:]))
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built tree of the parent commit (arm A)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a run may take")
    ap.add_argument("--out", default=os.path.join("profiles", "family_fused_predict.json"))
    ap.add_argument("--arm", choices=("A", "B", "share"), help="(internal) one run in this process")
    ap.add_argument("--root", default=".")
    args = ap.parse_args()
    if args.arm:
        print(json.dumps(run_arm(args.arm, args.root, args.reps)))
        return
    if not args.parent:
        ap.error("--parent <built tree of the parent commit> is required")
    out = dict(shape=SHAPE, reps=args.reps, A=[], B=[])

    def save():   # after every run
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    for _ in range(args.runs):
        out["A"].append(child(args, "--arm", "A", "--root", args.parent))
        out["B"].append(child(args, "--arm", "B", "--root", "."))
        save()
    cond = {}
    for name in ("predict_summary", "loo_summary", "prediction_single"):
        a, b = [r[name]["median_us"] for r in out["A"]], [r[name]["median_us"] for r in out["B"]]
        cond[name] = dict(A_fastest_us=min(a), B_slowest_us=max(b), met=bool(max(b) < min(a)), ratio=min(a) / max(b))
    for name in ("loop8_seconds", "loop201_seconds"):
        a, b = [r[name] for r in out["A"]], [r[name] for r in out["B"]]
        cond[name] = dict(A_fastest=min(a), B_slowest=max(b), met=bool(max(b) < min(a)), ratio=min(a) / max(b))
    out["condition"] = cond
    print(json.dumps(cond))
    save()


if __name__ == "__main__":
    main()
