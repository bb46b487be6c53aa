"""The 1-D fit two ways, timed, and one likelihood call with CCGP_OPT_FAMILY_FUSED off and on (profiles/family_fused.md).

The fit: D1's own settings (D1:1079-1100) -- n = 8, Matern nu = 5, start (0, 1.5, 0), N.max 10000, samp.size 5000, batch.size
20, alpha.geweke 0.5 -- on C seeded Latin-hypercube designs on [0, 1] with responses f2(x) = sin(10 x) (D1:331-339), sigma2
from fit.matern_MLEs (untimed, option off in both arms), one generator per design seeded with the design's number.
  arm A  fit.laplace_sets over the twin evaluator + fit.Metro_device_sets on a build WITHOUT the fused route (--parent <tree>,
         a build of the parent commit): the device refuses the family, so search and chains run on the host twin, every
         evaluation a ccgp_chain_logpost_sets call that goes set by set through the blocked sweep;
  arm B  this build, CombinedGP1D(fused=True): fit.laplace_device_sets + fit.Metro_device_sets, search and chains inside the
         kernel.
Each run is a process of its own (two builds of one package do not share a process): an untimed warm-up of every entry point
the arm uses, then the host clock around the blocking calls.  The arms alternate, --runs times each, every chain bounded by
--cap proposals in both arms (default 60000: N.max accepted draws at an acceptance rate of one in six, which no chain here
comes near); --N and --samp-size scale the alternating runs' chains down in both arms alike where the slow arm at D1's
length is not affordable three times; then arm B alone, at D1's settings, at the designs of --alone.  Calls are counted at the C entry points (chain_logpost_sets, metro_segments_sets, laplace_search_sets;
a refused call counts).  The one call: ccgp_loglik_batch at n = 8, nu = 5, K = 2, B = 1 and B = 1000, option off and on in one
process, the median of 20 after a warm-up.
Run from the repository root:  python scripts/family_fused_timing.py --parent <parent tree> [--out profiles/family_fused.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

NU = 5.0
SETTINGS = dict(n=8, nu=NU, start=[0.0, 1.5, 0.0], N=10000, samp_size=5000, batch_size=20, alpha_geweke=0.5)
MAX_PROPOSALS = 60000   # per chain: N.max accepted draws at an acceptance rate of one in six
COUNTED = ("chain_logpost_sets", "metro_segments_sets", "laplace_search_sets")


def designs(C, n=8):
    out = []
    for c in range(C):
        rng = np.random.default_rng(1000 + c)
        x = (rng.permutation(n) + rng.random(n)) / n
        out.append((x[:, None], np.sin(10.0 * x)))
    return out


def count_calls(api):
    calls = dict.fromkeys(COUNTED, 0)
    for name in COUNTED:
        inner = getattr(api.Handle, name)

        def counted(self, *a, _inner=inner, _name=name, **k):
            calls[_name] += 1
            return _inner(self, *a, **k)
        setattr(api.Handle, name, counted)
    return calls


def run_arm(arm, root, C, cap, N, samp_size):
    sys.path.insert(0, root)
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP1D

    calls = count_calls(api)
    h = api.Handle(0)
    gp = CombinedGP1D(NU, handle=h, fused=True) if arm == "B" else CombinedGP1D(NU, handle=h)
    sets = designs(C)
    Ds, ys = [s[0] for s in sets], [s[1] for s in sets]
    s2 = [fit.matern_MLEs(h, D, y, NU)["sigma2"] for D, y in sets]
    starts = np.tile(np.array(SETTINGS["start"]), (C, 1))
    kw = dict(N=N, samp_size=samp_size, batch_size=SETTINGS["batch_size"], alpha=SETTINGS["alpha_geweke"])

    def fit_all(short):
        # (the warm-up searches to the end as well: a chain started from an unconverged search need not move at all; every
        # chain is bounded in proposals, the timed ones far above what N.max accepted draws take -- the record says if one got there)
        k = dict(kw, N=40, samp_size=20, max_proposals=400) if short else dict(kw, max_proposals=cap)
        t0 = time.perf_counter()
        if arm == "A":
            fn = fit._twin_sets_evaluator(gp, Ds, ys, s2, None, None)
            ests = fit.laplace_sets(lambda rows, set_of: fn(np.asarray(rows), np.asarray(set_of, dtype=np.int64))[0], starts)
        else:
            ests = fit.laplace_device_sets(gp, Ds, ys, s2, starts)
        t1 = time.perf_counter()
        r = fit.Metro_device_sets(gp, None, D_trains=Ds, sigma2s=s2, ys=ys, rngs=[c + 1 for c in range(C)], laplace=ests, **k)
        t2 = time.perf_counter()
        return ests, r, t1 - t0, t2 - t1

    fit_all(True)                                    # warm-up: code objects, staging and pinned buffers
    for name in COUNTED:
        calls[name] = 0
    ests, r, t_lap, t_metro = fit_all(False)
    props = [c["proposals"] for c in r["chains"]]
    out = dict(arm=arm, designs=C, N=N, samp_size=samp_size, seconds=t_lap + t_metro, laplace_seconds=t_lap, metro_seconds=t_metro, calls=dict(calls),
               device_calls=sum(calls.values()), proposals=props, accepted=[c["accepted"] for c in r["chains"]],
               us_per_proposal_longest=1e6 * t_metro / max(props), max_proposals=cap, capped=[bool(p >= cap) for p in props],
               laplace_converged=[bool(e["converged"]) for e in ests],
               package=os.path.abspath(root))
    h.close()
    return out


def one_call(root):
    sys.path.insert(0, root)
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api

    h = api.Handle(0)
    x, y = designs(1)[0]
    rng = np.random.default_rng(7)
    out = {}
    h.set_kernel(api.KERNEL_MATERN, NU)
    try:
        for B in (1, 1000):
            P = np.column_stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.3, 0.9, B), rng.uniform(0.2, 0.4, B), rng.uniform(0.2, 0.4, B)])
            for on in (0, 1):
                h.set_option(api.OPT_FAMILY_FUSED, on)
                for _ in range(3):
                    h.loglik_batch(x, y, 2, P, 1.0)
                t = []
                for _ in range(20):
                    t0 = time.perf_counter()
                    h.loglik_batch(x, y, 2, P, 1.0)
                    t.append(time.perf_counter() - t0)
                out["B%d_option%d_us" % (B, on)] = dict(median=1e6 * float(np.median(t)), min=1e6 * min(t), max=1e6 * max(t))
    finally:
        h.set_option(api.OPT_FAMILY_FUSED, 0)
        h.set_kernel(api.KERNEL_GAUSS, 0.0)
        h.close()
    return out


def child(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), *extra]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:   # the run is ended with its process; the record says so and the others go on
        rec = dict(extra=list(extra), ended_after_seconds=args.limit)
        print(json.dumps(rec), flush=True)
        return rec
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(extra), r.returncode, (r.stdout + r.stderr)[-2000:]))
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built tree of the parent commit (arm A)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--designs", type=int, default=8)
    ap.add_argument("--alone", type=int, nargs="*", default=[8, 32, 201])
    ap.add_argument("--N", type=int, default=SETTINGS["N"], help="N.max of the alternating runs (the runs of --alone keep D1's)")
    ap.add_argument("--samp-size", type=int, default=SETTINGS["samp_size"], help="samp.size of the alternating runs")
    ap.add_argument("--cap", type=int, default=MAX_PROPOSALS,
                    help="proposals a chain of the alternating runs may make (both arms; a chain that gets there without samp.size accepted draws fails its run)")
    ap.add_argument("--limit", type=float, default=600.0, help="seconds a run may take")
    ap.add_argument("--out", default=os.path.join("profiles", "family_fused.json"))
    ap.add_argument("--arm", choices=("A", "B", "call"), help="(internal) one run in this process")
    ap.add_argument("--root", default=".")
    args = ap.parse_args()
    if args.arm == "call":
        print(json.dumps(one_call(args.root)))
        return
    if args.arm:
        print(json.dumps(run_arm(args.arm, args.root, args.designs, args.cap, args.N, args.samp_size)))
        return
    if not args.parent:
        ap.error("--parent <built tree of the parent commit> is required")
    out = dict(settings=SETTINGS, alternating=dict(N=args.N, samp_size=args.samp_size, cap=args.cap), A=[], B=[], alone=[])

    def save():   # after every run: a run that does not end leaves the others' figures
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    scaled = ("--cap", str(args.cap), "--N", str(args.N), "--samp-size", str(args.samp_size))
    for _ in range(args.runs):
        out["A"].append(child(args, "--arm", "A", "--root", args.parent, "--designs", str(args.designs), *scaled))
        out["B"].append(child(args, "--arm", "B", "--root", ".", "--designs", str(args.designs), *scaled))
        save()
    for C in args.alone:
        out["alone"].append(child(args, "--arm", "B", "--root", ".", "--designs", str(C)))
        save()
    out["one_call"] = child(args, "--arm", "call", "--root", ".")
    # (a run ended at its limit counts with the limit: a lower bound of its time)
    a = [r.get("seconds", r.get("ended_after_seconds")) for r in out["A"]]
    b = [r.get("seconds", r.get("ended_after_seconds")) for r in out["B"]]
    out["condition"] = dict(A_fastest=min(a), B_slowest=max(b), met=bool(max(b) < min(a)))
    print(json.dumps(out["condition"]))
    save()


if __name__ == "__main__":
    main()
