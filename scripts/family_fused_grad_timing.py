"""The step in front of the 1-D scripts' chains -- MLEs() (D1:455-471), the ordinary-kriging fit that yields sigma2 -- timed
design by design (fit.matern_MLEs(fused=True): a 96-point grid and a bounded scalar search per design) against all designs in
lockstep on the analytic gradient (fit.matern_MLEs_sets, CCGP_OPT_FAMILY_FUSED_GRAD) -- profiles/family_fused_grad.md.

D1's shape: n = 8, Matern nu = 5, y = sin 10 x on seeded Latin-hypercube designs of [0, 1]
(scripts/family_fused_predict_timing.designs).  Per run:
  mles8, mles201            fit.matern_MLEs(fused=True) per design over 8 and over 201 designs: seconds, device calls
  sets8, sets201            fit.matern_MLEs_sets over the same designs (arm B only): seconds, device calls, and the largest
                            |l_p difference| to the per-design fit
  grad_b1, grad_b1000       one ccgp_profile_batch(grad=True) at B = 1 and B = 1000 rows, K = 2 (arm B only): median of --reps
  arm A  a build of the parent commit (--parent <tree>): the per-design fit only -- it has neither the option nor the gradient;
  arm B  this build.
Each run is a process of its own: an untimed warm-up of every entry point used, then the host clock around the blocking calls.
The arms alternate, --runs times each; the summary sets the slowest lockstep run against the fastest per-design run of
either arm.  Nothing is asserted: the figures are recorded.
Run from the repository root:  python scripts/family_fused_grad_timing.py --parent <parent tree> [--out <json>]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

NU = 5.0
SHAPE = dict(n=8, nu=NU, designs=(8, 201))


def designs(C, n=8):
    out = []
    for c in range(C):
        rng = np.random.default_rng(1000 + c)
        x = (rng.permutation(n) + rng.random(n)) / n
        out.append((x, np.sin(10.0 * x)))
    return out


class Counting:
    """A handle proxy that counts the calls made through it (every one of them is one blocking C-ABI call)."""

    def __init__(self, h):
        self._h, self.calls = h, 0

    def __getattr__(self, name):
        attr = getattr(self._h, name)
        if not callable(attr) or name in ("close", "set_kernel", "set_option"):
            return attr

        def call(*a, **k):
            self.calls += 1
            return attr(*a, **k)
        return call


def run_arm(arm, root, reps):
    sys.path.insert(0, root)
    import ccgp_amd  # noqa: F401
    from ccgp_amd import api, fit

    h = api.Handle(0)
    sets = designs(201)
    out = dict(arm=arm, package=os.path.abspath(root))
    try:
        fit.matern_MLEs(h, sets[0][0], sets[0][1], NU, fused=True)                       # warm-up
        if arm == "B":
            fit.matern_MLEs_sets(h, [s[0] for s in sets[:2]], [s[1] for s in sets[:2]], NU)
        singles = {}
        for C in SHAPE["designs"]:
            hc = Counting(h)
            t0 = time.perf_counter()
            singles[C] = [fit.matern_MLEs(hc, D, y, NU, fused=True) for D, y in sets[:C]]
            out["mles%d" % C] = dict(seconds=time.perf_counter() - t0, calls=hc.calls)
        if arm == "B":
            n = SHAPE["n"]
            for C in SHAPE["designs"]:
                hc = Counting(h)
                t0 = time.perf_counter()
                r = fit.matern_MLEs_sets(hc, [s[0] for s in sets[:C]], [s[1] for s in sets[:C]], NU)
                dt = time.perf_counter() - t0
                lp = [fit.matern_profile(h, sets[c][0], sets[c][1], NU, [singles[C][c]["theta"]], fused_grad=True)["loglikeli"][0]
                      for c in range(C)]
                lp = [-(v + n * np.log(2.0 * np.pi) + n) / 2.0 for v in lp]
                out["sets%d" % C] = dict(seconds=dt, calls=hc.calls, max_lp_difference=float(max(abs(r[c]["loglik"] - lp[c]) for c in range(C))),
                                         lockstep_below_single=int(sum(r[c]["loglik"] < lp[c] - 1e-9 for c in range(C))))
            X, y = sets[0][0][:, None], sets[0][1]
            rng = np.random.default_rng(7)
            h.set_kernel(api.KERNEL_MATERN, NU)
            h.set_option(api.OPT_FAMILY_FUSED_GRAD, 1)
            for B in (1, 1000):
                p = rng.uniform(0.3, 0.7, B)
                P = np.column_stack([p, 1.0 - p, rng.uniform(0.2, 0.4, B), rng.uniform(0.2, 0.4, B)])
                h.profile_batch(X, y, 2, P, grad=True)
                t = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    st = h.profile_batch(X, y, 2, P, grad=True)[4]
                    t.append(time.perf_counter() - t0)
                out["grad_b%d" % B] = dict(median_us=1e6 * float(np.median(t)), min_us=1e6 * min(t), max_us=1e6 * max(t), failed=int((st != 0).sum()))
    finally:
        if arm == "B":
            h.set_option(api.OPT_FAMILY_FUSED_GRAD, 0)
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
    ap.add_argument("--out", default=os.path.join("profiles", "family_fused_grad.json"))
    ap.add_argument("--arm", choices=("A", "B"), help="(internal) one run in this process")
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
    summary = {}
    for C in SHAPE["designs"]:
        single = [r["mles%d" % C]["seconds"] for r in out["A"] + out["B"]]
        lock = [r["sets%d" % C]["seconds"] for r in out["B"]]
        summary["designs%d" % C] = dict(single_fastest_s=min(single), single_slowest_s=max(single), lockstep_fastest_s=min(lock),
                                        lockstep_slowest_s=max(lock), ratio=min(single) / max(lock),
                                        single_calls=out["B"][0]["mles%d" % C]["calls"], lockstep_calls=out["B"][0]["sets%d" % C]["calls"])
    out["summary"] = summary
    print(json.dumps(summary))
    save()


if __name__ == "__main__":
    main()
