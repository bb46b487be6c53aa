"""Metropolis chains on the device (ccgp_metro_segments_sets, fit.Metro_device_sets) against their host twin
(ccgp_chain_logpost_sets driven one proposal at a time): every output and the whole trace bit for bit, one shape per CHAIN
instance and all four priors (tests/chain_cases.py); a chain's independence of the other chains, of its position, of how its
proposals are cut into calls and of what the handle ran before; failed factorisations; refusals; fit.study(device_chains=True)
and the posterior mean against fit.Metro."""
import math

import numpy as np
import pytest

from chain_cases import CASES, T, make_case, walk
from conftest import load_gv
from ccgp_amd import api, fit
from ccgp_amd.rsurface import CombinedGP

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def twin_walk(h, case):
    def ev(theta):
        val, beta, _, st = h.chain_logpost_sets(case["D"][None], case["y"][None], [case["s2"]], case["prior"], theta[None], [0],
                                                case["pars"])
        return float(val[0]), float(beta[0]), int(st[0])
    return walk(case, ev)


def device_run(h, cases, n_prop=None, stop_acc=None, state=None, t0=0, sets=None, set_of=None, trace=True):
    """The cases as chains of ONE call (they share a shape and a prior); state: (theta, l, beta) per chain to start from."""
    A = len(cases)
    c0 = cases[0]
    Xs = np.stack([c["D"] for c in (sets or cases)])
    ys = np.stack([c["y"] for c in (sets or cases)])
    s2 = [c["s2"] for c in (sets or cases)]
    if state is None:
        state = []
        for c in cases:
            v, b, _, _ = h.chain_logpost_sets(c["D"][None], c["y"][None], [c["s2"]], c["prior"], c["theta0"][None], [0], c["pars"])
            state.append((c["theta0"], float(v[0]), float(b[0])))
    steps = np.stack([c["steps"][t0:] for c in cases])
    logu = np.stack([c["logu"][t0:] for c in cases])
    tt = steps.shape[1]
    return h.metro_segments_sets(Xs, ys, s2, c0["prior"], set_of if set_of is not None else list(range(A)),
                                 np.stack([s[0] for s in state]), [s[1] for s in state], steps, logu,
                                 n_prop if n_prop is not None else [tt] * A, stop_acc if stop_acc is not None else [tt] * A,
                                 c0["pars"], [s[2] for s in state], trace=trace)


def check_against_walk(r, j, tr, used=T):
    a = sum(tr["accept"][:used])
    assert r["used"][j] == used and r["accepted"][j] == a
    assert same_bits(r["trace_val"][j, :used], tr["val"][:used]) and same_bits(r["trace_beta"][j, :used], tr["beta"][:used])
    assert np.array_equal(r["trace_status"][j, :used], tr["status"][:used])
    assert np.array_equal(r["trace_accept"][j, :used], tr["accept"][:used])
    assert same_bits(r["draws"][j, :a], np.array(tr["draws"][:a]).reshape(a, -1))
    acc_at = [t for t in range(used) if tr["accept"][t]]
    assert same_bits(r["draw_val"][j, :a], [tr["val"][t] for t in acc_at])
    assert same_bits(r["draw_beta"][j, :a], [tr["beta"][t] for t in acc_at])
    if used == len(tr["val"]):
        assert same_bits(r["theta"][j], tr["theta"]) and same_bits(r["l"][j], tr["l"]) and same_bits(r["beta"][j], tr["beta_fin"])


@pytest.mark.parametrize("case_id", range(len(CASES)), ids=["n%d-%s" % (c[0], c[2]) for c in CASES])
def test_device_chain_equals_host_twin(handle, case_id):
    case = make_case(*CASES[case_id])
    tr = twin_walk(handle, case)
    r = device_run(handle, [case])
    acc = int(r["trace_accept"][0].sum())
    print(CASES[case_id], "accepted", acc, "rejected", T - acc, "failed", r["failed"])
    assert acc >= 5 and T - acc >= 5
    check_against_walk(r, 0, tr)
    assert r["failed"] == int((r["trace_status"][0] != 0).sum())
    assert np.isnan(r["draws"][0, acc:]).all() and np.isnan(r["draw_val"][0, acc:]).all()


@pytest.fixture(scope="module")
def trio(handle):
    """Three training sets of one shape (n = 17, d = 3, ISO) with a chain each, and every chain's twin walk."""
    cases = [make_case(17, 3, "ISO", 20 + i, 0.5) for i in range(3)]
    return cases, [twin_walk(handle, c) for c in cases]


def test_independent_of_the_other_chains(handle, trio):
    cases, walks = trio
    rng = np.random.default_rng(5)
    for A in (1, 5, 17):
        pos = int(rng.integers(A))
        which = [int(v) for v in rng.integers(3, size=A)]
        which[pos] = 1
        perm = [int(v) for v in rng.permutation(3)]                 # set c of the call is training set perm[c]
        r = device_run(handle, [cases[w] for w in which], sets=[cases[p] for p in perm], set_of=[perm.index(w) for w in which])
        check_against_walk(r, pos, walks[1])
        for j, w in enumerate(which):
            check_against_walk(r, j, walks[w])


def test_independent_of_the_cut_into_calls(handle, trio):
    cases, walks = trio
    case, tr = cases[2], walks[2]
    whole = device_run(handle, [case])
    check_against_walk(whole, 0, tr)
    # 13 proposals; then until 2 more acceptances; then 1 proposal; then the rest -- each call starts where the last ended
    state, t0, vals, accs, draws = None, 0, [], [], []
    for n_prop, stop in ((13, 13), (T, 2), (1, 1), (T, T)):
        left = T - t0
        r = device_run(handle, [case], n_prop=[min(n_prop, left)], stop_acc=[min(stop, left)], state=state, t0=t0)
        u, a = int(r["used"][0]), int(r["accepted"][0])
        assert u >= 1 and (u == min(n_prop, left) or a == stop)
        vals += list(r["trace_val"][0, :u]); accs += list(r["trace_accept"][0, :u]); draws += list(r["draws"][0, :a])
        assert np.isnan(r["trace_val"][0, u:]).all() and (r["trace_accept"][0, u:] == -1).all()
        state, t0 = [(r["theta"][0], float(r["l"][0]), float(r["beta"][0]))], t0 + u
    assert t0 == T and same_bits(vals, tr["val"]) and accs == tr["accept"] and same_bits(np.array(draws), np.array(tr["draws"]))
    assert same_bits(state[0][0], tr["theta"]) and same_bits(state[0][1], tr["l"]) and same_bits(state[0][2], tr["beta_fin"])
    # nothing to do: the state comes back as it went in
    r = device_run(handle, [case], n_prop=[0], stop_acc=[3])
    assert r["used"][0] == 0 and r["accepted"][0] == 0 and same_bits(r["theta"][0], case["theta0"]) and r["l"][0] == tr["l0"]


def test_independent_of_the_handles_history(handle, trio):
    cases, walks = trio
    try:
        handle.debug_fill_scratch(0xFF)
        r = device_run(handle, cases)
        for j in range(3):
            check_against_walk(r, j, walks[j])
        D, y = load_gv(50, 1)[:2]
        handle.loglik_batch(D, y, 2, np.tile(np.concatenate([[0.5, 0.5], np.full(9, 1.0), np.full(9, 2.0)]), (70, 1)), 1.0)
        X = np.random.default_rng(0).random((200, 2))
        handle.loglik_batch(X, X.sum(axis=1), 2, np.array([[0.5, 0.5, 1.0, 1.0, 9.0, 9.0]]), 1.0)
        r = device_run(handle, cases[::-1])
        for j in range(3):
            check_against_walk(r, j, walks[2 - j])
    finally:
        handle.debug_fill_scratch(-1)


@pytest.mark.parametrize("poison", ["singular", "nan"])
def test_failed_proposals_are_rejected_and_counted(handle, trio, poison):
    cases, walks = trio
    case, tr0 = dict(cases[0]), walks[0]
    case["steps"] = case["steps"].copy()
    hit = [t for t in range(5, T) if not tr0["accept"][t]][:2]   # two proposals the clean chain rejects as well
    for t in hit:
        # the state before proposal t (both poisons are rejections, so the states are the clean chain's); psi1 = psi2 = -40
        # makes both components' matrices all ones
        theta = case["theta0"].copy()
        for s in range(t):
            if tr0["accept"][s]:
                theta = theta + case["steps"][s]
        case["steps"][t, :2] = math.nan if poison == "nan" else -40.0 - theta[:2]
    tr = twin_walk(handle, case)
    r = device_run(handle, [case])
    check_against_walk(r, 0, tr)
    for t in hit:
        assert math.isnan(r["trace_val"][0, t]) and math.isnan(r["trace_beta"][0, t]) and r["trace_accept"][0, t] == 0
        assert r["trace_status"][0, t] >= 1
    assert r["failed"] == len(hit) == int((r["trace_status"][0] != 0).sum())
    # the chain goes on: every other proposal has the clean chain's bits
    others = [t for t in range(T) if t not in hit]
    assert same_bits(r["trace_val"][0, others], np.array(tr0["val"])[others])
    assert np.array_equal(r["trace_accept"][0, others], np.array(tr0["accept"])[others])
    assert same_bits(r["theta"][0], tr0["theta"]) and same_bits(r["l"][0], tr0["l"])


def raw_call(h, n=17, d=3, C=1, prior=api.PRIOR_ISO, A=1, set_of=(0,), Tn=4, M=2, n_prop=(4,), stop_acc=(2,), drop=None,
             partial_trace=False):
    """ccgp_metro_segments_sets through ctypes with every output pre-filled with sentinels -> (rc, outputs untouched?)."""
    rng = np.random.default_rng(1)
    Xs, ys, s2 = rng.random((C, d, n)), rng.random((C, n)), np.ones(C)
    q = 4 if prior == api.PRIOR_ANI else 3
    nA = max(A, 1)
    arr = dict(set=np.array(list(set_of) + [0] * nA, dtype=np.int32)[:nA], theta0=np.zeros((nA, q), order="F"), l0=np.zeros(nA),
               steps=0.1 * rng.standard_normal((nA, Tn, q)), logu=np.log(rng.random((nA, Tn))),
               n_prop=np.array(list(n_prop) + [0] * nA, dtype=np.int32)[:nA],
               stop_acc=np.array(list(stop_acc) + [0] * nA, dtype=np.int32)[:nA])
    outs = dict(used=np.full(nA, -7, dtype=np.int32), acc=np.full(nA, -7, dtype=np.int32), draws=np.full(nA * M * q, -7.0),
                dval=np.full(nA * M, -7.0), dbeta=np.full(nA * M, -7.0), theta=np.full(nA * q, -7.0), l=np.full(nA, -7.0),
                beta=np.full(nA, -7.0), tv=np.full(nA * Tn, -7.0), tb=np.full(nA * Tn, -7.0),
                ts=np.full(nA * Tn, -7, dtype=np.int32), ta=np.full(nA * Tn, -7, dtype=np.int32))
    p, ip = api._p, api._ipt

    def g(name, ptr):
        return None if drop == name else ptr
    rc = api.lib().ccgp_metro_segments_sets(
        h._h, g("Xs", p(Xs)), n, d, p(ys), p(s2), C, prior, None, A, g("set", ip(arr["set"])), g("theta0", p(arr["theta0"])),
        p(arr["l0"]), None, Tn, g("steps", p(arr["steps"])), p(arr["logu"]), ip(arr["n_prop"]), ip(arr["stop_acc"]), M,
        g("used", ip(outs["used"])), ip(outs["acc"]), p(outs["draws"]), p(outs["dval"]), p(outs["dbeta"]), p(outs["theta"]),
        g("l", p(outs["l"])), p(outs["beta"]), p(outs["tv"]), p(outs["tb"]), ip(outs["ts"]),
        None if partial_trace else ip(outs["ta"]))
    return rc, all((v == -7).all() for v in outs.values())


def test_refusals_leave_the_outputs_untouched(handle):
    bad = [dict(n=0), dict(d=0), dict(d=65), dict(C=0), dict(prior=7), dict(prior=api.PRIOR_INVGAMMA), dict(prior=api.PRIOR_ANI),
           dict(A=-1), dict(set_of=(1,)), dict(set_of=(-1,)), dict(Tn=0), dict(M=0), dict(n_prop=(5,)), dict(n_prop=(-1,)),
           dict(stop_acc=(3,)), dict(stop_acc=(-1,)), dict(drop="Xs"), dict(drop="set"), dict(drop="theta0"), dict(drop="steps"),
           dict(drop="used"), dict(drop="l"), dict(partial_trace=True)]
    for kw in bad:
        rc, untouched = raw_call(handle, **kw)
        assert rc == -1 and untouched, kw
    rc, untouched = raw_call(handle, n=129)
    assert rc == -4 and untouched
    try:
        handle.set_kernel(api.KERNEL_MATERN, 2.5)
        rc, untouched = raw_call(handle, d=1)
        assert rc == -4 and untouched
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)
    rc, untouched = raw_call(handle, A=0)
    assert rc == 0 and untouched
    rc, untouched = raw_call(handle)
    assert rc >= 0 and not untouched


SHORT = dict(N=150, samp_size=100, batch_size=20)


def refused_shapes(handle):
    """The two kinds of shape the device chain refuses, each with a gp, a training set and a Laplace estimate: n = 129
    (Gaussian family, the blocked route) and the Matern family (1-D, the set-by-set route of the twin)."""
    rng = np.random.default_rng(3)
    D = rng.random((129, 4))
    big = (CombinedGP("ISO", handle=handle), D, np.sin(3.0 * D).sum(axis=1), np.array([2.0, 3.5, 0.3]))
    x = np.linspace(0.0, 1.0, 8)[:, None]
    from ccgp_amd.rsurface import CombinedGP1D
    matern = (CombinedGP1D(2.5, handle=handle), x, np.sin(5.0 * x[:, 0]) + 0.3 * x[:, 0], np.array([-1.0, 0.0, 0.3]))
    return dict(n129=big, matern=matern)


@pytest.mark.parametrize("shape", ["n129", "matern"])
def test_fallback_where_the_device_refuses(handle, shape):
    """Where ccgp_metro_segments_sets says CCGP_EUNSUPPORTED, Metro_device_sets carries the chain on the twin and returns the
    chain on_device=False gives; the twin itself serves the shape (the blocked route, the set-by-set route of the 1-D
    families) with ccgp_logpost_sets' likelihood."""
    gp, D, y, mode = refused_shapes(handle)[shape]
    rows = mode + 0.1 * np.random.default_rng(4).standard_normal((5, 3))
    Xs, Y = np.stack([D, D]), np.stack([y, y])
    set_of = [0, 1, 1, 0, 1]
    val, beta, ll, st = gp.h.chain_logpost_sets(Xs, Y, [1.0, 1.3], gp.cfg["prior"], rows, set_of)
    val0, beta0, ll0, st0 = gp.h.logpost_sets(Xs, Y, [1.0, 1.3], gp.cfg["prior"], rows, set_of)
    # the two differ in the exp and log of the terms alone, each within an ulp or two: 1e-11 of the value is far outside that
    assert not st.any() and not st0.any()
    assert np.allclose(val, val0, rtol=1e-11, atol=0) and np.allclose(beta, beta0, rtol=1e-9, atol=1e-12)
    with pytest.raises(api.CcgpError) as err:
        gp.h.metro_segments_sets(Xs, Y, [1.0, 1.3], gp.cfg["prior"], [0], rows[:1], [0.0], np.zeros((1, 4, 3)), np.zeros((1, 4)),
                                 [4], [4])
    assert err.value.code == -4
    est = dict(mode=mode, var=0.02 * np.eye(3), converged=True, value=0.0)
    kw = dict(N=12, samp_size=8, batch_size=4, alpha=2.0)
    a = fit.Metro_device_sets(gp, None, D_trains=[D], sigma2s=[1.0], ys=[y], rngs=[1], laplace=[est], max_proposals=60, **kw)
    b = fit.Metro_device_sets(gp, None, D_trains=[D], sigma2s=[1.0], ys=[y], rngs=[1], laplace=[est], max_proposals=60,
                              on_device=False, **kw)
    assert a["chains"][0]["accepted"] >= 8 and same_bits(a["chains"][0]["sample"], b["chains"][0]["sample"])
    assert same_bits(a["chains"][0]["beta"], b["chains"][0]["beta"])
    assert a["chains"][0]["proposals"] == b["chains"][0]["proposals"]


def test_driver_on_the_device_equals_driver_on_the_twin(handle):
    """The whole driver -- segments, Geweke checks, pending numbers -- on three GV sets: device chains against the twin's."""
    sets = [load_gv(50, i) for i in (1, 2, 3)]
    gp = CombinedGP("GV", handle=handle)
    s2 = [float(np.var(s[1], ddof=1)) for s in sets]
    est = [dict(mode=np.array([1.0, 1.0, 0.0]), var=0.05 * np.eye(3), converged=True, value=0.0) for _ in sets]
    args = dict(D_trains=[s[0] for s in sets], sigma2s=s2, ys=[s[1] for s in sets], laplace=est, alpha=0.5, block=64, **SHORT)
    a = fit.Metro_device_sets(gp, None, rngs=[1, 2, 3], seg=50, **args)
    b = fit.Metro_device_sets(gp, None, rngs=[1, 2, 3], seg=50, on_device=False, **args)
    assert a["device_batches"] < b["device_batches"]
    for ca, cb in zip(a["chains"], b["chains"]):
        assert same_bits(ca["sample"], cb["sample"]) and same_bits(ca["beta"], cb["beta"])
        assert ca["proposals"] == cb["proposals"] and ca["accepted"] == cb["accepted"] and ca["geweke_p"] == cb["geweke_p"]


def test_study_with_device_chains(handle):
    sets = [load_gv(50, i) for i in (1, 2, 3)]
    gp = CombinedGP("GV", handle=handle)
    s2 = [float(np.var(s[1], ddof=1)) for s in sets]
    r = fit.study(gp, sets, 0.05, SHORT["N"], SHORT["samp_size"], SHORT["batch_size"], 0.5, sigma2s=s2, rngs=[1, 2, 3],
                  device_chains=True)
    direct = fit.Metro_device_sets(gp, np.tile([1.0, 1.0, 0.0], (3, 1)), SHORT["N"], SHORT["samp_size"], SHORT["batch_size"], 0.5,
                                   [s[0] for s in sets], s2, [s[1] for s in sets], rngs=[1, 2, 3])
    for got, want in zip(r["chains"], direct["chains"]):
        assert same_bits(got["sample"], want["sample"]) and got["proposals"] == want["proposals"]
    assert len(r["tables"]) == 3 and all(np.isfinite(t["y_hat"]).all() for t in r["tables"])
    assert r["calls"]["metro"] < sum(c["proposals"] for c in r["chains"]) / 10


def test_posterior_mean_agrees_with_metro(handle):
    """GV train_50_1 at the reference's settings (N 5000, samp.size 1000, batch 20, alpha.geweke 0.5): the device chain and
    fit.Metro draw from one posterior -- each parameter's mean within 5 standard errors, the error from the spectral density
    at zero of both chains."""
    D, y = load_gv(50, 1)[:2]
    gp = CombinedGP("GV", handle=handle)
    s2 = float(np.var(y, ddof=1))
    a = fit.Metro(gp, np.array([1.0, 1.0, 0.0]), 5000, 1000, 20, 0.5, D, s2, y, rng=1)
    b = fit.Metro_device(gp, np.array([1.0, 1.0, 0.0]), 5000, 1000, 20, 0.5, D, s2, y, rng=2)
    for j in range(3):
        xa, xb = a["sample"][:, j], b["sample"][:, j]
        se = math.sqrt(fit._spectrum0_ar(xa) / xa.size + fit._spectrum0_ar(xb) / xb.size)
        print("parameter %d: means %.4f %.4f, se %.4f" % (j, xa.mean(), xb.mean(), se))
        assert abs(xa.mean() - xb.mean()) <= 5.0 * se
