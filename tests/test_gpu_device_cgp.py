"""The CGP refinement on the device (ccgp_cgp_fit_sets, cgp.refine_starts_device, cgp.CGP / CGP_sets(on_device=True),
fit.study(device_cgp=True)) against its host twin (ccgp_cgp_fit_eval_sets driven one evaluation at a time through
ccgp_fit_feed): the final state and the whole trace bit for bit at (n, d) = (5, 1), (14, 2), (50, 9), (64, 4), (65, 3) and
(128, 2) -- both sides of the evaluator's lane-ownership split at 64 and its largest carve -- run at once, cut into calls of 7
and of 1 evaluations, and with look = 1 against 16; a start's independence of the other starts, of the order of the sets and of
what the handle's buffers held; a start whose first point fails and one whose clipped lower point fails; refusals; and the
Python layers, whose fits must be the default's in every field but calls, refinement_calls and seconds.

Every evaluation of the twin is ccgp_cgp_state_batch_sets on the rows csrc/cgp_fit_logic.h forms, so "device == twin" holds
the gated evaluator inside the loop to that call's bits as well as the step kernel to ccgp_fit_feed's."""
import os

import numpy as np
import pytest

from ccgp_amd import api, cgp
from conftest import load_gv, synthetic_design

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1), (14, 2), (50, 9), (64, 4), (65, 3), (128, 2)]
C, S = 2, 3
STEP = 1e-5
CAP = 4096
HDR = api.FIT_HEADER
BACKTRACKS, PAIRS = 4, 7   # words of a start's state (csrc/fit_logic.h)
# (maxit, max_backtracks) of the six starts of a shape: a cap on the iterations keeps the n = 128 case short; a line search
# given up early, with pairs in the memory, is what empties a quasi-Newton memory; maxit = 2 stops a start with code 3
OPTS = [(8, 30), (8, 1), (2, 30), (8, 30), (8, 0), (8, 2)]
SKIP = ("calls", "refinement_calls", "seconds")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def problem(handle, n, d):
    """C seeded sets of one shape and, per set, the S best of 24 points of a seeded hypercube over the set's box, in the
    hypercube's order: how CGP takes its starts (GV:144-151)."""
    rng = np.random.default_rng(1000 * n + d)
    Xs, ys, box = [], [], []
    for c in range(C):
        X, y = synthetic_design(n, d, 7 * n + d + 31 * c)
        Xs.append(cgp.standardise(X)[0])
        ys.append(y * (1.0 + 0.2 * c) + 0.05 * rng.standard_normal(n))
        box.append(cgp.bounds(Xs[-1]))
    Xs, ys = np.stack(Xs), np.stack(ys)
    cand = [box[c][0] + cgp.lhd(24, d + 3, rng) * (box[c][1] - box[c][0]) for c in range(C)]
    val, _, _, _, st = handle.cgp_state_batch_sets(Xs, ys, cgp.rows_from_ww(np.concatenate(cand)), np.repeat(np.arange(C), 24))
    val = np.where(np.isfinite(val), val, cgp.NONFINITE)
    starts = np.concatenate([cand[c][np.sort(np.argsort(val[24 * c:24 * (c + 1)], kind="stable")[:S])] for c in range(C)])
    owner = np.repeat(np.arange(C), S)
    lowers, uppers = np.stack([box[c][0] for c in owner]), np.stack([box[c][1] for c in owner])
    state = np.stack([api.fit_begin(starts[a], lowers[a], uppers[a], maxit=OPTS[a][0], max_backtracks=OPTS[a][1])
                      for a in range(C * S)])
    return dict(n=n, d=d, Xs=Xs, ys=ys, starts=starts, owner=owner, lowers=lowers, uppers=uppers, state=state)


def new_counters():
    return dict(accepted=0, backtracks=0, resets=0, clipped=0)


def twin(h, pr, state, owner=None, Xs=None, ys=None, step=STEP, max_evals=CAP):
    """The contract's sequential form, all starts side by side: (state, trace_f, trace_status per start, what occurred)."""
    state = np.array(state)
    owner = pr["owner"] if owner is None else owner
    Xs, ys = (pr["Xs"], pr["ys"]) if Xs is None else (Xs, ys)
    A, P = state.shape[0], pr["d"] + 3
    tr_f, tr_s = [[] for _ in range(A)], [[] for _ in range(A)]
    cnt = new_counters()
    for _ in range(max_evals):
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        w = api.fit_trial(state[live])
        lo, hi = state[live, HDR + 4 * P:HDR + 5 * P], state[live, HDR + 5 * P:HDR + 6 * P]
        f, g, st = h.cgp_fit_eval_sets(Xs, ys, w, lo, hi, step, owner[live])
        cnt["clipped"] += int(((w - step < lo) | (w + step > hi)).sum())
        for k, a in enumerate(live):
            pairs, its = state[a, PAIRS], state[a, api.FIT_ITERATIONS]
            api.fit_feed(state[a], f[k], np.asarray(g[k]).ravel(), st[k] == 0)
            running = state[a, api.FIT_CODE] == api.FIT_RUNNING
            cnt["accepted"] += int(state[a, api.FIT_ITERATIONS] > its)
            cnt["backtracks"] += int(running and state[a, BACKTRACKS] > 0)
            cnt["resets"] += int(pairs > 0 and state[a, PAIRS] == 0)
            tr_f[a].append(f[k])
            tr_s[a].append(int(st[k]))
    return state, tr_f, tr_s, cnt


def launch(h, pr, state, max_evals, owner=None, look=16, **kw):
    return h.cgp_fit_sets(pr["Xs"], pr["ys"], pr["owner"] if owner is None else owner, state, STEP, max_evals, look, trace=True,
                          **kw)


def check(r, j, want_state, tr_f, tr_s, t0=0, used=None):
    used = len(tr_f) - t0 if used is None else used
    assert r["evals"][j] == used
    assert same_bits(r["trace_f"][j, :used], tr_f[t0:t0 + used])
    assert np.array_equal(r["trace_status"][j, :used], tr_s[t0:t0 + used])
    assert np.isnan(r["trace_f"][j, used:]).all() and (r["trace_status"][j, used:] == -1).all()
    if want_state is not None:
        assert same_bits(r["state"][j], want_state)


@pytest.fixture(scope="module")
def reference_runs(handle):
    """The twin's runs, computed once per shape on demand and never changed."""
    cache = {}

    def get(shape):
        if shape not in cache:
            pr = problem(handle, *shape)
            cache[shape] = (pr,) + twin(handle, pr, pr["state"])
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-d%d" % s)
def test_device_refinement_is_the_twin(handle, reference_runs, shape):
    pr, want, tr_f, tr_s, cnt = reference_runs(shape)
    s0, A = pr["state"], C * S
    longest = max(len(t) for t in tr_f)
    print("shape %s: evaluations %s, iterations %s, codes %s, %s" % (
        shape, [len(t) for t in tr_f], want[:, api.FIT_ITERATIONS].astype(int).tolist(),
        want[:, api.FIT_CODE].astype(int).tolist(), cnt))
    assert longest < CAP and (want[:, api.FIT_CODE] != api.FIT_RUNNING).all()
    assert (want[:, api.FIT_CODE] != api.FIT_NOT_EVALUABLE).all()
    # evaluation 0 is ccgp_cgp_state_batch_sets on the rows of cgp._fit_sets.evaluate, directly
    P = shape[1] + 3
    up, dn = np.minimum(pr["starts"] + STEP, pr["uppers"]), np.maximum(pr["starts"] - STEP, pr["lowers"])
    pts = np.repeat(pr["starts"][:, None, :], 1 + 2 * P, axis=1)
    for j in range(P):
        pts[:, 1 + 2 * j, j], pts[:, 2 + 2 * j, j] = up[:, j], dn[:, j]
    val, _, _, _, st = handle.cgp_state_batch_sets(pr["Xs"], pr["ys"], cgp.rows_from_ww(pts.reshape(-1, P)),
                                                   np.repeat(pr["owner"], 1 + 2 * P))
    F = np.where(np.isfinite(val), val, cgp.NONFINITE).reshape(A, -1)
    f0, g0, st0 = handle.cgp_fit_eval_sets(pr["Xs"], pr["ys"], pr["starts"], pr["lowers"], pr["uppers"], STEP, pr["owner"])
    assert same_bits(f0, F[:, 0]) and same_bits(g0, (F[:, 1::2] - F[:, 2::2]) / (up - dn))
    assert np.array_equal(st0, st.reshape(A, -1)[:, 0]) and same_bits([t[0] for t in tr_f], f0)
    # all at once, looking every 16 rounds and every round
    for look in (16, 1):
        r = launch(handle, pr, s0, CAP, look=look, T=CAP)
        assert r["failed"] == sum(int(s != 0) for t in tr_s for s in t)
        for j in range(A):
            check(r, j, want[j], tr_f[j], tr_s[j])
    # cut by max_evals = 7, then 1, per call, the state of one call the start of the next
    for cut in (7, 1):
        state, t0 = s0, np.zeros(A, dtype=int)
        while (state[:, api.FIT_CODE] == api.FIT_RUNNING).any():
            r = launch(handle, pr, state, cut)
            for j in range(A):
                check(r, j, None, tr_f[j], tr_s[j], t0[j], min(cut, len(tr_f[j]) - t0[j]))
            state, t0 = r["state"], t0 + r["evals"]
        assert same_bits(state, want)
    # max_evals = 0: the state as it came, nothing evaluated; a stopped start is returned as it came
    r = launch(handle, pr, s0, 0, T=4)
    assert same_bits(r["state"], s0) and not r["evals"].any() and np.isnan(r["trace_f"]).all()
    r = launch(handle, pr, want, 5)
    assert same_bits(r["state"], want) and not r["evals"].any()


def test_every_branch_of_the_step_occurred(reference_runs):
    """Over the module's shapes: accepted steps, backtracks, a memory reset, clipped differences, two stop codes at least."""
    total, codes = new_counters(), set()
    for shape in SHAPES:
        _, want, _, _, cnt = reference_runs(shape)
        codes |= set(want[:, api.FIT_CODE].astype(int).tolist())
        for k, v in cnt.items():
            total[k] += v
    print(total, "stop codes", sorted(codes))
    assert total["accepted"] > 0 and total["backtracks"] > 0 and total["resets"] > 0, total
    assert len(codes) >= 2 and api.FIT_RUNNING not in codes


def test_a_start_depends_on_its_own_inputs_only(handle, reference_runs):
    pr, want, tr_f, tr_s, _ = reference_runs((14, 2))
    s0, j = pr["state"], 4
    r = launch(handle, pr, s0[j:j + 1], CAP, owner=pr["owner"][j:j + 1])   # alone
    check(r, 0, want[j], tr_f[j], tr_s[j])
    r = launch(handle, pr, np.concatenate([s0[:3], s0, s0[j:j + 1]]), CAP,
               owner=np.concatenate([pr["owner"][:3], pr["owner"], pr["owner"][j:j + 1]]))   # last of ten
    check(r, 9, want[j], tr_f[j], tr_s[j])
    # the sets in the other order
    r = handle.cgp_fit_sets(pr["Xs"][::-1], pr["ys"][::-1], 1 - pr["owner"], s0, STEP, CAP, 16, trace=True)
    for k in range(C * S):
        check(r, k, want[k], tr_f[k], tr_s[k])
    try:
        handle.debug_fill_scratch(0xFF)   # whatever the handle's buffers held
        r = launch(handle, pr, s0, CAP)
        for k in range(C * S):
            check(r, k, want[k], tr_f[k], tr_s[k])
    finally:
        handle.debug_fill_scratch(-1)


def test_failed_rows(handle):
    """nugget_l = 0 opens lambda = 0, where Q is the Gaussian matrix G alone.  Two sets of one shape:
      set 0 has a duplicated row.  Its start at lambda = 0 ends with code 5.  (So would any start on it: with rows i = j the
        reweighting gives s_i = s_j, and the 2 x 2 block of Q on them has determinant lambda (sqrt s_i - sqrt s_j)^2 = 0 at every
        lambda.  A start that goes on after a failed LOWER point therefore cannot live on a duplicated row; it lives on set 1.)
      set 1 has distinct rows under a theta box of 1e-9 .. 1e-7, where G is numerically of rank 4 and any lambda > 0 restores
        the pivots.  Its start at lambda = 0 ends with code 5 as well; its start at lambda = step / 2 has its lower point clipped
        to 0, which fails: it differences with the 1e6, goes on, and is the twin; a third start is the neighbour, which is what
        it is alone."""
    n, d = 14, 2
    P = d + 3
    X, y = synthetic_design(n, d, 5)
    Xd = X.copy()
    Xd[4] = Xd[3]
    Xs = np.stack([cgp.standardise(Xd)[0], cgp.standardise(X)[0]])
    ys = np.stack([y, y])
    box = [cgp.bounds(cgp.standardise(X)[0], nugget_l=0.0), cgp.bounds(Xs[1], nugget_l=0.0, theta_l=1e-9, alpha_l=1e-7)]
    rng = np.random.default_rng(8)
    owner = np.array([0, 1, 1, 1])
    lowers, uppers = np.stack([box[c][0] for c in owner]), np.stack([box[c][1] for c in owner])
    starts = lowers + cgp.lhd(4, P, rng) * (uppers - lowers)
    starts[0, 0] = starts[1, 0] = 0.0
    starts[2, 0] = STEP / 2
    pr = dict(n=n, d=d, Xs=Xs, ys=ys, owner=owner)
    state = np.stack([api.fit_begin(starts[a], lowers[a], uppers[a], maxit=6) for a in range(4)])
    want, tr_f, tr_s, _ = twin(handle, pr, state)
    r = launch(handle, pr, state, CAP)
    for k in range(4):
        check(r, k, want[k], tr_f[k], tr_s[k])
    print("codes %s, evaluations %s, failed %d" % (r["state"][:, api.FIT_CODE].astype(int).tolist(), r["evals"].tolist(), r["failed"]))
    for a in (0, 1):
        assert r["state"][a, api.FIT_CODE] == api.FIT_NOT_EVALUABLE and r["evals"][a] == 1 and np.isinf(r["state"][a, api.FIT_F])
        assert r["trace_f"][a, 0] == cgp.NONFINITE and r["trace_status"][a, 0] > 0
    assert r["failed"] == sum(int(s != 0) for t in tr_s for s in t) >= 2
    # the clipped lower point of start 2 fails on its own; the start differences with the 1e6 and goes on
    row = cgp.rows_from_ww(np.concatenate([[0.0], starts[2, 1:]])[None])
    val, _, _, _, st = handle.cgp_state_batch_sets(Xs, ys, row, [1])
    assert st[0] > 0 and np.isnan(val[0])
    assert r["trace_status"][2, 0] == 0 and np.isfinite(r["trace_f"][2, 0]) and r["trace_f"][2, 0] != cgp.NONFINITE
    assert r["evals"][2] > 1 and r["state"][2, api.FIT_CODE] != api.FIT_NOT_EVALUABLE
    g2 = handle.cgp_fit_eval_sets(Xs, ys, starts[2:3], lowers[2:3], uppers[2:3], STEP, [1])[1]
    up = starts[2, 0] + STEP
    val_up, _, _, _, st_up = handle.cgp_state_batch_sets(Xs, ys, cgp.rows_from_ww(np.concatenate([[up], starts[2, 1:]])[None]), [1])
    assert st_up[0] == 0 and g2[0, 0] == (val_up[0] - cgp.NONFINITE) / (up - 0.0) < -1e9
    # the neighbour is what it is alone
    assert r["state"][3, api.FIT_CODE] != api.FIT_NOT_EVALUABLE and r["evals"][3] > 1
    alone = launch(handle, pr, state[3:4], CAP, owner=owner[3:4])
    assert same_bits(alone["state"][0], r["state"][3])


def test_refusals_leave_the_handle_as_it_was(handle, reference_runs):
    pr = reference_runs((14, 2))[0]
    n, d = 14, 2
    s0 = pr["state"][:2]
    launch(handle, pr, s0, 2, owner=pr["owner"][:2])
    handle.cgp_fit_eval_sets(pr["Xs"], pr["ys"], pr["starts"][:2], pr["lowers"][:2], pr["uppers"][:2], STEP, pr["owner"][:2])
    before = handle.workspace_bytes()
    L = api.lib()
    Xb = np.ascontiguousarray(np.transpose(pr["Xs"], (0, 2, 1)))
    yb = np.ascontiguousarray(pr["ys"])

    def call(A=2, state=None, max_evals=(2, 2), T=4, tr_f=True, tr_s=True, n=n, d=d, C=C, set_of=(0, 1), step=STEP, look=16, X=True,
             yy=True, se=True, ev=True, me=True, st=True, hh=None):
        state = np.array(s0) if state is None else state
        mx = np.array(max_evals, dtype=np.int32)
        idx = np.array(set_of, dtype=np.int32)
        nA = max(state.shape[0], 2)
        evals = np.full(nA, -7, dtype=np.int32)
        f, s = np.full((nA, max(T, 1)), 5.0), np.full((nA, max(T, 1)), 9, dtype=np.int32)
        keep = state.copy()
        rc = L.ccgp_cgp_fit_sets((hh or handle)._h, api._p(Xb) if X else None, n, d, api._p(yb) if yy else None, C, A,
                                 api._ipt(idx) if se else None, api._p(state) if st else None, step,
                                 api._ipt(mx) if me else None, look, api._ipt(evals) if ev else None,
                                 api._p(f) if tr_f else None, api._ipt(s) if tr_s else None, T)
        assert same_bits(state, keep) and (evals == -7).all() and (f == 5.0).all() and (s == 9).all()
        return rc
    wrong_d = np.array(s0)
    wrong_d[1, 0] = 13
    for kw in (dict(A=-1), dict(T=-1), dict(C=0), dict(look=0), dict(look=65), dict(step=0.0), dict(step=-1e-5),
               dict(step=float("nan")), dict(step=float("inf")), dict(set_of=(0, 2)), dict(set_of=(-1, 0)),
               dict(max_evals=(2, 5)), dict(max_evals=(-1, 2)), dict(max_evals=(2, 4097), T=5000), dict(tr_s=False),
               dict(tr_f=False), dict(X=False), dict(yy=False), dict(se=False), dict(ev=False), dict(me=False), dict(st=False),
               dict(state=wrong_d), dict(d=0), dict(n=0)):
        assert call(**kw) == -1, kw
    assert call(A=0) == 0
    # unsupported: n = 129 (as ccgp_cgp_state_batch_sets), 65 variables, A R > 65535
    assert call(n=129) == -4
    assert call(d=62, state=np.zeros((2, HDR + 16 * 65))) == -4
    many = 65535 // api.cgp_fit_rows(d) + 1
    assert call(A=many, state=np.tile(s0[:1], (many, 1)), max_evals=np.full(many, 2), set_of=np.zeros(many)) == -4
    # the twin's evaluator: its own refusals, outputs untouched
    w = np.asfortranarray(pr["starts"][:2])
    lo, hi = np.asfortranarray(pr["lowers"][:2]), np.asfortranarray(pr["uppers"][:2])

    def call_eval(B=2, n=n, d=d, C=C, set_of=(0, 1), step=STEP, X=True, wp=True, lp=True, hp=True, of=True, og=True, se=True):
        f, g, st = np.full(2, 5.0), np.full((2, d + 3), 5.0), np.full(2, 9, dtype=np.int32)
        idx = np.array(set_of, dtype=np.int32)
        rc = L.ccgp_cgp_fit_eval_sets(handle._h, api._p(Xb) if X else None, n, d, api._p(yb), C, api._p(w) if wp else None,
                                      api._p(lo) if lp else None, api._p(hi) if hp else None, step,
                                      api._ipt(idx) if se else None, B, api._p(f) if of else None, api._p(g) if og else None,
                                      api._ipt(st))
        assert (f == 5.0).all() and (g == 5.0).all() and (st == 9).all()
        return rc
    for kw in (dict(B=-1), dict(C=0), dict(set_of=(0, 2)), dict(step=0.0), dict(step=float("nan")), dict(X=False), dict(wp=False),
               dict(lp=False), dict(hp=False), dict(of=False), dict(og=False), dict(se=False), dict(n=0), dict(d=0)):
        assert call_eval(**kw) == -1, kw
    assert call_eval(B=0) == 0
    assert call_eval(n=129) == -4
    assert handle.workspace_bytes() == before
    # a workspace limit the rows do not fit under: the device call refuses, the twin chunks, the driver goes there by itself
    h2 = api.Handle(0)
    try:
        h2.set_workspace_limit(1 << 20)   # the smallest limit a handle takes: 720 starts need 1.2 MB (states 0.55, rows 0.38)
        rep = 120
        starts, owner = np.tile(pr["starts"], (rep, 1)), np.tile(pr["owner"], rep)
        lowers, uppers = np.tile(pr["lowers"], (rep, 1)), np.tile(pr["uppers"], (rep, 1))
        before2 = h2.workspace_bytes()
        assert call(hh=h2, A=6 * rep, state=np.tile(pr["state"], (rep, 1)), max_evals=np.full(6 * rep, 2), set_of=owner) == -4
        assert h2.workspace_bytes() == before2
        a = cgp.refine_starts_device(h2, pr["Xs"], pr["ys"], starts, lowers, uppers, owner, STEP, maxit=3)
        b = cgp.refine_starts_device(handle, pr["Xs"], pr["ys"], starts, lowers, uppers, owner, STEP, maxit=3)
        assert same_bits(a["x"], b["x"]) and same_bits(a["f"], b["f"]) and np.isfinite(a["f"]).all()
        assert np.array_equal(a["calls_per_start"], b["calls_per_start"]) and b["calls"] == 1 < a["calls"]
    finally:
        h2.close()


def _same_fit(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in SKIP:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def test_cgp_on_the_device_is_cgp(handle):
    X, y = load_gv(50, 1)[:2]
    base = cgp.CGP(handle, X, y)
    dev = cgp.CGP(handle, X, y, on_device=True)
    _same_fit(dev, base)
    print("CGP train_50_1: refinement calls %d (lockstep: %d), calls %d (%d), refinement %.4f s (%.4f s)" % (
        dev["refinement_calls"], base["refinement_calls"], dev["calls"], base["calls"], dev["seconds"]["refinement"],
        base["seconds"]["refinement"]))
    assert dev["refinement_calls"] < base["refinement_calls"] and dev["calls"] < base["calls"]
    _same_fit(cgp.CGP(handle, X, y, on_device=True, look=1), base)


def test_cgp_sets_on_the_device_are_the_per_set_fits(handle):
    sets = [load_gv(50, i)[:2] for i in (1, 2, 3)]
    alone = [cgp.CGP(handle, X, y) for X, y in sets]
    got = cgp.CGP_sets(handle, [s[0] for s in sets], [s[1] for s in sets], on_device=True)
    for c in range(3):
        _same_fit(got[c], alone[c])
    assert got[0]["refinement_calls"] < max(a["refinement_calls"] for a in alone)


def test_study_writes_the_same_tables(handle, tmp_path):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP

    def twelve(c):
        X, y = synthetic_design(12, 2, 40 + c)
        Xt, yt = synthetic_design(6, 2, 70 + c)
        return X, y * (1.0 + 0.2 * c) + 0.3 * c * X[:, 0], Xt, yt * (1.0 + 0.2 * c) + 0.3 * c * Xt[:, 0]
    gp = CombinedGP("GV", handle=handle)
    sets = [twelve(c) for c in range(3)]
    arms = {on: fit.study(gp, sets, 0.05, 300, 60, 20, 0.5, net_samp_size=40, rngs=[1, 2, 3], cgp=True, device_cgp=on,
                          out_dir=str(tmp_path / ("dev" if on else "host"))) for on in (False, True)}
    off, on = arms[False], arms[True]
    for i in range(3):
        name = "results_%d.txt" % (i + 1)
        with open(os.path.join(str(tmp_path / "host"), name), "rb") as a, open(os.path.join(str(tmp_path / "dev"), name), "rb") as b:
            assert a.read() == b.read(), name
        _same_fit(on["tables"][i]["CGP"], off["tables"][i]["CGP"])
        assert on["summaries"][i] == off["summaries"][i]
    assert on["pooled"] == off["pooled"]
    print("cgp device calls: %d (lockstep: %d)" % (on["calls"]["cgp"], off["calls"]["cgp"]))
    assert 0 < on["calls"]["cgp"] < off["calls"]["cgp"]
    # compare_GP passes the option on as well
    D_train, y_train, D_test, y_test = sets[0]
    t_off = fit.compare_GP(gp, D_test, 0.05, y_test, off["draws"][0], D_train, off["sigma2"][0], y_train, exact=True, cgp=True)
    t_on = fit.compare_GP(gp, D_test, 0.05, y_test, off["draws"][0], D_train, off["sigma2"][0], y_train, exact=True, cgp=True,
                          device_cgp=True)
    _same_fit(t_on["CGP"], t_off["CGP"])
    assert t_on["CGP"]["refinement_calls"] < t_off["CGP"]["refinement_calls"]
    np.testing.assert_array_equal(t_on["y_hat_CGP"], t_off["y_hat_CGP"])
