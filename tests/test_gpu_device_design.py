"""The maximum-entropy design search on the device (ccgp_design_fit, design.minimize_starts_device, Entropy_optim(on_device=True))
against its host twin (ccgp_design_fit_eval driven one evaluation at a time through ccgp_fit_feed): the final state and the whole
trace bit for bit, one shape per DFIT instance NB = 1 .. 8 (two for NB = 2: d = 9 crosses the epilogue's 8-dimension chunk); a
start's independence of the other starts, of its position, of how its evaluations are cut into calls and of what the handle ran
before; a start on a coincident pair; refusals; and the two batch-sequential searches through rsurface.

Every evaluation of the twin is ccgp_mixed_logdet_grad_designs on the design (D.old on top of the trial's rows), so "device ==
twin" holds the kernel's evaluation inside the loop to that call's bits as well as the stepper to ccgp_fit_feed's."""
import numpy as np
import pytest

from ccgp_amd import api, design
from ccgp_amd.rsurface import CombinedGP
from design_ref import BSQ_PRIOR, design_distance, initial_me_design, params_row

pytestmark = pytest.mark.gpu

# (n, d, n_fixed): NB = 1 the first batch of the batch-sequential script, NB = 2 its second batch and nv = 63 with d = 9,
# NB = 3, 4 (nv = 63), 5 (nv = 64, the ceiling, d = 1), 6, 7, 8 (nv = 64)
SHAPES = [(14, 2, 0), (21, 2, 14), (17, 9, 10), (33, 3, 16), (50, 9, 43), (65, 1, 1), (81, 2, 60), (97, 5, 90), (128, 4, 112)]
CAP = 4096
MAXIT = 12
HDR = api.FIT_HEADER
BACKTRACKS, PAIRS = 4, 7   # words of a start's state (csrc/fit_logic.h)
# max_backtracks of the four starts where it is not 30: a line search given up early, with pairs in the memory, is what empties
# a quasi-Newton memory (the start forgets its model and tries steepest descent once more)
BT = {(14, 2, 0): [30, 30, 30, 1], (33, 3, 16): [30, 1, 30, 30], (97, 5, 90): [0, 0, 0, 30], (128, 4, 112): [0, 30, 30, 0]}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def problem(n, d, nf):
    """Four starts of one shape: the shared parameter row (p = 0.5, theta2 = 4 theta1, as the script's prior medians), the
    fixed rows, the starts and their boxes, the states.  The two script shapes are the script's problems; the others spread a
    Latin hypercube of n points over the box (its first n_fixed rows are D.old, the starts jitter the others by a fraction of
    the spacing h = 2 n^(-1/d)) with theta1 = 1 / h^2, so that neighbours correlate at about exp(-1) and every start can be
    factorised.  (65, 1, 1): start 3 is built to fail inside its run (see below)."""
    nfree = n - nf
    lo, hi = np.full((4, nfree, d), -1.0), np.full((4, nfree, d), 1.0)
    if (n, d, nf) == (14, 2, 0):
        theta, D_old, starts = BSQ_PRIOR[1:], None, design.make_starts(4, 14, 2, 0)
    elif (n, d, nf) == (21, 2, 14):
        theta, D_old, starts = BSQ_PRIOR[1:], initial_me_design(), design.make_starts(4, 7, 2, 0)
    else:
        rng = np.random.default_rng(1000 * n + 10 * d + nf)
        h = 2.0 * n ** (-1.0 / d)
        theta = (1.0 / h ** 2, 4.0 / h ** 2)
        pts = design.make_starts(1, n, d, rng)[0]
        if d == 1:
            # the ceiling shape on a line: a jittered grid in a random row order, so that the construction below knows its
            # neighbours
            grid = -1.0 + (np.arange(n) + 0.5) * h
            pts = (grid + 0.1 * h * rng.uniform(-1.0, 1.0, n))[rng.permutation(n)][:, None]
        D_old = pts[:nf] if nf else None
        starts = np.stack([np.clip(pts[nf:] + (0.25 * h * rng.uniform(-1.0, 1.0, (nfree, d)) if s else 0.0), -1.0, 1.0)
                           for s in range(4)])
        if d == 1:
            # A failed trial inside a running start: two neighbours on the line, a and b, each with its OTHER neighbour moved
            # to 0.15 h from it, so that the gradient pushes a and b towards each other; their boxes end at the midpoint c.
            # The first steepest-descent trial (a step of unit length, most of it on these four rows) clips both to c: two
            # coincident rows, a zero pivot, an infeasible trial, and the line search halves its way back.
            x = starts[3, :, 0]
            order = np.argsort(x)
            m = nfree // 2
            left, a, b, right = order[m - 1], order[m], order[m + 1], order[m + 2]
            c = 0.5 * (x[a] + x[b])
            x[left], x[right] = x[a] - 0.15 * h, x[b] + 0.15 * h
            hi[3, a, 0], lo[3, b, 0] = c, c
    row = params_row(0.5, theta[0], theta[1], d)
    bt = BT.get((n, d, nf), [30] * 4)
    state = np.stack([api.fit_begin(starts[s].ravel(), lo[s].ravel(), hi[s].ravel(), maxit=MAXIT, max_backtracks=bt[s])
                      for s in range(4)])
    return dict(n=n, d=d, nf=nf, nfree=nfree, theta=theta, row=row, D_old=D_old, starts=starts, state=state, ld_offset=0.0)


def new_counters():
    return dict(backtracks=0, frozen=0, resets=0, failed_inside=0)


def twin(h, pr, state, max_evals=CAP):
    """The contract's sequential form, all starts side by side: (state, trace_f, trace_status per start, what occurred)."""
    state = np.array(state)
    A, nfree, d = state.shape[0], pr["nfree"], pr["d"]
    nv = nfree * d
    tr_f, tr_s = [[] for _ in range(A)], [[] for _ in range(A)]
    cnt = new_counters()
    for _ in range(max_evals):
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        f, g, st = h.design_fit_eval(api.fit_trial(state[live]).reshape(-1, nfree, d), 2, pr["row"], pr["D_old"], pr["ld_offset"])
        for k, a in enumerate(live):
            pairs = state[a, PAIRS]
            api.fit_feed(state[a], f[k], np.asarray(g[k]).ravel(), st[k] == 0)
            running = state[a, api.FIT_CODE] == api.FIT_RUNNING
            s = state[a]
            x, gr, lo, hi = s[HDR:HDR + nv], s[HDR + nv:HDR + 2 * nv], s[HDR + 4 * nv:HDR + 5 * nv], s[HDR + 5 * nv:HDR + 6 * nv]
            cnt["backtracks"] += int(running and s[BACKTRACKS] > 0)
            cnt["frozen"] += int(running and bool((((x <= lo) & (gr > 0.0)) | ((x >= hi) & (gr < 0.0))).any()))
            cnt["resets"] += int(pairs > 0 and s[PAIRS] == 0)
            cnt["failed_inside"] += int(running and st[k] != 0 and len(tr_f[a]) > 0)
            tr_f[a].append(f[k])
            tr_s[a].append(int(st[k]))
    return state, tr_f, tr_s, cnt


def launch(h, pr, state, max_evals, **kw):
    return h.design_fit(pr["nfree"], pr["d"], 2, pr["row"], state, max_evals, pr["D_old"], pr["ld_offset"], trace=True, **kw)


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
            pr = problem(*shape)
            if pr["nf"]:
                ld_old, st_old = handle.mixed_logdet_designs(pr["D_old"][None], 2, pr["row"])
                assert st_old[0] == 0
                pr["ld_offset"] = float(ld_old[0])
            cache[shape] = (pr,) + twin(handle, pr, pr["state"])
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-d%d-fixed%d" % s)
def test_device_search_is_the_twin(handle, reference_runs, shape):
    pr, want, tr_f, tr_s, cnt = reference_runs(shape)
    s0, nf, nfree, d = pr["state"], pr["nf"], pr["nfree"], pr["d"]
    longest = max(len(t) for t in tr_f)
    print("shape %s: evaluations %s, iterations %s, codes %s, %s" % (
        shape, [len(t) for t in tr_f], want[:, api.FIT_ITERATIONS].astype(int).tolist(),
        want[:, api.FIT_CODE].astype(int).tolist(), cnt))
    assert longest < CAP and (want[:, api.FIT_CODE] != api.FIT_RUNNING).all()
    # every start evaluates and makes at least 3 accepted iterations
    assert (want[:, api.FIT_CODE] != api.FIT_NOT_EVALUABLE).all() and (want[:, api.FIT_ITERATIONS] >= 3).all()
    # evaluation 0 is ccgp_mixed_logdet_grad_designs on that design, directly
    full = pr["starts"] if not nf else np.concatenate([np.broadcast_to(pr["D_old"], (4, nf, d)), pr["starts"]], axis=1)
    ld, g, st = handle.mixed_logdet_grad_designs(full, 2, pr["row"], nf)
    f0, g0, st0 = handle.design_fit_eval(pr["starts"], 2, pr["row"], pr["D_old"], pr["ld_offset"])
    assert not st.any() and not st0.any() and same_bits(f0, -(ld - pr["ld_offset"])) and same_bits(g0, -g)
    assert same_bits([t[0] for t in tr_f], f0)
    # all at once
    r = launch(handle, pr, s0, CAP, T=CAP)
    assert r["failed"] == sum(int(s != 0) for t in tr_s for s in t)
    for j in range(4):
        check(r, j, want[j], tr_f[j], tr_s[j])
    # cut by max_evals = 7, then 1, per call, the state of one call the start of the next
    for cut in (7, 1):
        state, t0 = s0, np.zeros(4, dtype=int)
        while (state[:, api.FIT_CODE] == api.FIT_RUNNING).any():
            r = launch(handle, pr, state, cut)
            for j in range(4):
                check(r, j, None, tr_f[j], tr_s[j], t0[j], min(cut, len(tr_f[j]) - t0[j]))
            state, t0 = r["state"], t0 + r["evals"]
        assert same_bits(state, want)
    # max_evals = 0: the state as it came, nothing evaluated; a stopped start is returned as it came
    r = launch(handle, pr, s0, 0, T=4)
    assert same_bits(r["state"], s0) and not r["evals"].any() and np.isnan(r["trace_f"]).all()
    r = launch(handle, pr, want, 5)
    assert same_bits(r["state"], want) and not r["evals"].any()


def test_every_branch_of_the_step_occurred(reference_runs):
    """Over the module's shapes: backtracks, a variable frozen at a bound, a memory reset, a failed trial inside a running start."""
    total = new_counters()
    for shape in SHAPES:
        for k, v in reference_runs(shape)[4].items():
            total[k] += v
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_a_start_depends_on_its_own_state_only(handle, reference_runs):
    shape = (21, 2, 14)
    pr, want, tr_f, tr_s, _ = reference_runs(shape)
    s0, j = pr["state"], 2
    r = launch(handle, pr, s0[j:j + 1], CAP)   # alone
    check(r, 0, want[j], tr_f[j], tr_s[j])
    others = np.stack([api.fit_begin(s.ravel(), -1.0, 1.0, maxit=MAXIT) for s in design.make_starts(39, 7, 2, 99)])
    r = launch(handle, pr, np.concatenate([others, s0[j:j + 1]]), CAP)   # last of 40
    check(r, 39, want[j], tr_f[j], tr_s[j])
    try:
        for byte in (0x00, 0x3F, 0xFF):   # whatever the handle's buffers held
            handle.debug_fill_scratch(byte)
            r = launch(handle, pr, s0, CAP)
            for k in range(4):
                check(r, k, want[k], tr_f[k], tr_s[k])
        rng = np.random.default_rng(3)   # whatever ran before
        Xb = rng.random((300, 3))
        handle.loglik_batch(Xb, np.sin(Xb).sum(axis=1), 2, np.array([[0.5, 0.5, 1.0, 2.0, 3.0, 30.0, 40.0, 50.0]]), 1.0)
        handle.mixed_logdet_grad_designs(rng.uniform(-1.0, 1.0, (3, 40, 3)), 2, params_row(0.5, 3.0, 12.0, 3), 5)
        r = launch(handle, pr, s0, CAP)
        for k in range(4):
            check(r, k, want[k], tr_f[k], tr_s[k])
    finally:
        handle.debug_fill_scratch(-1)


def test_a_start_on_a_coincident_pair(handle, reference_runs):
    pr, want, tr_f, tr_s, _ = reference_runs((14, 2, 0))
    bad = pr["starts"][1].copy()
    bad[3] = bad[4]   # two coincident rows: R is singular
    state = np.stack([pr["state"][0], api.fit_begin(bad.ravel(), -1.0, 1.0, maxit=MAXIT), pr["state"][2]])
    r = launch(handle, pr, state, CAP)
    assert r["state"][1, api.FIT_CODE] == api.FIT_NOT_EVALUABLE and r["evals"][1] == 1 and r["failed"] >= 1
    assert np.isnan(r["trace_f"][1, 0]) and r["trace_status"][1, 0] > 0 and np.isinf(r["state"][1, api.FIT_F])
    f, g, st = handle.design_fit_eval(bad[None], 2, pr["row"])
    assert st[0] == r["trace_status"][1, 0] and bits(f)[0] == 0x7ff8000000000000 and np.isnan(g).all()
    check(r, 0, want[0], tr_f[0], tr_s[0])
    check(r, 2, want[2], tr_f[2], tr_s[2])


def test_refusals_leave_the_handle_as_it_was(handle):
    n, d, nf = 21, 2, 14
    pr = problem(n, d, nf)
    s0 = pr["state"][:2]
    launch(handle, pr, s0, 2)
    handle.design_fit_eval(pr["starts"][:2], 2, pr["row"], pr["D_old"])
    before = handle.workspace_bytes()
    L = api.lib()
    old = np.ascontiguousarray(np.asfortranarray(pr["D_old"]).ravel(order="F"))
    row = np.ascontiguousarray(pr["row"])

    def call(A=2, state=None, max_evals=(2, 2), T=4, tr_f=True, tr_s=True, n=n, d=d, K=2, nf=nf, old=old, row=row, ev=True, me=True,
             st=True):
        state = np.array(s0) if state is None else state
        mx = np.array(max_evals, dtype=np.int32)
        evals = np.full(2, -7, dtype=np.int32)
        f, s = np.full((2, max(T, 1)), 5.0), np.full((2, max(T, 1)), 9, dtype=np.int32)
        keep = state.copy()
        rc = L.ccgp_design_fit(handle._h, api._p(old), nf, n, d, K, api._p(row), 0.25, A, api._p(state) if st else None,
                               api._ipt(mx) if me else None, api._ipt(evals) if ev else None, api._p(f) if tr_f else None,
                               api._ipt(s) if tr_s else None, T)
        assert same_bits(state, keep) and (evals == -7).all() and (f == 5.0).all() and (s == 9).all()
        return rc
    wrong_d = np.array(s0)
    wrong_d[1, 0] = 13
    for kw in (dict(A=-1), dict(T=-1), dict(max_evals=(2, 5)), dict(max_evals=(-1, 2)), dict(max_evals=(2, 4097), T=5000),
               dict(tr_s=False), dict(tr_f=False), dict(old=None), dict(row=None), dict(ev=False), dict(me=False), dict(st=False),
               dict(state=wrong_d), dict(d=0), dict(d=65), dict(n=0), dict(K=0), dict(K=9), dict(nf=-1), dict(nf=n),
               dict(nf=n + 1)):
        assert call(**kw) == -1, kw
    assert call(A=0) == 0
    # unsupported: n = 129, nv = 65, the Matern family
    assert call(n=129, nf=122) == -4
    s65 = np.zeros((2, HDR + 16 * 65))
    assert call(n=13, d=5, nf=0, old=None, row=np.ascontiguousarray(params_row(0.5, 1.0, 4.0, 5)), state=s65) == -4
    handle.set_kernel(api.KERNEL_MATERN, 2.5)
    try:
        s1 = np.stack([api.fit_begin(np.linspace(-0.5, 0.5, 7), -1.0, 1.0)] * 2)
        assert call(n=7, d=1, nf=0, old=None, row=np.ascontiguousarray(params_row(0.5, 1.0, 4.0, 1)), state=s1) == -4
        with pytest.raises(api.CcgpError) as e:
            handle.design_fit_eval(np.linspace(-0.5, 0.5, 7).reshape(1, 7, 1), 2, params_row(0.5, 1.0, 4.0, 1))
        assert e.value.code == -4
    finally:
        handle.set_kernel(0, 0.0)
    # the twin's evaluator: its own refusals, outputs untouched
    x = np.ascontiguousarray(pr["starts"][:2])

    def call_eval(B=2, n=n, nf=nf, old=old, row=row, xp=True, of=True, og=True):
        f, g, st = np.full(2, 5.0), np.full(x.shape, 5.0), np.full(2, 9, dtype=np.int32)
        rc = L.ccgp_design_fit_eval(handle._h, api._p(old), nf, n, d, 2, api._p(row), 0.0, api._p(x) if xp else None, B,
                                    api._p(f) if of else None, api._p(g) if og else None, api._ipt(st))
        assert (f == 5.0).all() and (g == 5.0).all() and (st == 9).all()
        return rc
    for kw in (dict(B=-1), dict(nf=-1), dict(nf=n), dict(old=None), dict(row=None), dict(xp=False), dict(of=False), dict(og=False),
               dict(n=0)):
        assert call_eval(**kw) == -1, kw
    assert call_eval(B=0) == 0
    assert handle.workspace_bytes() == before
    # nv = 65 on the driver: minimize_starts over the twin's evaluator
    S = design.make_starts(2, 13, 5, 1)
    row5 = params_row(0.5, 1.0, 4.0, 5)
    got = design.minimize_starts_device(handle, S, 2, row5, maxit=3)

    def evaluate(X):
        ld, g, st = handle.mixed_logdet_grad_designs(X, 2, row5, 0)
        return -ld, -g, st
    want = design.minimize_starts(evaluate, S, maxit=3)
    assert same_bits(got["x"], want["x"]) and same_bits(got["f"], want["f"])
    # (128, 8, 124): the design gradient's carve fits (20011 of 20472 doubles) but not with the 562 words of a start of nv = 32
    # behind it: the device call refuses, the driver goes to the twin by itself
    rng = np.random.default_rng(5)
    D_old = design.make_starts(1, 124, 8, rng)[0]
    S = design.make_starts(2, 4, 8, rng)
    row8 = params_row(0.5, 0.84, 3.36, 8)
    with pytest.raises(api.CcgpError) as e:
        handle.design_fit(4, 8, 2, row8, np.stack([api.fit_begin(s.ravel(), -1.0, 1.0) for s in S]), 2, D_old)
    assert e.value.code == -4
    a = design.minimize_starts_device(handle, S, 2, row8, D_old=D_old, maxit=3)
    b = design.minimize_starts_device(handle, S, 2, row8, D_old=D_old, maxit=3, on_device=False)
    assert same_bits(a["x"], b["x"]) and same_bits(a["f"], b["f"]) and np.isfinite(a["f"]).all() and a["calls"] == b["calls"]


def _same_result(dev, base):
    assert sorted(dev) == sorted(base)
    for k in base:
        if k != "device_calls":
            a, b = np.asarray(dev[k]), np.asarray(base[k])
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def test_entropy_optim_on_the_device(handle):
    gp = CombinedGP("BSQ", handle=handle)
    base = gp.Entropy_optim(14, 2, *BSQ_PRIOR, 20, rng=0)
    dev = gp.Entropy_optim(14, 2, *BSQ_PRIOR, 20, rng=0, on_device=True)
    _same_result(dev, base)
    # every start stops within one launch of 512 evaluations: device_calls is at most the number of launches + 1
    assert dev["device_calls"] == 1 < base["device_calls"]
    print("Entropy_optim: %d device calls (lockstep: %d)" % (dev["device_calls"], base["device_calls"]))
    # it finds `Initial ME Design.txt` again, under the conditions of tests/test_gpu_design_grad.py
    D0 = initial_me_design()
    ld0, st0 = handle.mixed_logdet_designs(D0[None], 2, params_row(*BSQ_PRIOR, 2))
    assert st0[0] == 0 and dev["logdet"] >= ld0[0] - 1e-7 and design_distance(dev["Design"], D0) <= 1e-3


def test_batch_entropy_optim_on_the_device(handle):
    gp = CombinedGP("BSQ", handle=handle)
    D0 = initial_me_design()
    S = design.make_starts(25, 7, 2, 0)
    base = gp.Batch_Entropy_optim(D0, 7, 2, *BSQ_PRIOR, 25, starts=S)
    dev = gp.Batch_Entropy_optim(D0, 7, 2, *BSQ_PRIOR, 25, starts=S, on_device=True)
    _same_result(dev, base)
    assert dev["device_calls"] == 2 < base["device_calls"]   # one launch, and log det R(D.old)
    print("Batch_Entropy_optim: %d device calls (lockstep: %d)" % (dev["device_calls"], base["device_calls"]))
    assert abs(dev["logdet"] - (-7.67936)) <= 1e-5   # the Schur criterion of the second batch (tests/test_design_optim.py)
