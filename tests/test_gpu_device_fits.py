"""The ordinary-kriging fits on the device (ccgp_profile_fit_sets, fit.ordinary_kriging_fit_device_sets) against their host
twin (ccgp_profile_fit_eval_sets driven one evaluation at a time through ccgp_fit_feed): the final state and the whole trace
bit for bit, one shape per FIT instance NB = 1 .. 8 and d in {1, 2, 9}; a start's independence of the other starts, of its
position, of how its evaluations are cut into calls and of what the handle ran before; a start that cannot be evaluated;
refusals; and the fit end to end on the Qian and Ground-Vibrations data and through fit.study(device_fits=True).

Every evaluation of the twin is ccgp_profile_batch_sets on the row (1, exp(trial)), so "device == twin" holds the kernel's
evaluation inside the loop to that call's bits as well as the stepper to ccgp_fit_feed's."""
import numpy as np
import pytest

from conftest import golden, load_gv, load_hyper, load_qian
from ccgp_amd import api, fit
from ccgp_amd.rsurface import CombinedGP

pytestmark = pytest.mark.gpu

SHAPES_N = [2, 16, 17, 33, 50, 65, 90, 100, 113, 128]
CAP = 4096


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def route_is_reg(n, d):
    """small_route_fit of csrc/small_layout.h restated: the in-LDS tier's one-row carve (where the gradient has its register
    route at all), the gradient instance's carve, and the start's words behind it."""
    limit = (160 * 1024 - 64) // 8
    if n > 128:
        return False
    lds_tier = (n + 3) * n + d * n + 8 * n + (d + 8) + 8 * d + 8 + 16 + 256
    nb = (n + 15) // 16
    NP, XR = 16 * nb, 16 * (nb + 1)
    tail = NP + d + 1 + 2 * (NP + XR) + NP + 2 * NP + 8
    carve = d * n + tail + NP * (NP + 2) + 1 + 4 * 28
    return lds_tier <= limit and carve <= limit and carve + 2 * 256 + 2 + 64 + 16 + 16 * d <= limit


def make_sets(n, d, C=2, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    Xs = rng.random((C, n, d))
    ys = np.stack([np.sin(3.0 * X).sum(axis=1) + 0.3 * c + 0.05 * rng.standard_normal(n) for c, X in enumerate(Xs)])
    return Xs, ys


def begin(Xs, set_of, seed=0, lo=-12.0):
    """One state per start: kriging_starts' kind of point, spread by the seed -- the log of a rate over the squared spacing
    n^(-1/d) of the design, so that the start itself can be factorised at every shape (128 points on a line included)."""
    rng = np.random.default_rng(seed)
    n, d = Xs.shape[1:]
    return np.stack([api.fit_begin(np.log(rng.uniform(1.0, 5.0, size=d) * n ** (2.0 / d)), lo, 12.0) for _ in set_of])


def twin(h, Xs, ys, set_of, state, max_evals=CAP):
    """The contract's sequential form, all starts side by side: returns (state, evals, trace_f, trace_status) as lists per start."""
    state = np.array(state)
    A = state.shape[0]
    set_of = np.asarray(set_of)
    tr_f, tr_s = [[] for _ in range(A)], [[] for _ in range(A)]
    for _ in range(max_evals):
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        f, g, _, _, _, st = h.profile_fit_eval_sets(Xs, ys, api.fit_trial(state[live]), set_of[live])
        for k, a in enumerate(live):
            api.fit_feed(state[a], f[k], g[k], st[k] == 0)
            tr_f[a].append(f[k])
            tr_s[a].append(int(st[k]))
    return state, tr_f, tr_s


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

    def get(n, d):
        if (n, d) not in cache:
            Xs, ys = make_sets(n, d)
            set_of = [0, 1, 1]
            s0 = begin(Xs, set_of, seed=n + d)
            cache[(n, d)] = (Xs, ys, set_of, s0) + twin(handle, Xs, ys, set_of, s0)
        return cache[(n, d)]
    return get


@pytest.mark.parametrize("d", [1, 2, 9])
@pytest.mark.parametrize("n", SHAPES_N)
def test_device_fit_is_the_twin(handle, reference_runs, n, d):
    if not route_is_reg(n, d):
        Xs, ys = make_sets(n, d)
        with pytest.raises(api.CcgpError) as e:
            handle.profile_fit_sets(Xs, ys, [0], begin(Xs, [0]), 8, trace=True)
        assert e.value.code == -4
        return
    Xs, ys, set_of, s0, want, tr_f, tr_s = reference_runs(n, d)
    longest = max(len(t) for t in tr_f)
    assert 2 <= longest < CAP and (want[:, api.FIT_CODE] != api.FIT_RUNNING).all()
    # the gradient the stepper is fed is -(g_theta theta), the product spelled out, on the bits of ccgp_profile_batch_sets
    x = api.fit_trial(s0)
    f, g, theta, s2, beta, st = handle.profile_fit_eval_sets(Xs, ys, x, set_of)
    ll, s2p, betap, gp, stp = handle.profile_batch_sets(Xs, ys, 1, np.concatenate([np.ones((3, 1)), theta], axis=1), set_of)
    assert not st.any() and np.array_equal(st, stp)
    assert same_bits(f, -ll) and same_bits(g, -(gp[:, 1:] * theta)) and same_bits(s2, s2p) and same_bits(beta, betap)
    # all at once
    r = handle.profile_fit_sets(Xs, ys, set_of, s0, CAP, trace=True, T=CAP)
    assert r["failed"] == sum(int(s != 0) for t in tr_s for s in t)
    for j in range(3):
        check(r, j, want[j], tr_f[j], tr_s[j])
    print("n %d d %d: evaluations %s, codes %s" % (n, d, r["evals"].tolist(), want[:, api.FIT_CODE].astype(int).tolist()))
    # cut by max_evals = 7 per call, the state of one call the start of the next
    state, t0 = s0, np.zeros(3, dtype=int)
    while (state[:, api.FIT_CODE] == api.FIT_RUNNING).any():
        r = handle.profile_fit_sets(Xs, ys, set_of, state, 7, trace=True)
        for j in range(3):
            check(r, j, None, tr_f[j], tr_s[j], t0[j], min(7, len(tr_f[j]) - t0[j]))
        state, t0 = r["state"], t0 + r["evals"]
    assert same_bits(state, want)
    # max_evals = 0: the state as it came, nothing evaluated
    r = handle.profile_fit_sets(Xs, ys, set_of, s0, 0, trace=True, T=4)
    assert same_bits(r["state"], s0) and not r["evals"].any() and np.isnan(r["trace_f"]).all()
    # a stopped start is returned as it came
    r = handle.profile_fit_sets(Xs, ys, set_of, want, 5, trace=True)
    assert same_bits(r["state"], want) and not r["evals"].any()


@pytest.mark.parametrize("n,d", [(17, 9), (50, 2)])
def test_one_evaluation_per_call(handle, reference_runs, n, d):
    Xs, ys, set_of, s0, want, tr_f, tr_s = reference_runs(n, d)
    state, t0 = s0, np.zeros(3, dtype=int)
    for _ in range(40):
        r = handle.profile_fit_sets(Xs, ys, set_of, state, 1, trace=True)
        for j in range(3):
            check(r, j, None, tr_f[j], tr_s[j], t0[j], min(1, len(tr_f[j]) - t0[j]))
        state, t0 = r["state"], t0 + r["evals"]
    # 40 calls in: every start is where the twin was after as many evaluations
    for j in range(3):
        part = twin(handle, Xs, ys, [set_of[j]], s0[j:j + 1], max_evals=40)[0]
        assert same_bits(state[j], part[0])


def test_a_start_depends_on_its_own_inputs_only(handle, reference_runs):
    n, d = 50, 2
    Xs, ys, set_of, s0, want, tr_f, tr_s = reference_runs(n, d)
    j = 2
    # alone
    r = handle.profile_fit_sets(Xs, ys, [set_of[j]], s0[j:j + 1], CAP, trace=True)
    check(r, 0, want[j], tr_f[j], tr_s[j])
    # last of 40, among starts of both sets
    others = begin(Xs, list(range(39)), seed=99)
    r = handle.profile_fit_sets(Xs, ys, [k % 2 for k in range(39)] + [set_of[j]], np.concatenate([others, s0[j:j + 1]]), CAP,
                                trace=True)
    check(r, 39, want[j], tr_f[j], tr_s[j])
    # the sets permuted, a third one added
    X3, y3 = make_sets(n, d, C=3, seed=5)
    Xp, yp = np.stack([X3[2], Xs[1], Xs[0]]), np.stack([y3[2], ys[1], ys[0]])
    r = handle.profile_fit_sets(Xp, yp, [0, 2, 1], np.stack([others[0], s0[0], s0[j]]), CAP, trace=True)
    check(r, 2, want[j], tr_f[j], tr_s[j])
    check(r, 1, want[0], tr_f[0], tr_s[0])
    # whatever the handle's buffers held, whatever ran before
    handle.debug_fill_scratch(0xFF)
    try:
        r = handle.profile_fit_sets(Xs, ys, set_of, s0, CAP, trace=True)
        for k in range(3):
            check(r, k, want[k], tr_f[k], tr_s[k])
        rng = np.random.default_rng(3)
        Xb = rng.random((300, 3))
        handle.loglik_batch(Xb, np.sin(Xb).sum(axis=1), 2, np.array([[0.5, 0.5, 1.0, 2.0, 3.0, 30.0, 40.0, 50.0]]), 1.0)
        handle.profile_batch_sets(Xs, ys, 1, np.ones((5, 1 + d)), [0, 1, 0, 1, 0])
        handle.cgp_state_batch(Xs[0], ys[0], np.array([[0.3, 3.0, 2.0, 9.0, 8.0, 0.5]]))
        r = handle.profile_fit_sets(Xs, ys, set_of, s0, CAP, trace=True)
        for k in range(3):
            check(r, k, want[k], tr_f[k], tr_s[k])
    finally:
        handle.debug_fill_scratch(-1)


def test_a_start_that_cannot_be_evaluated(handle):
    """theta = 1e-17: every entry of R is exactly 1, the second pivot exactly 0 (the failed row of tests/test_gpu_cgp.py)."""
    n, d = 30, 2
    Xs, ys = make_sets(n, d)
    good = begin(Xs, [0, 1], seed=4)
    bad = api.fit_begin(np.log(np.full(d, 1e-17)), -60.0, 12.0)
    state = np.stack([good[0], bad, good[1]])
    r = handle.profile_fit_sets(Xs, ys, [0, 1, 1], state, CAP, trace=True)
    assert r["state"][1, api.FIT_CODE] == api.FIT_NOT_EVALUABLE and r["evals"][1] == 1
    assert np.isnan(r["trace_f"][1, 0]) and r["trace_status"][1, 0] == 2 and np.isinf(r["state"][1, api.FIT_F])
    want, tr_f, tr_s = twin(handle, Xs, ys, [0, 1, 1], state)
    for j in range(3):
        check(r, j, want[j], tr_f[j], tr_s[j])
    assert r["failed"] == sum(int(s != 0) for t in tr_s for s in t) >= 1
    alone = handle.profile_fit_sets(Xs, ys, [0, 1], good, CAP, trace=True)
    assert same_bits(alone["state"], r["state"][[0, 2]])


def test_refusals_leave_the_handle_as_it_was(handle):
    n, d = 20, 2
    Xs, ys = make_sets(n, d)
    s0 = begin(Xs, [0, 1])
    handle.profile_fit_sets(Xs, ys, [0, 1], s0, 2)
    before = handle.workspace_bytes()
    L = api.lib()
    Xb, yb, _, idx, C, _, _ = handle._sets(Xs, ys, None, [0, 1], 2)
    W = api.fit_state_doubles(d)

    def call(C=C, A=2, idx=idx, state=None, max_evals=(2, 2), T=4, tr_f=True, tr_s=True, n=n, d=d, Xp=Xb, ev=True):
        state = np.array(s0) if state is None else state
        me = np.array(max_evals, dtype=np.int32)
        evals = np.full(2, -7, dtype=np.int32)
        f, s = np.full((2, max(T, 1)), 5.0), np.full((2, max(T, 1)), 9, dtype=np.int32)
        keep = state.copy()
        rc = L.ccgp_profile_fit_sets(handle._h, api._p(Xp), n, d, api._p(yb), C, A, api._ipt(np.asarray(idx, dtype=np.int32)),
                                     api._p(state), api._ipt(me), api._ipt(evals) if ev else None, api._p(f) if tr_f else None,
                                     api._ipt(s) if tr_s else None, T)
        assert same_bits(state, keep) and (evals == -7).all() and (f == 5.0).all() and (s == 9).all()
        return rc
    wrong_d = np.array(s0)
    wrong_d[1, 0] = d + 1
    for kw in (dict(C=0), dict(A=-1), dict(idx=[0, 2]), dict(idx=[-1, 0]), dict(max_evals=(2, 5)), dict(max_evals=(-1, 2)),
               dict(max_evals=(2, 4097), T=5000), dict(tr_s=False), dict(tr_f=False), dict(Xp=None), dict(ev=False),
               dict(state=wrong_d), dict(d=0), dict(T=-1)):
        assert call(**kw) == -1, kw
    assert call(A=0) == 0
    # unsupported: n = 129, the Matern family
    X129, y129 = make_sets(129, 2)
    with pytest.raises(api.CcgpError) as e:
        handle.profile_fit_sets(X129, y129, [0, 1], s0, 2)
    assert e.value.code == -4
    X1, y1 = make_sets(20, 1)
    s1 = begin(X1, [0, 1])
    handle.set_kernel(api.KERNEL_MATERN, 2.5)
    try:
        with pytest.raises(api.CcgpError) as e:
            handle.profile_fit_sets(X1, y1, [0, 1], s1, 2)
        assert e.value.code == -4
        # the twin's evaluator serves what ccgp_profile_batch_sets serves: the value-only form of the Matern family
        f = handle.profile_fit_eval_sets(X1, y1, np.zeros((2, 1)), [0, 1], grad=False)[0]
        assert np.isfinite(f).all()
    finally:
        handle.set_kernel(0, 0.0)
    assert handle.workspace_bytes() == before
    # n = 129 on the driver: the twin carries it
    X129, y129 = make_sets(129, 9)
    r = fit.ordinary_kriging_fit_device_sets(handle, X129, y129, starts=2, rng=1)
    t = fit.ordinary_kriging_fit_device_sets(handle, X129, y129, starts=2, rng=1, on_device=False)
    for a, b in zip(r, t):
        assert same_bits(a["x"], b["x"]) and same_bits(a["f"], b["f"]) and a["sigma2"] == b["sigma2"]


def test_fit_on_qian(handle):
    D, y, _, _ = load_qian()
    ref = fit.ordinary_kriging_fit(handle, D, y, starts=8, rng=0)
    r = fit.ordinary_kriging_fit_device(handle, D, y, starts=8, rng=0)
    t = fit.ordinary_kriging_fit_device(handle, D, y, starts=8, rng=0, on_device=False)
    print("Qian: %d device calls for %d evaluations (lockstep: %d calls, %d evaluations), best log-likelihood %.6f (lockstep "
          "%.6f), sigma2 %.4f" % (r["calls"], r["evaluations"], ref["calls"], ref["evaluations"], r["loglik"], ref["loglik"],
                                  r["sigma2"]))
    assert sorted(r) == sorted(ref)
    assert abs(r["loglik"] - ref["loglik"]) <= 1e-3
    assert 57.5 <= r["sigma2"] <= 66.75
    assert r["calls"] == 2 and r["evaluations"] > 8
    for k in ("x", "f", "converged", "theta", "sigma2", "beta", "loglik", "evaluations"):
        assert same_bits(r[k], t[k]), k
    H = load_hyper("hx")
    _, arg = handle.grid_marginal(D, y, r["sigma2"], H, 1000, 50.0, True)
    assert arg == 292


def test_fit_on_ground_vibrations_from_the_mlegp_theta(handle):
    fx = golden("gv_mlegp_recovered.json")
    D, y, _, _ = load_gv(50)
    ref = fit.ordinary_kriging_fit_sets(handle, [D], [y], starts=8, rng=0, extra_starts=[fx["theta"]])[0]
    r = fit.ordinary_kriging_fit_device(handle, D, y, starts=8, rng=0, extra_starts=[fx["theta"]])
    print("GV: %d device calls for %d evaluations (lockstep: %d calls, %d evaluations), best log-likelihood %.6f (lockstep %.6f)"
          % (r["calls"], r["evaluations"], ref["calls"], ref["evaluations"], r["loglik"], ref["loglik"]))
    assert r["f"].shape == (9,)
    assert abs(r["loglik"] - ref["loglik"]) <= 1e-3


def test_study_with_device_fits(handle):
    sets = [load_gv(50, i) for i in (1, 2)]
    gp = CombinedGP("GV", handle=handle)
    r = fit.study(gp, sets, 0.05, 150, 100, 20, 0.5, rngs=[1, 2], single=True, device_fits=True)
    direct = fit.ordinary_kriging_fit_device_sets(handle, [s[0] for s in sets], [s[1] for s in sets])
    assert r["sigma2"] == [f["sigma2"] for f in direct]
    assert r["calls"]["sigma2"] == max(f["calls"] for f in direct) <= 3
    for tb in r["tables"]:
        for k in ("y_hat_single", "LL_single", "UL_single"):
            assert np.isfinite(tb[k]).all(), k
