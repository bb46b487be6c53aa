"""The Laplace search on the device (ccgp_laplace_search_sets, fit.laplace_device_sets) against its host twin
(ccgp_chain_logpost_sets driven one evaluation at a time through ccgp_nm_feed): the final state and the whole trace bit for
bit, one training set and start per NM instance of small_reg_kernel (tests/chain_cases.py: NB = 1 .. 8, general and FULL, four
priors); three searches run to convergence against fit.laplace_sets over the twin evaluator; a search's independence of the
other searches, of its position, of how its evaluations are cut into calls and of what the handle ran before; a vertex that
cannot be factorised; refusals; fit.study(device_chains=True, device_laplace=True) against fit.study(device_chains=True).

Every evaluation of the twin is ccgp_chain_logpost_sets on the state's trial point, so "device == twin" holds the kernel's
evaluation inside the loop to that call's bits as well as the step to ccgp_nm_feed's.

Module time on an MI355X: see profiles/device_laplace.md."""
import numpy as np
import pytest

from chain_cases import CASES, make_case, training_set
from conftest import load_gv
from ccgp_amd import api, fit
from ccgp_amd.rsurface import CombinedGP

pytestmark = pytest.mark.gpu

CAP = 4096
SHORT = 400            # maxiter of the short runs: about 99 iterations and 180 evaluations
TO_THE_END = [(17, 2, "ANI"), (50, 9, "GV"), (65, 3, "ISO")]
IDS = ["%d-%d-%s" % c[:3] for c in CASES]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def problem(c):
    case = make_case(*c)
    return dict(Xs=case["D"][None], ys=case["y"][None], s2=[case["s2"]], prior=case["prior"], pars=case["pars"],
                x0=case["theta0"], script=case["script"])


def search(h, p, set_of, state, max_evals, **kw):
    return h.laplace_search_sets(p["Xs"], p["ys"], p["s2"], p["prior"], set_of, state, max_evals, p["pars"], trace=True, **kw)


def twin(h, p, set_of, state, max_evals=CAP):
    """The contract's sequential form, all searches side by side -> (state, trace_val, trace_status), lists per search."""
    state = np.array(state)
    A = state.shape[0]
    set_of = np.asarray(set_of)
    tr_v, tr_s = [[] for _ in range(A)], [[] for _ in range(A)]
    for _ in range(max_evals):
        live = np.flatnonzero(state[:, api.NM_CODE] == api.NM_RUNNING)
        if live.size == 0:
            break
        val, _, _, st = h.chain_logpost_sets(p["Xs"], p["ys"], p["s2"], p["prior"], api.nm_trial(state[live]), set_of[live],
                                             p["pars"])
        for k, a in enumerate(live):
            api.nm_feed(state[a], val[k])
            tr_v[a].append(val[k])
            tr_s[a].append(int(st[k]))
    return state, tr_v, tr_s


def check(r, j, want_state, tr_v, tr_s, t0=0, used=None):
    used = len(tr_v) - t0 if used is None else used
    assert r["evals"][j] == used
    assert same_bits(r["trace_val"][j, :used], tr_v[t0:t0 + used])
    assert np.array_equal(r["trace_status"][j, :used], tr_s[t0:t0 + used])
    assert np.isnan(r["trace_val"][j, used:]).all() and (r["trace_status"][j, used:] == -1).all()
    if want_state is not None:
        assert same_bits(r["state"][j], want_state)


@pytest.fixture(scope="module")
def short_runs(handle):
    """Per case: the problem, the start state with maxiter = SHORT, the twin's run and the device's, computed once."""
    cache = {}

    def get(c):
        if c not in cache:
            p = problem(c)
            s0 = api.nm_begin(p["x0"], maxiter=SHORT)[None]
            want, tr_v, tr_s = twin(handle, p, [0], s0)
            cache[c] = (p, s0, want, tr_v, tr_s, search(handle, p, [0], s0, CAP, T=CAP))
        return cache[c]
    return get


@pytest.fixture(scope="module")
def full_runs(handle):
    """The searches of TO_THE_END run to convergence on the device, once."""
    cache = {}

    def get(key):
        if key not in cache:
            p = problem([c for c in CASES if c[:3] == key][0])
            cache[key] = (p, search(handle, p, [0], api.nm_begin(p["x0"])[None], CAP, T=CAP))
        return cache[key]
    return get


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_device_search_is_the_twin(handle, short_runs, c):
    p, s0, want, tr_v, tr_s, r = short_runs(c)
    assert want[0, api.NM_CODE] == api.NM_MAXITER and SHORT <= want[0, api.NM_CHARGED] < SHORT + 4 + len(p["x0"])
    # charged = q + 1 + 4 iterations + q shrinks; an iteration makes one evaluation at the least
    q, it = len(p["x0"]), int(want[0, api.NM_ITERATIONS])
    assert want[0, api.NM_CHARGED] == q + 1 + 4 * it + q * want[0, api.NM_COUNTERS["shrink"]]
    assert q + 1 + it <= len(tr_v[0]) == want[0, api.NM_FED] < want[0, api.NM_CHARGED] and not any(tr_s[0])
    check(r, 0, want[0], tr_v[0], tr_s[0])
    assert r["failed"] == 0
    print("%s: %d iterations, %d evaluations (charged %d)" % (c[:3], want[0, api.NM_ITERATIONS], len(tr_v[0]),
                                                              want[0, api.NM_CHARGED]))
    # cut by max_evals = 7 per call, the state of one call the start of the next
    state, t0 = s0, 0
    while state[0, api.NM_CODE] == api.NM_RUNNING:
        r = search(handle, p, [0], state, 7)
        check(r, 0, None, tr_v[0], tr_s[0], t0, min(7, len(tr_v[0]) - t0))
        state, t0 = r["state"], t0 + int(r["evals"][0])
    assert same_bits(state, want)
    # max_evals = 0: the state as it came, nothing evaluated; a stopped search is returned as it came
    r = search(handle, p, [0], s0, 0, T=4)
    assert same_bits(r["state"], s0) and not r["evals"].any() and np.isnan(r["trace_val"]).all()
    r = search(handle, p, [0], want, 5)
    assert same_bits(r["state"], want) and not r["evals"].any()


@pytest.mark.parametrize("key", [(17, 2, "ANI"), (50, 9, "GV")], ids=lambda k: "%d-%d-%s" % k)
def test_one_evaluation_per_call(handle, short_runs, key):
    p, s0, want, tr_v, tr_s, _ = short_runs([c for c in CASES if c[:3] == key][0])
    state = s0
    for t in range(40):
        r = search(handle, p, [0], state, 1)
        check(r, 0, None, tr_v[0], tr_s[0], t, 1)
        state = r["state"]
    assert same_bits(state, twin(handle, p, [0], s0, max_evals=40)[0])


@pytest.mark.parametrize("key", TO_THE_END, ids=lambda k: "%d-%d-%s" % k)
def test_converged_search_is_laplace_sets_over_the_twin(handle, full_runs, key):
    p, r = full_runs(key)
    state = r["state"][0]

    def fn(rows, set_of):
        return handle.chain_logpost_sets(p["Xs"], p["ys"], p["s2"], p["prior"], rows, set_of, p["pars"])[0]

    want = fit.laplace_sets(fn, p["x0"][None])[0]
    sim, val = api.nm_simplex(state)
    assert want["converged"] and state[api.NM_CODE] == api.NM_CONVERGED
    assert same_bits(sim[0], want["mode"]) and same_bits(val[0], want["value"])
    assert state[api.NM_ITERATIONS] == want["iterations"] and state[api.NM_CHARGED] == want["evaluations"]
    assert state[api.NM_FED] == r["evals"][0] < want["evaluations"] and r["failed"] == 0
    print("%s: %d iterations, %d evaluations on the device, %d charged" % (key, want["iterations"], r["evals"][0],
                                                                        want["evaluations"]))
    # the driver: every key of laplace_sets' dict
    gp = CombinedGP(p["script"], handle=handle)
    got = fit.laplace_device_sets(gp, p["Xs"], p["ys"], p["s2"], p["x0"][None])[0]
    assert sorted(set(got) - set(want)) == ["calls", "fed"] and got["calls"] == -(-got["fed"] // 512) + 1
    for k in want:
        assert same_bits(got[k], want[k]), k


def test_every_branch_occurred_on_the_device(short_runs, full_runs):
    total = dict.fromkeys(api.NM_COUNTERS, 0)
    states = [short_runs(c)[5]["state"][0] for c in CASES] + [full_runs(k)[1]["state"][0] for k in TO_THE_END]
    for s in states:
        for k, i in api.NM_COUNTERS.items():
            total[k] += int(s[i])
    print(total)
    for k in ("expansion_taken", "reflection", "outside_contraction", "inside_contraction", "shrink"):
        assert total[k] > 0, total


def gv_problem():
    """Three Ground-Vibrations sets of one shape (50, 9) and the short run of a search on set 1."""
    sets = [training_set(50, 9, s) for s in (5, 6, 7)]
    return dict(Xs=np.stack([s[0] for s in sets]), ys=np.stack([s[1] for s in sets]),
                s2=[float(np.var(s[1], ddof=1)) for s in sets], prior=api.PRIOR_GV, pars=None)


def test_a_search_depends_on_its_own_inputs_only(handle):
    p = gv_problem()
    s0 = np.stack([api.nm_begin([1.0, 1.0, 0.0], maxiter=SHORT), api.nm_begin([0.5, 1.5, 0.3], maxiter=SHORT),
                   api.nm_begin([1.0, 1.0, 0.0], maxiter=SHORT)])
    set_of = [0, 1, 1]
    want, tr_v, tr_s = twin(handle, p, set_of, s0)
    assert not same_bits(want[0], want[2])          # one start on two sets: two searches
    r = search(handle, p, set_of, s0, CAP)
    for k in range(3):
        check(r, k, want[k], tr_v[k], tr_s[k])
    j = 2
    # alone
    r = search(handle, p, [set_of[j]], s0[j:j + 1], CAP)
    check(r, 0, want[j], tr_v[j], tr_s[j])
    # last of 40, among searches of all three sets
    rng = np.random.default_rng(99)
    others = np.stack([api.nm_begin([1.0, 1.0, 0.0] + 0.3 * rng.standard_normal(3), maxiter=SHORT) for _ in range(39)])
    r = search(handle, p, [k % 3 for k in range(39)] + [set_of[j]], np.concatenate([others, s0[j:j + 1]]), CAP)
    check(r, 39, want[j], tr_v[j], tr_s[j])
    # the sets permuted
    q = dict(p, Xs=p["Xs"][[2, 1, 0]], ys=p["ys"][[2, 1, 0]], s2=[p["s2"][2], p["s2"][1], p["s2"][0]])
    r = search(handle, q, [0, 2, 1], np.stack([others[0], s0[0], s0[j]]), CAP)
    check(r, 2, want[j], tr_v[j], tr_s[j])
    check(r, 1, want[0], tr_v[0], tr_s[0])
    # whatever the handle's buffers held, whatever ran before
    handle.debug_fill_scratch(0xFF)
    try:
        r = search(handle, p, set_of, s0, CAP)
        for k in range(3):
            check(r, k, want[k], tr_v[k], tr_s[k])
        Xb = rng.random((300, 3))
        handle.loglik_batch(Xb, np.sin(Xb).sum(axis=1), 2, np.array([[0.5, 0.5, 1.0, 2.0, 3.0, 30.0, 40.0, 50.0]]), 1.0)
        handle.profile_batch_sets(p["Xs"], p["ys"], 1, np.ones((5, 10)), [0, 1, 0, 1, 2])
        handle.profile_fit_sets(p["Xs"], p["ys"], [0, 1], np.stack([api.fit_begin(np.zeros(9), -12.0, 12.0)] * 2), 5)
        r = search(handle, p, set_of, s0, CAP)
        for k in range(3):
            check(r, k, want[k], tr_v[k], tr_s[k])
    finally:
        handle.debug_fill_scratch(-1)


def test_a_vertex_that_cannot_be_factorised(handle):
    """Rates of exp(-40) in both components: every entry of R is exactly 1 and the factorisation fails.  Vertex 2 of the
    initial simplex is put there: its value is not finite, the search stores 1e300 for it and goes on."""
    p = gv_problem()
    good = api.nm_begin([1.0, 1.0, 0.0], maxiter=SHORT)
    bad = good.copy()
    bad[api.NM_HEADER + 2 * 3:api.NM_HEADER + 3 * 3] = [-40.0, -40.0, 0.0]
    state = np.stack([good, bad, good])
    r = search(handle, p, [0, 1, 1], state, CAP)
    want, tr_v, tr_s = twin(handle, p, [0, 1, 1], state)
    for j in range(3):
        check(r, j, want[j], tr_v[j], tr_s[j])
    assert np.isnan(r["trace_val"][1, 2]) and r["trace_status"][1, 2] >= 1
    sim, val = api.nm_simplex(r["state"][1])
    assert r["evals"][1] > 10 and r["state"][1, api.NM_CODE] != api.NM_RUNNING and np.isfinite(val).all() and val[0] > -1e299
    assert r["failed"] == sum(int(s != 0) for t in tr_s for s in t) >= 1
    alone = search(handle, p, [0, 1], np.stack([good, good]), CAP)
    assert same_bits(alone["state"], r["state"][[0, 2]])


def test_refusals_leave_the_handle_as_it_was(handle):
    p = gv_problem()
    n, d = 50, 9
    s0 = np.stack([api.nm_begin([1.0, 1.0, 0.0])] * 2)
    search(handle, p, [0, 1], s0, 2)
    before = handle.workspace_bytes()
    L = api.lib()
    Xb, yb, s2b, idx, C, _, _ = handle._sets(p["Xs"], p["ys"], p["s2"], [0, 1], 2)

    def call(C=C, A=2, idx=idx, state=None, max_evals=(2, 2), T=4, tr_v=True, tr_s=True, n=n, d=d, Xp=Xb, ev=True,
             prior=api.PRIOR_GV, s2p=s2b):
        state = np.array(s0) if state is None else state
        me = np.array(max_evals, dtype=np.int32)
        evals = np.full(2, -7, dtype=np.int32)
        v, s = np.full((2, max(T, 1)), 5.0), np.full((2, max(T, 1)), 9, dtype=np.int32)
        keep = state.copy()
        rc = L.ccgp_laplace_search_sets(handle._h, api._p(Xp), n, d, api._p(yb), api._p(s2p), C, prior, None, A,
                                        api._ipt(np.asarray(idx, dtype=np.int32)), api._p(state), api._ipt(me),
                                        api._ipt(evals) if ev else None, api._p(v) if tr_v else None,
                                        api._ipt(s) if tr_s else None, T)
        assert same_bits(state, keep) and (evals == -7).all() and (v == 5.0).all() and (s == 9).all()
        return rc
    s4 = np.stack([api.nm_begin([1.0, 1.0, 0.0, 0.0])] * 2)       # the anisotropic script's state under a 3-parameter prior
    wrong_q = np.array(s0)
    wrong_q[1, api.NM_Q] = 4
    for kw in (dict(C=0), dict(A=-1), dict(idx=[0, 3]), dict(idx=[-1, 0]), dict(max_evals=(2, 5)), dict(max_evals=(-1, 2)),
               dict(max_evals=(2, 4097), T=5000), dict(tr_s=False), dict(tr_v=False), dict(Xp=None), dict(ev=False),
               dict(s2p=None), dict(state=wrong_q), dict(state=s4), dict(d=0), dict(T=-1), dict(prior=7),
               dict(prior=api.PRIOR_INVGAMMA), dict(prior=api.PRIOR_ANI)):
        assert call(**kw) == -1, kw
    assert call(A=0) == 0
    # unsupported: n = 129, the Matern family
    rng = np.random.default_rng(0)
    X129 = rng.random((2, 129, 2))
    big = dict(Xs=X129, ys=np.sin(3.0 * X129).sum(axis=2), s2=[1.0, 1.0], prior=api.PRIOR_ISO, pars=None)
    with pytest.raises(api.CcgpError) as e:
        search(handle, big, [0, 1], s0, 2)
    assert e.value.code == -4
    assert call(n=129, d=2, Xp=np.ascontiguousarray(np.transpose(X129, (0, 2, 1)))) == -4
    handle.set_kernel(api.KERNEL_MATERN, 2.5)
    try:
        assert call() == -4
    finally:
        handle.set_kernel(0, 0.0)
    assert handle.workspace_bytes() == before
    # n = 129 on the driver: the twin carries it
    gp = CombinedGP("ISO", handle=handle)
    x0 = np.array([[2.0, 3.5, 0.3], [2.0, 3.5, 0.3]])
    r = fit.laplace_device_sets(gp, big["Xs"], big["ys"], big["s2"], x0, maxiter=40)
    t = fit.laplace_device_sets(gp, big["Xs"], big["ys"], big["s2"], x0, maxiter=40, on_device=False)
    for a, b in zip(r, t):
        assert sorted(a) == sorted(b)
        for k in a:
            assert same_bits(a[k], b[k]), k


def test_study_with_device_laplace(handle):
    sets = [load_gv(50, i) for i in (1, 2)]
    gp = CombinedGP("GV", handle=handle)
    s2 = [float(np.var(s[1], ddof=1)) for s in sets]
    kw = dict(sigma2s=s2, device_chains=True)
    want = fit.study(gp, sets, 0.05, 150, 100, 20, 0.5, rngs=[1, 2], **kw)
    got = fit.study(gp, sets, 0.05, 150, 100, 20, 0.5, rngs=[1, 2], device_laplace=True, **kw)
    for a, b in zip(got["tables"], want["tables"]):
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for a, b in zip(got["chains"], want["chains"]):
        assert same_bits(a["sample"], b["sample"]) and a["proposals"] == b["proposals"]
    print("laplace calls: %d on the device, %d in lockstep" % (got["calls"]["laplace"], want["calls"]["laplace"]))
    assert got["calls"]["laplace"] <= 3 < want["calls"]["laplace"]
