"""The portable Nelder-Mead stepper (csrc/nm_logic.h through ccgp_nm_begin / ccgp_nm_feed) against fit.laplace_sets, without a
GPU.  First numpy is held to the summation order the header assumes.  Then laplace_sets and the stepper are given the same
closed forms: mode, value, iterations, the charged evaluation count and the converged flag must agree as bytes; every point
the stepper asks for must be, in order, one of the points laplace_sets asked for (the stepper asks for one value at a time
where laplace_sets sends four), with the same value stored; and the final simplex must consist of such points, best first.
The forms together take every branch of the search, shown by the state's counters."""
import numpy as np
import pytest

from ccgp_amd import api, fit


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("p", range(1, 9))
def test_numpy_sums_a_block_row_after_row(p):
    """xbar = sim[:-1].sum(axis=0) / p: left to right from vertex 0, no pairwise blocks, for every p a search can have."""
    rng = np.random.default_rng(p)
    for scale in (1.0, 1e8, 1e-8):
        sim = rng.standard_normal((p + 1, p)) * scale * np.exp(3.0 * rng.standard_normal((p + 1, p)))
        want = sim[0].copy()
        for v in range(1, p):
            want = want + sim[v]
        assert same_bits(sim[:-1].sum(axis=0), want)
        big = rng.standard_normal((3, p + 1, p))   # the slice laplace_sets takes: sim[c, :-1] of a [C, p + 1, p] array
        want = big[1, 0].copy()
        for v in range(1, p):
            want = want + big[1, v]
        assert same_bits(big[1, :-1].sum(axis=0), want)


# ---- closed forms: rows [B, q] -> values [B] -------------------------------------------------------------------------------
def bowl(x):
    return -((x - np.arange(1, x.shape[1] + 1) * 0.3) ** 2 * (1.0 + np.arange(x.shape[1]))).sum(axis=1)


def valley(x):
    """A curved ridge (Rosenbrock's, negated; for q = 1 a quartic): long runs of expansions and both contractions."""
    if x.shape[1] == 1:
        return -(x[:, 0] - 1.0) ** 4 - 0.5 * (x[:, 0] - 1.0) ** 2
    return -(100.0 * (x[:, 1:] - x[:, :-1] ** 2) ** 2 + (1.0 - x[:, :-1]) ** 2).sum(axis=1)


def banded(x):
    """Not evaluable in a band of x0: the contraction fails there and the simplex shrinks."""
    v = 2.0 * x[:, 0] - 0.1 * x[:, 0] ** 4 - ((x[:, 1:] - 0.5) ** 2).sum(axis=1)
    return np.where((x[:, 0] > 1.003) & (x[:, 0] < 1.045), np.nan, v)


def start(kind, q):
    if kind == "shrink":
        return np.concatenate([[1.0, 0.4, 0.5], np.full(8, 0.45)])[:q]
    if kind == "zero":
        return np.concatenate([[0.0, 1.2, -0.7, 0.0], np.linspace(0.5, 2.0, 8)])[:q]
    if kind == "far":
        return np.concatenate([[-1.2, 1.0, 2.5], np.linspace(-2.0, 2.0, 8)])[:q]
    return np.full(q, 0.25)


CASES = [(form, q, kind, maxiter)
         for form in (bowl, valley, banded) for q in (1, 2, 3, 4, 8) for kind, maxiter in
         (("zero", 2000), ("far", 2000), ("flat", 2000), ("shrink", 2000), ("far", 37), ("zero", 0))]


def drive(form, x0, maxiter):
    """The stepper, one evaluation at a time -> (state, the points asked for, the values stored)."""
    state = api.nm_begin(x0, 1e-6, 1e-9, maxiter)
    asked, stored = [], []
    for _ in range(200000):
        x = api.nm_trial(state)
        v = float(form(x[None])[0])
        asked.append(x)
        stored.append(v)
        if api.nm_feed(state, v) != api.NM_RUNNING:
            break
    return state, asked, stored


@pytest.mark.parametrize("form,q,kind,maxiter", CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_stepper_is_laplace_sets(form, q, kind, maxiter):
    x0 = start(kind, q)
    sent = []

    def fn_sets(rows, set_of):
        vals = form(np.asarray(rows))
        sent.append((np.array(rows), np.array(vals)))
        return vals

    want = fit.laplace_sets(fn_sets, x0[None], maxiter=maxiter)[0]
    sent = sent[:-1]   # the last call holds the Hessian's points
    pts = np.concatenate([r for r, _ in sent])
    vals = np.concatenate([v for _, v in sent])
    state, asked, stored = drive(form, x0, maxiter)
    assert state[api.NM_CODE] == (api.NM_CONVERGED if want["converged"] else api.NM_MAXITER)
    sim, fsim = api.nm_simplex(state)
    assert same_bits(sim[0], want["mode"]) and same_bits(fsim[0], want["value"])
    assert state[api.NM_ITERATIONS] == want["iterations"] and state[api.NM_CHARGED] == want["evaluations"]
    assert state[api.NM_FED] == len(asked) <= want["evaluations"]
    # every point asked for is, in order, one of laplace_sets' points
    at = 0
    keys = [r.tobytes() for r in pts]
    for x, v in zip(asked, stored):
        k = x.tobytes()
        while at < len(keys) and keys[at] != k:
            at += 1
        assert at < len(keys), "a point laplace_sets never asked for"
        assert same_bits(vals[at], v)
        at += 1
    # the final simplex: points that were evaluated, with their values (-1e300 where not finite), best first
    known = {r.tobytes(): (v if np.isfinite(v) else -1e300) for r, v in zip(pts, vals)}
    for v in range(q + 1):
        assert same_bits(known[sim[v].tobytes()], fsim[v])
    assert (np.diff(fsim) <= 0.0).all()
    c = {k: int(state[i]) for k, i in api.NM_COUNTERS.items()}
    assert c["expansion_taken"] + c["expansion_refused"] + c["reflection"] + c["outside_contraction"] + \
        c["inside_contraction"] + c["shrink"] == want["iterations"]
    assert want["evaluations"] == q + 1 + 4 * want["iterations"] + q * c["shrink"]
    if maxiter == 37:
        assert not want["converged"] and want["iterations"] < 37 and want["evaluations"] >= 37
    if maxiter == 0:
        assert want["iterations"] == 0 and len(asked) == q + 1
    if form is banded and kind == "shrink" and q in (3, 4):
        assert c["shrink"] > 0


def test_every_branch_was_taken():
    _counters = {}
    for form, q, kind, maxiter in CASES:
        state = drive(form, start(kind, q), maxiter)[0]
        _counters[(form.__name__, q, kind, maxiter)] = {k: int(state[i]) for k, i in api.NM_COUNTERS.items()}
    total = {k: sum(c[k] for c in _counters.values()) for k in api.NM_COUNTERS}
    print(total)
    assert all(v > 0 for v in total.values()), total
    for q in (1, 2, 3, 4, 8):
        per_q = {k: sum(c[k] for key, c in _counters.items() if key[1] == q) for k in api.NM_COUNTERS}
        assert per_q["expansion_taken"] > 0 and per_q["inside_contraction"] > 0, (q, per_q)


def test_cut_anywhere_the_state_carries_the_search():
    """A state copied between any two evaluations goes on to the same end: nothing of a search lives outside its state."""
    x0 = start("shrink", 4)
    whole, asked, stored = drive(banded, x0, 2000)
    state = api.nm_begin(x0, 1e-6, 1e-9, 2000)
    for v in stored:
        state = np.array(state)   # a fresh copy every evaluation
        api.nm_feed(state, v)
    assert same_bits(state, whole)
    assert api.nm_feed(state, 1.0) == state[api.NM_CODE] and same_bits(state, whole)   # a stopped search stays as it is


def test_refusals():
    L = api.lib()
    assert [api.nm_state_doubles(q) for q in (1, 3, 4, 8)] == [24, 42, 54, 122]
    assert L.ccgp_nm_state_doubles(0) == -1 and L.ccgp_nm_state_doubles(9) == -1
    with pytest.raises(api.CcgpError):
        api.nm_state_doubles(9)
    x = np.ones(9)
    state = np.zeros(api.nm_state_doubles(8))
    for q, st, x0, maxiter in ((0, state, x, 10), (9, state, x, 10), (3, None, x, 10), (3, state, None, 10), (3, state, x, -1)):
        keep = state.copy()
        assert L.ccgp_nm_begin(api._p(st), q, api._p(x0), 1e-6, 1e-9, maxiter) == -1
        assert same_bits(state, keep)
    s3 = api.nm_begin(np.ones(3))
    keep = s3.copy()
    assert L.ccgp_nm_feed(api._p(s3), 4, 1.0) == -1 and L.ccgp_nm_feed(None, 3, 1.0) == -1
    assert L.ccgp_nm_feed(api._p(s3), 0, 1.0) == -1 and L.ccgp_nm_feed(api._p(s3), 9, 1.0) == -1
    for word, value in ((api.NM_Q, 4.0), (api.NM_CODE, 3.0), (api.NM_CODE, 0.5), (api.NM_PHASE, 6.0), (3, 4.0), (3, -1.0)):
        bad = keep.copy()
        bad[word] = value
        assert L.ccgp_nm_feed(api._p(bad), 3, 1.0) == -1, (word, value)
    assert same_bits(s3, keep)
    with pytest.raises(ValueError):
        api.nm_feed(s3[:10], 1.0)
    with pytest.raises(ValueError):
        api.nm_feed(np.zeros(42), 1.0)
    assert api.nm_feed(s3, 1.0) == api.NM_RUNNING and s3[api.NM_FED] == 1
