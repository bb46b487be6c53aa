"""The portable quasi-Newton stepper (csrc/fit_logic.h through ccgp_fit_begin / ccgp_fit_feed) against design._Start, without a
GPU.  The kernel of ccgp_profile_fit_sets steps a start with this arithmetic, so it has to BE _Start: both are fed the same
(f, g, ok) and compared after every evaluation -- the bytes of the next trial point, f, the stopping code and the iteration
count.  The objectives are closed forms chosen so that every branch of the iteration is taken, and counters prove that it was.

fit_logic.h sums in the order np.add.reduce uses for these lengths; the first test holds numpy to that order, so a numpy that
sums differently fails HERE and not as an unexplained mismatch below.

The transform theta = exp(log theta) is chain_exp; ccgp_chain_terms exports it (theta1 = exp(psi1) of the GV prior's row), and
it is held to mpmath within chain_terms.h's 2 ulp band on [-12, 12].  That the gradient g_k = -(g_theta_k theta_k) has the bits
of that product spelled out needs the device's g_theta: tests/test_gpu_device_fits.py holds it."""
import math

import mpmath as mp
import numpy as np
import pytest

from ccgp_amd import api, design

DIMS = [1, 3, 7, 8, 9, 16, 17, 64]
CODES = {"": api.FIT_RUNNING, "REL_REDUCTION": api.FIT_CONV_REDUCTION, "PROJECTED GRADIENT": api.FIT_CONV_PROJ_GRAD,
         "maxit": api.FIT_MAXIT, "ABNORMAL": api.FIT_LINE_SEARCH, "cannot be evaluated": api.FIT_NOT_EVALUABLE}


def stated_sum(a):
    """The order fit_logic.h states for np.add.reduce at lengths up to 128."""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res = res + float(v)
        return res
    r = [float(v) for v in a[:8]]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + float(a[i + j])
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + float(v)
    return res


def test_numpy_sums_in_the_stated_order():
    rng = np.random.default_rng(20261020)
    for n in list(range(1, 20)) + [63, 64]:
        for _ in range(200):
            a = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, size=n)
            assert float(np.add.reduce(a)).hex() == stated_sum(a).hex(), n


def code_of(st):
    if st.running:
        return api.FIT_RUNNING
    return next(c for key, c in CODES.items() if key and key in st.message)


# ---- objectives: (x, evaluation index) -> (f, g, ok) ------------------------------------------------------------------------
def quadratic(sign):
    """Optimum outside the box [-1, 1]: beyond the upper bound in even coordinates, beyond the lower in odd ones (sign = 1)."""
    def fn(x, t):
        k = np.arange(x.size)
        c = sign * np.where(k % 2 == 0, 1.5, -1.7)
        w = 1.0 + 0.37 * k
        return float(0.5 * np.sum(w * (x - c) ** 2)), w * (x - c), True
    return fn


def rosenbrock(x, t):
    if x.size == 1:   # no chain in one dimension: a quartic with a ripple, whose secant steps overshoot
        v = x[0]
        return float(50.0 * v ** 4 - v + 3.0 * np.cos(9.0 * v)), np.array([200.0 * v ** 3 - 1.0 - 27.0 * np.sin(9.0 * v)]), True
    a, b = x[:-1], x[1:]
    g = np.zeros_like(x)
    g[:-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[1:] += 200.0 * (b - a * a)
    return float(np.sum(100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2)), g, True


def holed(how):
    """A quadratic with its optimum at 0.25 beside a region x_0 > 0.2 that cannot be evaluated: status (ok = False) or a NaN."""
    def fn(x, t):
        f, g = float(0.5 * np.sum((x - 0.25) ** 2)), x - 0.25
        if x[0] > 0.2:
            return (f, g, False) if how == "status" else (float("nan"), g, True)
        return f, g, True
    return fn


def unevaluable(x, t):
    return 1.0, np.zeros_like(x), False


def flat(x, t):
    return 3.0, np.zeros_like(x), True


def liar(honest):
    """Honest for `honest` evaluations (the start, then steps that fill the memory), then every trial is reported worse than
    the iterate.  Two lengths: how soon a first step is accepted depends on the dimension."""
    def fn(x, t):
        w = 1.0 + np.arange(x.size)
        if t < honest:
            return float(np.sum(np.cosh(w * (x + 0.4)))), w * np.sinh(w * (x + 0.4)), True
        return 1e6 + t, w, True
    return fn


CASES = [("quadratic+", quadratic(1.0), {}), ("quadratic-", quadratic(-1.0), {}), ("rosenbrock", rosenbrock, {}),
         ("hole-status", holed("status"), {}), ("hole-nan", holed("nan"), {}), ("unevaluable", unevaluable, {}),
         ("flat", flat, {}), ("liar2", liar(2), dict(max_backtracks=3)),
         ("liar4", liar(4), dict(max_backtracks=3)), ("maxit", rosenbrock, dict(maxit=3))]


def run_case(d, fn, opts, seen):
    rng = np.random.default_rng(7 * d + 1)
    x0 = rng.uniform(-0.9, 0.1, size=d)
    lo, hi = np.full(d, -1.0), np.full(d, 1.0)
    kw = dict(m=5, maxit=100, factr=1e7, pgtol=0.0, max_backtracks=30)
    kw.update(opts)
    st = design._Start(x0, lo, hi, **kw)
    state = api.fit_begin(x0, lo, hi, kw["maxit"], kw["factr"], kw["pgtol"], kw["max_backtracks"])
    assert state.shape == (api.fit_state_doubles(d),) and state[0] == d
    t = 0
    while st.running:
        assert t < 5000
        assert api.fit_trial(state).tobytes() == st.trial.tobytes(), (d, t)
        f, g, ok = fn(st.trial.copy(), t)
        had_pairs, bt, t_before = len(st.S), getattr(st, "backtracks", 0), getattr(st, "t", None)
        first = st.first
        st.feed(f, g, ok)
        code = api.fit_feed(state, f, g, ok)
        t += 1
        assert code == code_of(st) == int(state[api.FIT_CODE]), (d, t, st.message)
        assert int(state[api.FIT_ITERATIONS]) == st.iterations and int(state[api.FIT_EVALS]) == t
        assert float(state[api.FIT_F]).hex() == float(st.f).hex(), (d, t)
        assert api.fit_x(state).tobytes() == st.x.tobytes(), (d, t)
        # which branch _Start took
        if not first and st.running and getattr(st, "backtracks", 0) == bt + 1:
            usable = ok and math.isfinite(f)
            seen["interpolated" if usable else "halved"] += 1
            if usable and st.t not in (0.1 * t_before, 0.5 * t_before):
                seen["interior_interpolation"] += 1
        if not first and had_pairs and not st.S and st.running and st.backtracks == 0 and st.iterations == int(state[5]):
            seen["memory_reset"] += 1
    seen["code%d" % code_of(st)] += 1
    seen["at_lo"] += int(np.any(st.x == lo))
    seen["at_hi"] += int(np.any(st.x == hi))
    seen["evaluations"] += t
    # a stopped state takes no further step
    before = state.copy()
    assert api.fit_feed(state, 0.0, np.zeros(d), True) == code_of(st) and state.tobytes() == before.tobytes()


@pytest.mark.parametrize("d", DIMS)
def test_stepper_is_design_start(d):
    from collections import Counter
    seen = Counter()
    for name, fn, opts in CASES:
        run_case(d, fn, opts, seen)
    for branch in ["interpolated", "interior_interpolation", "halved", "memory_reset", "at_lo", "at_hi", "code1", "code2",
                   "code3", "code4", "code5"]:
        assert seen[branch] > 0, (d, branch, dict(seen))


def test_state_arguments():
    L = api.lib()
    state = api.fit_begin(np.zeros(3), -1.0, 1.0)
    g = np.zeros(3)
    assert L.ccgp_fit_feed(api._p(state), 4, 0.0, api._p(g), 1) == -1      # the state was begun with d = 3
    assert L.ccgp_fit_feed(None, 3, 0.0, api._p(g), 1) == -1
    assert L.ccgp_fit_begin(api._p(state), 65, api._p(g), api._p(g), api._p(g), 100, 1e7, 0.0, 30) == -1
    assert L.ccgp_fit_begin(api._p(state), 3, None, api._p(g), api._p(g), 100, 1e7, 0.0, 30) == -1
    assert L.ccgp_fit_state_doubles(0) == -1 and L.ccgp_fit_state_doubles(65) == -1
    assert [api.fit_state_doubles(d) for d in (1, 9, 64)] == [32, 160, 1040]
    # the start is clipped into its box
    s = api.fit_begin([-3.0, 0.5, 7.0], -1.0, [1.0, 1.0, 2.0])
    assert api.fit_trial(s).tolist() == [-1.0, 0.5, 2.0] and api.fit_x(s).tolist() == [-1.0, 0.5, 2.0]


def test_portable_exp_on_the_fit_box():
    """theta = chain_exp(log theta) within 2 ulp of exp on [-12, 12] (chain_terms.h's band for its exp-derived entries)."""
    mp.mp.dps = 40
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-12.0, 12.0, size=2000), [-12.0, 12.0, 0.0, 1e-300, -1e-17, 2.0 ** -30]])
    rows, _, _ = api.chain_terms(api.PRIOR_GV, 1, np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1))
    worst = 0.0
    for xi, got in zip(x, rows[:, 2]):
        want = mp.exp(mp.mpf(float(xi)))
        err = abs(mp.mpf(float(got)) - want) / mp.mpf(math.ulp(float(want)))
        worst = max(worst, float(err))
    print("chain_exp on [-12, 12]: worst error %.3f ulp" % worst)
    assert worst <= 2.0
