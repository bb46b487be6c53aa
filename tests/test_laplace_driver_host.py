"""fit.laplace_device_sets' driver without a GPU, on a stand-in handle whose log-posterior is a closed form of the point and of
the set (one set has a band where it cannot be evaluated, so its search shrinks) and whose laplace_search_sets is the launch
restated on the host with the library's own stepper (ccgp_nm_begin / ccgp_nm_feed, which need no device).  What is held: the
driver's estimates equal fit.laplace_sets' over the same evaluator in every key, whatever `seg` cuts the search into, whether
a set is searched alone or among others, and whether the steps run in the (stand-in) launch or on the twin; the C = 1 form is
the sets form's one entry; a handle that says CCGP_EUNSUPPORTED sends the driver to the twin; fit.study reaches the driver
with device_laplace=True only."""
import types

import numpy as np
import pytest

from ccgp_amd import api, fit


class SearchHandle:
    """chain_logpost_sets as a closed form, laplace_search_sets as the launch on the host.  launches / eval_calls: calls made
    by a driver; points[c]: points evaluated on set c by a launch."""

    def __init__(self, device=True):
        self.device = device
        self.launches, self.eval_calls, self.refused = 0, 0, 0
        self.points = {}

    @staticmethod
    def _value(Xs, ys, sigma2s, theta_t, set_of):
        T = np.atleast_2d(np.asarray(theta_t, dtype=np.float64))
        c = np.asarray(set_of, dtype=np.int64)
        m = np.asarray(ys, dtype=np.float64).mean(axis=1)[c]
        centre = 0.5 + 0.1 * m[:, None] * np.arange(1, T.shape[1] + 1)
        val = 2.0 * T[:, 0] - 0.1 * T[:, 0] ** 4 - ((T[:, 1:] - centre[:, 1:]) ** 2).sum(axis=1) - 0.5 * np.log(np.asarray(sigma2s)[c])
        band = (c == 1) & (T[:, 0] > 1.003) & (T[:, 0] < 1.045)
        return np.where(band, np.nan, val), m + T[:, 0]

    def chain_logpost_sets(self, Xs, ys, sigma2s, prior_id, theta_t, set_of, prior_pars=None):
        self.eval_calls += 1
        val, beta = self._value(Xs, ys, sigma2s, theta_t, set_of)
        return val, beta, val, np.zeros(len(val), dtype=np.int32)

    def laplace_search_sets(self, Xs, ys, sigma2s, prior_id, set_of, state, max_evals, prior_pars=None, trace=False, T=None):
        if not self.device:
            self.refused += 1
            raise api.CcgpError(-4, "the stand-in has no device search")
        self.launches += 1
        state = np.array(state, dtype=np.float64)
        A = state.shape[0]
        max_evals = np.broadcast_to(np.asarray(max_evals), (A,))
        evals = np.zeros(A, dtype=np.int32)
        for a in range(A):
            while evals[a] < max_evals[a] and state[a, api.NM_CODE] == api.NM_RUNNING:
                val = self._value(Xs, ys, sigma2s, api.nm_trial(state[a])[None], [set_of[a]])[0]
                api.nm_feed(state[a], val[0])
                evals[a] += 1
                self.points[int(set_of[a])] = self.points.get(int(set_of[a]), 0) + 1
        return dict(state=state, evals=evals, failed=0)


def make_gp(device=True):
    return types.SimpleNamespace(h=SearchHandle(device), cfg=dict(prior=api.PRIOR_GV, npar=3), script="GV")


def make_sets(C, n=6, d=3):
    rng = np.random.default_rng(11)
    Ds = [rng.random((n, d)) for _ in range(C)]
    ys = [rng.standard_normal(n) + c for c in range(C)]
    return Ds, ys, [1.0 + 0.5 * c for c in range(C)]


STARTS = np.array([[1.0, 1.0, 0.0], [1.0, 0.4, 0.5], [0.3, 0.0, 2.0]])


def lockstep(Ds, ys, s2, starts, **kw):
    gp = make_gp()
    fn = fit._twin_sets_evaluator(gp, Ds, ys, s2, None, None)
    return fit.laplace_sets(lambda rows, set_of: fn(rows, set_of)[0], starts, **kw)


def same(fa, fb, skip=()):
    assert sorted(k for k in fa if k not in skip) == sorted(k for k in fb if k not in skip)
    for k in fb:
        if k not in skip:
            np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
            assert np.asarray(fa[k], dtype=np.float64).tobytes() == np.asarray(fb[k], dtype=np.float64).tobytes(), k


@pytest.fixture(scope="module")
def reference():
    Ds, ys, s2 = make_sets(3)
    return Ds, ys, s2, lockstep(Ds, ys, s2, STARTS)


@pytest.mark.parametrize("seg", [1, 7, 512])
@pytest.mark.parametrize("pick", [[0], [0, 1], [0, 1, 2]])
def test_twin_driver_is_laplace_sets(reference, seg, pick):
    Ds, ys, s2, want = reference
    gp = make_gp()
    got = fit.laplace_device_sets(gp, [Ds[c] for c in pick], [ys[c] for c in pick], [s2[c] for c in pick], STARTS[pick],
                                  on_device=False, seg=seg)
    assert gp.h.launches == 0 and len(got) == len(pick)
    for j, c in enumerate(pick):
        same(got[j], want[c], skip=("fed", "calls"))
        assert got[j]["converged"] and got[j]["fed"] < got[j]["evaluations"]
        assert got[j]["calls"] == got[j]["fed"] + 1
    # every step carried every running search, the Hessian's points are one call more
    assert gp.h.eval_calls == max(e["fed"] for e in got) + 1


def test_the_banded_set_shrinks(reference):
    Ds, ys, s2, want = reference
    state = api.nm_begin(STARTS[1])
    h = SearchHandle()
    while state[api.NM_CODE] == api.NM_RUNNING:
        api.nm_feed(state, h._value(np.stack(Ds), np.stack(ys), s2, api.nm_trial(state)[None], [1])[0][0])
    assert state[api.NM_COUNTERS["shrink"]] > 0
    assert want[1]["evaluations"] == 4 + 4 * want[1]["iterations"] + 3 * int(state[api.NM_COUNTERS["shrink"]])


@pytest.mark.parametrize("seg", [1, 7, 512])
def test_launch_and_twin_leave_the_same_estimates(reference, seg):
    Ds, ys, s2, want = reference
    gd, gt = make_gp(), make_gp()
    dev = fit.laplace_device_sets(gd, Ds, ys, s2, STARTS, seg=seg)
    twin = fit.laplace_device_sets(gt, Ds, ys, s2, STARTS, on_device=False, seg=seg)
    for c in range(3):
        same(dev[c], twin[c], skip=("calls",))
        same(dev[c], want[c], skip=("fed", "calls"))
        assert dev[c]["fed"] == gd.h.points[c]
        assert dev[c]["calls"] == -(-dev[c]["fed"] // seg) + 1   # a search leaves the launches once it has stopped
    assert gd.h.launches == max(e["calls"] for e in dev) - 1 and gd.h.eval_calls == 1


def test_maxiter_stops_where_laplace_sets_stops():
    Ds, ys, s2 = make_sets(3)
    want = lockstep(Ds, ys, s2, STARTS, maxiter=50)
    got = fit.laplace_device_sets(make_gp(), Ds, ys, s2, STARTS, maxiter=50, seg=7)
    for c in range(3):
        same(got[c], want[c], skip=("fed", "calls"))
        assert not got[c]["converged"] and got[c]["evaluations"] >= 50 > got[c]["iterations"]
    want = lockstep(Ds, ys, s2, STARTS, hess_step=1e-2)
    got = fit.laplace_device_sets(make_gp(), Ds, ys, s2, STARTS, hess_step=1e-2)
    for c in range(3):
        same(got[c], want[c], skip=("fed", "calls"))


def test_one_set_is_the_sets_form_field_for_field(reference):
    Ds, ys, s2, want = reference
    one = fit.laplace_device(make_gp(), Ds[0], ys[0], s2[0], STARTS[0])
    many = fit.laplace_device_sets(make_gp(), Ds[:1], ys[:1], s2[:1], STARTS[:1])
    same(one, many[0])
    same(one, want[0], skip=("fed", "calls"))
    assert sorted(set(one) - set(want[0])) == ["calls", "fed"]
    # an evaluator of the caller's keeps the search on the host
    gp = make_gp()
    fn = fit._twin_sets_evaluator(make_gp(), Ds[:1], ys[:1], s2[:1], None, None)
    own = fit.laplace_device(gp, Ds[0], ys[0], s2[0], STARTS[0], logpost_fn=lambda rows: fn(rows, np.zeros(len(rows), dtype=int)))
    same(own, one, skip=("calls",))
    assert gp.h.launches == 0 and gp.h.eval_calls == 0


def test_unsupported_falls_back_to_the_twin(reference):
    Ds, ys, s2, want = reference
    gp = make_gp(device=False)
    got = fit.laplace_device_sets(gp, Ds, ys, s2, STARTS)
    assert gp.h.refused == 1 and gp.h.launches == 0 and gp.h.eval_calls > 1
    for c in range(3):
        same(got[c], want[c], skip=("fed", "calls"))

    class Broken(SearchHandle):
        def laplace_search_sets(self, *a, **k):
            raise api.CcgpError(-3, "a device error is not a refusal")
    gp.h = Broken()
    with pytest.raises(api.CcgpError):
        fit.laplace_device_sets(gp, Ds, ys, s2, STARTS)


def test_driver_refuses_bad_arguments():
    Ds, ys, s2 = make_sets(2)
    for bad in (dict(seg=0), dict(seg=4097), dict(maxiter=-1)):
        with pytest.raises(ValueError):
            fit.laplace_device_sets(make_gp(), Ds, ys, s2, STARTS[:2], **bad)
    with pytest.raises(ValueError):
        fit.laplace_device_sets(make_gp(), Ds, ys, s2, STARTS)            # three starts for two sets
    with pytest.raises(ValueError):
        fit.laplace_device_sets(make_gp(), Ds, ys, s2[:1], STARTS[:2])
    with pytest.raises(ValueError):
        fit.laplace_device_sets(make_gp(), Ds, ys, s2, np.ones((2, 4)))   # the script has three parameters


def test_study_reaches_the_driver_only_when_asked(monkeypatch):
    class Reached(Exception):
        pass

    def stop(name):
        def fn(*a, **k):
            raise Reached(name)
        return fn
    monkeypatch.setattr(fit, "laplace_device_sets", stop("device"))
    monkeypatch.setattr(fit, "laplace_sets", stop("lockstep"))
    monkeypatch.setattr(fit, "Metro_device_sets", stop("chains"))
    Ds, ys, s2 = make_sets(2)
    sets = [(D, y, D[:2], y[:2]) for D, y in zip(Ds, ys)]
    gp = make_gp()
    for kw, want in ((dict(), "lockstep"), (dict(device_chains=True), "lockstep"), (dict(device_fits=True), "lockstep"),
                     (dict(device_laplace=True), "device"), (dict(device_laplace=True, device_chains=True), "device"),
                     (dict(device_laplace=True, laplace=[dict(), dict()], device_chains=True), "chains")):
        with pytest.raises(Reached) as e:
            fit.study(gp, sets, 0.05, 10, 5, 5, 0.5, sigma2s=s2, **kw)
        assert str(e.value) == want, kw
