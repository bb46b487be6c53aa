"""fit.ordinary_kriging_fit_device_sets' driver without a GPU, on a stand-in handle whose objective is a closed form
(host_handles.ClosedFormHandle's profile likelihood) and whose profile_fit_sets is the launch restated on the host with the
library's own stepper (ccgp_fit_begin / ccgp_fit_feed, which need no device).  What is held: a start is the plain sequential
loop written here, with the same bits whatever `seg` cuts it into, whether its set is fitted alone or among others, and whether
the steps run in the (stand-in) launch or on the twin; the C = 1 form is the sets form's one entry; a handle that says
CCGP_EUNSUPPORTED sends the driver to the twin; calls and evaluations are what the handle saw; fit.study reaches the driver
with device_fits=True only."""
import types

import numpy as np
import pytest

from ccgp_amd import api, fit
from host_handles import ClosedFormHandle


class FitHandle(ClosedFormHandle):
    """ClosedFormHandle with the two fit calls.  launches / eval_calls: calls made by a driver; points[c]: points evaluated
    on set c, by either call."""

    def __init__(self, device=True):
        super().__init__()
        self.device = device
        self.launches, self.eval_calls, self.refused = 0, 0, 0
        self.points = {}

    def _objective(self, Xs, ys, logtheta, set_of, grad):
        logtheta = np.atleast_2d(np.asarray(logtheta, dtype=np.float64))
        theta = np.exp(logtheta)
        rows = np.concatenate([np.ones((len(theta), 1)), theta], axis=1)
        self.inner = True
        try:
            ll, s2, beta, g, st = self.profile_batch_sets(Xs, ys, 1, rows, set_of, grad=grad)
        finally:
            self.inner = False
        for c in np.asarray(set_of):
            self.points[int(c)] = self.points.get(int(c), 0) + 1
        return -ll, (-(g[:, 1:] * theta) if grad else None), theta, s2, beta, st

    def profile_fit_eval_sets(self, Xs, ys, logtheta, set_of, grad=True):
        self.eval_calls += 1
        return self._objective(Xs, ys, logtheta, set_of, grad)

    def profile_fit_sets(self, Xs, ys, set_of, state, max_evals, trace=False, T=None):
        if not self.device:
            self.refused += 1
            raise api.CcgpError(-4, "the stand-in has no device fit")
        self.launches += 1
        state = np.array(state, dtype=np.float64)
        A = state.shape[0]
        max_evals = np.broadcast_to(np.asarray(max_evals), (A,))
        evals = np.zeros(A, dtype=np.int32)
        for a in range(A):
            while evals[a] < max_evals[a] and state[a, api.FIT_CODE] == api.FIT_RUNNING:
                f, g, _, _, _, st = self._objective(Xs, ys, api.fit_trial(state[a])[None], [set_of[a]], True)
                api.fit_feed(state[a], f[0], g[0], st[0] == 0)
                evals[a] += 1
        return dict(state=state, evals=evals, failed=0)


def make_sets(C, n=6, d=3):
    rng = np.random.default_rng(11)
    return [rng.random((n, d)) for _ in range(C)], [rng.standard_normal(n) + c for c in range(C)]


def sequential(D, y, rng_seed, starts=4):
    """Every start of one set as the contract states it: one evaluation, one step, until the start stops."""
    h = FitHandle()
    x0 = fit.kriging_starts(D, starts, rng_seed)
    out, evaluations = [], 0
    for x in x0:
        state = api.fit_begin(x, -12.0, 12.0)
        while state[api.FIT_CODE] == api.FIT_RUNNING:
            f, g, _, _, _, st = h.profile_fit_eval_sets(D[None], y[None], api.fit_trial(state)[None], [0])
            api.fit_feed(state, f[0], g[0], st[0] == 0)
            evaluations += 1
        out.append(state)
    return np.stack(out), evaluations


def same(fa, fb, skip=()):
    assert sorted(fa) == sorted(fb)
    for k in fa:
        if k not in skip:
            np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)


@pytest.mark.parametrize("seg", [1, 7, 512])
@pytest.mark.parametrize("C", [1, 3])
def test_twin_driver_is_the_sequential_loop(seg, C):
    Ds, ys = make_sets(3)
    h = FitHandle()
    fits = fit.ordinary_kriging_fit_device_sets(h, Ds[:C], ys[:C], starts=4, rng=3, on_device=False, seg=seg)
    assert h.launches == 0 and len(fits) == C
    for c in range(C):
        states, evaluations = sequential(Ds[c], ys[c], 3)
        np.testing.assert_array_equal(fits[c]["x"], api.fit_x(states))
        np.testing.assert_array_equal(fits[c]["f"], states[:, api.FIT_F])
        code = states[:, api.FIT_CODE]
        np.testing.assert_array_equal(fits[c]["converged"], (code == 1) | (code == 2))
        assert fits[c]["converged"].all()
        assert fits[c]["evaluations"] == evaluations + 1 == h.points[c]
        best = int(np.argmin(states[:, api.FIT_F]))
        np.testing.assert_array_equal(fits[c]["theta"], np.exp(api.fit_x(states)[best]))
        assert fits[c]["loglik"] == -states[best, api.FIT_F]
        # the optimum of the closed form: log theta = 0.5 + 0.1 mean(y)
        np.testing.assert_allclose(np.log(fits[c]["theta"]), 0.5 + 0.1 * ys[c].mean(), atol=1e-5)
    # every step carried every running start: the calls of the group are those of its slowest start, the final one besides
    assert h.eval_calls == max(f["calls"] for f in fits)


@pytest.mark.parametrize("seg", [1, 7, 512])
def test_launch_and_twin_leave_the_same_fits(seg):
    Ds, ys = make_sets(3)
    hd, ht = FitHandle(), FitHandle()
    dev = fit.ordinary_kriging_fit_device_sets(hd, Ds, ys, starts=4, rng=[1, 2, 3], seg=seg)
    twin = fit.ordinary_kriging_fit_device_sets(ht, Ds, ys, starts=4, rng=[1, 2, 3], on_device=False, seg=seg)
    for c in range(3):
        same(dev[c], twin[c], skip=("calls",))
        assert dev[c]["evaluations"] == hd.points[c] == ht.points[c]
    # calls = launches + 1, and a set stops being launched once its starts have stopped
    assert max(f["calls"] for f in dev) == hd.launches + 1 and hd.eval_calls == 1
    longest = max(int(f["evaluations"]) for f in dev)
    assert hd.launches <= -(-longest // seg) + 1


def test_one_set_is_the_sets_form_field_for_field():
    Ds, ys = make_sets(1)
    one = fit.ordinary_kriging_fit_device(FitHandle(), Ds[0], ys[0], starts=3, rng=5, extra_starts=[[0.7, 1.1, 2.0]])
    many = fit.ordinary_kriging_fit_device_sets(FitHandle(), Ds, ys, starts=3, rng=5, extra_starts=[[0.7, 1.1, 2.0]])
    same(one, many[0])
    assert one["x"].shape == (4, 3) and one["f"].shape == (4,)
    lock = fit.ordinary_kriging_fit_sets(FitHandle(), Ds, ys, starts=3, rng=5, extra_starts=[[0.7, 1.1, 2.0]])
    assert sorted(one) == sorted(lock[0])            # ordinary_kriging_fit_sets' keys


def test_unsupported_falls_back_to_the_twin():
    Ds, ys = make_sets(2)
    h = FitHandle(device=False)
    got = fit.ordinary_kriging_fit_device_sets(h, Ds, ys, starts=4, rng=3)
    assert h.refused == 1 and h.launches == 0 and h.eval_calls > 1
    want = fit.ordinary_kriging_fit_device_sets(FitHandle(), Ds, ys, starts=4, rng=3, on_device=False)
    for c in range(2):
        same(got[c], want[c])

    class Broken(FitHandle):
        def profile_fit_sets(self, *a, **k):
            raise api.CcgpError(-3, "a device error is not a refusal")
    with pytest.raises(api.CcgpError):
        fit.ordinary_kriging_fit_device_sets(Broken(), Ds, ys)


def test_driver_refuses_bad_arguments():
    Ds, ys = make_sets(2)
    for bad in (dict(seg=0), dict(seg=4097), dict(rng=[1, 2, 3])):
        with pytest.raises(ValueError):
            fit.ordinary_kriging_fit_device_sets(FitHandle(), Ds, ys, **bad)
    with pytest.raises(ValueError):
        fit.ordinary_kriging_fit_device_sets(FitHandle(), [Ds[0], Ds[1][:4]], ys)


def test_study_reaches_the_driver_only_when_asked(monkeypatch):
    class Reached(Exception):
        pass

    def stop(name):
        def fn(*a, **k):
            raise Reached(name)
        return fn
    monkeypatch.setattr(fit, "ordinary_kriging_fit_device_sets", stop("device_sets"))
    monkeypatch.setattr(fit, "ordinary_kriging_fit_device", stop("device"))
    monkeypatch.setattr(fit, "ordinary_kriging_fit_sets", stop("lockstep"))
    monkeypatch.setattr(fit, "ordinary_kriging_fit", stop("single"))
    Ds, ys = make_sets(2)
    sets = [(D, y, D[:2], y[:2]) for D, y in zip(Ds, ys)]
    gp = types.SimpleNamespace(h=object())
    for kw, want in ((dict(), "lockstep"), (dict(device_fits=True), "device_sets"), (dict(lockstep_fits=False), "single"),
                     (dict(lockstep_fits=False, device_fits=True), "device")):
        with pytest.raises(Reached) as e:
            fit.study(gp, sets, 0.05, 10, 5, 5, 0.5, **kw)
        assert str(e.value) == want
