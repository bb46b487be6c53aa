"""design.minimize_starts_device's driver without a GPU: the twin path (on_device=False) over design_ref's numpy evaluator, every
step through the library's own stepper (ccgp_fit_begin / ccgp_fit_feed, which need no device), against design.minimize_starts
over the same evaluator.  The iterate is the design, so nothing lies between stepper and evaluator and the two must agree bit
for bit in every key but `calls`: for the two batch-sequential problems (Entropy.optim(14, 2, .., 20) and Batch.Entropy.optim
(D0, 7, 2, .., 25) at the prior medians) and for a run with a start on a coincident pair (code 5: the start itself cannot be
evaluated).  Also: the cut into segments changes nothing, a handle that says CCGP_EUNSUPPORTED sends the driver to the twin,
a stand-in launch restated on the host gives the same states, and rsurface reaches the driver with on_device=True only."""
import numpy as np
import pytest

from ccgp_amd import api, design
from design_ref import BSQ_PRIOR, initial_me_design, numpy_evaluator, params_row

KEYS = ("x", "f", "converged", "iterations", "calls_per_start")


def _same(got, want):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.tobytes() == b.tobytes(), k
    assert got["message"] == want["message"]


def _problems():
    D0 = initial_me_design()
    first = (numpy_evaluator(*BSQ_PRIOR), design.make_starts(20, 14, 2, 0))
    second = (numpy_evaluator(*BSQ_PRIOR, D_old=D0), design.make_starts(25, 7, 2, 0))
    S = design.make_starts(3, 14, 2, 0)
    S[1, 3] = S[1, 4]   # two coincident rows: R is singular
    return dict(first=first, second=second, coincident=(numpy_evaluator(*BSQ_PRIOR), S))


@pytest.fixture(scope="module")
def reference():
    return {k: design.minimize_starts(ev, S) for k, (ev, S) in _problems().items()}


@pytest.mark.parametrize("name", ["first", "second", "coincident"])
def test_twin_equals_minimize_starts(name, reference):
    ev, S = _problems()[name]
    want = reference[name]
    got = design.minimize_starts_device(None, S, 2, params_row(*BSQ_PRIOR, 2), on_device=False, evaluate=ev)
    _same(got, want)
    assert got["calls"] == want["calls"]   # on the twin every call carries every running start, as minimize_starts' do
    if name == "coincident":
        assert got["message"][1] == "the start itself cannot be evaluated" and np.isinf(got["f"][1])
        assert np.isfinite(got["f"][[0, 2]]).all()


def test_segments_and_options_change_nothing(reference):
    ev, S = _problems()["second"]
    row = params_row(*BSQ_PRIOR, 2)
    for seg in (1, 7):
        _same(design.minimize_starts_device(None, S, 2, row, on_device=False, evaluate=ev, seg=seg), reference["second"])
    opts = dict(maxit=6, factr=1e4, max_backtracks=3, lower=-0.9, upper=0.8)
    want = design.minimize_starts(ev, S, **opts)
    _same(design.minimize_starts_device(None, S, 2, row, on_device=False, evaluate=ev, **opts), want)
    assert (want["iterations"] <= 6).all() and "NEW_X: maxit reached" in want["message"]
    with pytest.raises(ValueError):
        design.minimize_starts_device(None, S, 2, row, on_device=False, evaluate=ev, seg=0)


class StandIn:
    """A handle whose design_fit is the launch restated on the host and whose design_fit_eval is the numpy evaluator."""

    def __init__(self, ev, device=True):
        self.ev, self.device = ev, device
        self.launches, self.eval_calls, self.refused = 0, 0, 0

    def design_fit_eval(self, x, K, params_row, D_old=None, ld_offset=0.0):
        self.eval_calls += 1
        return self.ev(np.asarray(x))

    def design_fit(self, n_free, d, K, params_row, state, max_evals, D_old=None, ld_offset=0.0, trace=False, T=None):
        if not self.device:
            self.refused += 1
            raise api.CcgpError(-4, "the stand-in has no device search")
        self.launches += 1
        state = np.array(state, dtype=np.float64)
        A = state.shape[0]
        max_evals = np.broadcast_to(np.asarray(max_evals), (A,))
        evals = np.zeros(A, dtype=np.int32)
        for a in range(A):
            while evals[a] < max_evals[a] and state[a, api.FIT_CODE] == api.FIT_RUNNING:
                f, g, st = self.ev(api.fit_trial(state[a]).reshape(1, n_free, d))
                api.fit_feed(state[a], f[0], g[0].ravel(), st[0] == 0)
                evals[a] += 1
        return dict(state=state, evals=evals, failed=0)


def test_launches_fallback_and_calls(reference):
    ev, S = _problems()["first"]
    row = params_row(*BSQ_PRIOR, 2)
    longest = int(reference["first"]["calls_per_start"].max())
    h = StandIn(ev)
    got = design.minimize_starts_device(h, S, 2, row, seg=16)
    _same(got, reference["first"])
    assert got["calls"] == h.launches == -(-longest // 16) and h.eval_calls == 0
    h = StandIn(ev, device=False)
    got = design.minimize_starts_device(h, S, 2, row)
    _same(got, reference["first"])
    assert h.refused == 1 and h.launches == 0 and got["calls"] == h.eval_calls == reference["first"]["calls"]


def test_more_than_64_variables_run_minimize_starts():
    ev = numpy_evaluator(*BSQ_PRIOR)
    S = design.make_starts(2, 33, 2, 3)
    want = design.minimize_starts(ev, S, maxit=3)
    got = design.minimize_starts_device(StandIn(ev), S, 2, params_row(*BSQ_PRIOR, 2), maxit=3)
    _same(got, want)


def test_rsurface_reaches_the_driver_with_on_device_only(monkeypatch):
    from ccgp_amd.rsurface import CombinedGP

    seen = []
    real = design.minimize_starts_device

    def spy(handle, starts, K, row, D_old=None, ld_offset=0.0, **kw):
        seen.append((np.asarray(starts).shape, D_old is not None, float(ld_offset), dict(kw)))
        return real(handle, starts, K, row, D_old, ld_offset, **kw)

    monkeypatch.setattr(design, "minimize_starts_device", spy)
    D0 = initial_me_design()
    ld_old = -numpy_evaluator(*BSQ_PRIOR)(D0[None])[0][0]

    class H(StandIn):
        def mixed_logdet_designs(self, designs, K, row):
            return np.array([ld_old]), np.zeros(1, dtype=np.int32)

        def mixed_logdet_grad_designs(self, designs, K, row, n_fixed=0):
            f, g, st = self.ev(np.asarray(designs)[:, n_fixed:])
            return -f + (ld_old if n_fixed else 0.0), -g, st

    gp = CombinedGP("HX", handle=H(numpy_evaluator(*BSQ_PRIOR)))
    S = design.make_starts(3, 14, 2, 0)
    base = gp.Entropy_optim(14, 2, *BSQ_PRIOR, 3, starts=S, maxit=4)
    assert not seen
    dev = gp.Entropy_optim(14, 2, *BSQ_PRIOR, 3, starts=S, maxit=4, on_device=True)
    assert len(seen) == 1 and seen[0][:3] == ((3, 14, 2), False, 0.0) and seen[0][3] == dict(maxit=4)
    for k in base:
        if k != "device_calls":
            assert np.asarray(base[k]).tobytes() == np.asarray(dev[k]).tobytes(), k
    gp.Entropy_optim(14, 2, *BSQ_PRIOR, 3, starts=S, maxit=2, m=3, on_device=True)   # another memory keeps the host path
    assert len(seen) == 1
    gp2 = CombinedGP("HX", handle=H(numpy_evaluator(*BSQ_PRIOR, D_old=D0)))
    S2 = design.make_starts(2, 7, 2, 0)
    gp2.Batch_Entropy_optim(D0, 7, 2, *BSQ_PRIOR, 2, starts=S2, maxit=2, on_device=True)
    assert len(seen) == 2 and seen[1][:3] == ((2, 7, 2), True, float(ld_old))
