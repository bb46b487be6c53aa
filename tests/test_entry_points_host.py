"""The single-set routines of the host layers and their sets forms: fit.ordinary_kriging_fit and cgp.CGP share one routine
each with their sets form and differ in the evaluator they hand it; fit.Metro and fit.Metro_sets share _Chain.  Held here, without a GPU, on a stand-in handle that
records every method called and with how many rows (host_handles.ClosedFormHandle):

  * a single-set routine calls the single-set methods only, a sets routine the sets methods only (plus cgp_predict);
  * the calls a result reports are the calls the handle saw;
  * with C = 1 the sets routine returns the single-set routine's result, field for field with equal bytes, and leaves the
    generator in the same state;
  * leave_one_out takes a fitted single-GP model as dict(est=...) like compare_GP does.

n = 8, d = 2 throughout; the objectives are closed forms, so a fit is a few dozen calls."""
import numpy as np
import pytest

from conftest import synthetic_design
from host_handles import ClosedFormHandle
from ccgp_amd import api, cgp, fit

N, SAMP, BATCH, ALPHA = 40, 20, 10, 0.05
START = np.array([0.2, 0.1, -0.1])


class _GP:
    """What fit needs of a CombinedGP: the handle, the script and its prior id, and leave_one_out's table."""
    script, cfg = "GV", dict(prior=api.PRIOR_GV, npar=3)

    def __init__(self):
        self.h = ClosedFormHandle()

    def leave_one_out(self, alpha, draws, D_train, sigma2, y_train):
        y = np.asarray(y_train, dtype=np.float64).ravel()
        return dict(y_hat=0.9 * y, Quant=np.full(y.size, 0.5), LL=y - 1.0, UL=y + 1.0, pit=np.full(y.size, 0.5))


@pytest.fixture(scope="module")
def two_sets():
    return [synthetic_design(8, 2, 90), synthetic_design(8, 2, 91)]


def _same(got, want, skip=()):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in skip:
            continue
        if isinstance(want[k], dict):
            _same(got[k], want[k])
        elif isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        else:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], k


def _methods(h):
    return {name for name, _ in h.log}


@pytest.mark.parametrize("speculate", [0, 3])
def test_metro_and_metro_sets(two_sets, speculate):
    (X, y), _ = two_sets
    gp = _GP()
    rng = np.random.default_rng(5)
    one = fit.Metro(gp, START, N, SAMP, BATCH, ALPHA, X, 1.5, y, rng=rng, speculate=speculate)
    assert _methods(gp.h) == {"logpost_batch"}
    # the Laplace stage alone, on the same evaluator, makes the calls Metro made before its chain; one more for the mode
    lap = ClosedFormHandle()
    fit.laplace(lambda rows: lap.logpost_batch(X, y, 1.5, api.PRIOR_GV, rows)[0], START)
    assert len(gp.h.log) == len(lap.log) + 1 + one["device_batches"]
    per = (1 << speculate) - 1 if speculate else 1
    assert [r for _, r in gp.h.log[len(lap.log) + 1:]] == [per] * one["device_batches"]

    gs = _GP()
    rng1 = np.random.default_rng(5)
    sets = fit.Metro_sets(gs, None, N, SAMP, BATCH, ALPHA, [X], [1.5], [y], rngs=[rng1], speculate=speculate,
                          laplace=[one["laplace"]])
    assert _methods(gs.h) == {"logpost_sets"}
    assert sets["laplace_calls"] == 0 and len(gs.h.log) == 1 + sets["device_batches"]
    _same(sets["chains"][0], one)
    assert rng1.bit_generator.state == rng.bit_generator.state

    g2 = _GP()
    both = fit.Metro_sets(g2, np.stack([START, START]), N, SAMP, BATCH, ALPHA, [s[0] for s in two_sets], [1.5, 0.7],
                          [s[1] for s in two_sets], rngs=[5, 6], speculate=speculate)
    assert _methods(g2.h) == {"logpost_sets"}
    assert len(g2.h.log) == both["laplace_calls"] + 1 + both["device_batches"]
    assert both["device_batches"] == max(ch["device_batches"] for ch in both["chains"])


def test_ordinary_kriging_fit_and_its_sets_form(two_sets):
    (X, y), _ = two_sets
    h = ClosedFormHandle()
    one = fit.ordinary_kriging_fit(h, X, y, starts=2, rng=3)
    assert _methods(h) == {"profile_batch"}
    assert len(h.log) == one["calls"] and sum(r for _, r in h.log) == one["evaluations"]
    hs = ClosedFormHandle()
    sets = fit.ordinary_kriging_fit_sets(hs, [X], [y], starts=2, rng=3)
    assert _methods(hs) == {"profile_batch_sets"}
    assert len(hs.log) == sets[0]["calls"] and sum(r for _, r in hs.log) == sets[0]["evaluations"]
    _same(sets[0], one)
    h2 = ClosedFormHandle()
    both = fit.ordinary_kriging_fit_sets(h2, [s[0] for s in two_sets], [s[1] for s in two_sets], starts=2, rng=3)
    assert _methods(h2) == {"profile_batch_sets"}
    assert len(h2.log) == max(f["calls"] for f in both) and sum(r for _, r in h2.log) == sum(f["evaluations"] for f in both)
    _same(both[0], one)


def test_cgp_and_cgp_sets(two_sets):
    (X, y), _ = two_sets
    h = ClosedFormHandle()
    one = cgp.CGP(h, X, y, num_starts=2, rng=4)
    assert _methods(h) == {"cgp_state_batch", "cgp_predict"}
    assert len(h.log) == one["calls"] and sum(r for _, r in h.log) == one["evaluations"]
    assert h.calls["cgp_state_batch"] == 1 + one["refinement_calls"] + 1 and h.calls["cgp_predict"] == 1
    hs = ClosedFormHandle()
    sets = cgp.CGP_sets(hs, [X], [y], num_starts=2, rngs=[4])
    assert _methods(hs) == {"cgp_state_batch_sets", "cgp_predict"}
    assert len(hs.log) == sets[0]["calls"] and sum(r for _, r in hs.log) == sets[0]["evaluations"]
    _same(sets[0], one, skip=("seconds",))   # host clock
    h2 = ClosedFormHandle()
    both = cgp.CGP_sets(h2, [s[0] for s in two_sets], [s[1] for s in two_sets], num_starts=2, rngs=[4, 4])
    assert _methods(h2) == {"cgp_state_batch_sets", "cgp_predict"}
    assert len(h2.log) == both[0]["calls"] and sum(r for _, r in h2.log) == sum(e["evaluations"] for e in both)
    _same(both[0], one, skip=("seconds", "calls", "refinement_calls"))   # the group's calls: those of its slowest set


def test_leave_one_out_takes_a_fitted_single_model(two_sets):
    (X, y), _ = two_sets
    gp = _GP()
    est = fit.ordinary_kriging_fit(gp.h, X, y, starts=2, rng=3)
    seen = len(gp.h.log)
    by_est = fit.leave_one_out(gp, 0.1, None, X, 1.0, y, single=dict(est=est))
    by_pars = fit.leave_one_out(gp, 0.1, None, X, 1.0, y, single=dict(theta=est["theta"], sigma2=est["sigma2"]))
    assert gp.h.log[seen:] == [("loo_batch", 1)] * 2   # nothing is fitted
    assert by_est["single"] is est
    _same(by_est, by_pars, skip=("single",))
