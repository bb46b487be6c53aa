"""cgp.refine_starts_device's driver without a GPU: a handle whose cgp_fit_sets says CCGP_EUNSUPPORTED sends the driver to the
twin -- every evaluation through cgp_fit_eval_sets (here numpy's central differences over tests/cgp_ref.NumpyHandle), every step
through the library's own stepper (ccgp_fit_begin / ccgp_fit_feed, which need no device) -- and the result must equal
design.minimize_starts over the same evaluator in every key, on n = 5, d = 1 and n = 14, d = 2.  Also: the cut into segments
changes nothing, a stand-in launch restated on the host gives the same states with fewer calls, and cgp.CGP(on_device=True)
returns cgp.CGP()'s fields."""
import numpy as np
import pytest

import cgp_ref
from ccgp_amd import api, cgp, design

KEYS = ("x", "f", "converged", "iterations", "calls_per_start")
SHAPES = [(5, 1), (14, 2)]
STEP = 1e-5


def _same(got, want):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.tobytes() == b.tobytes(), k
    assert got["message"] == want["message"]


class Fake(cgp_ref.NumpyHandle):
    """NumpyHandle plus the two entry points of the refinement: cgp_fit_eval_sets is cgp._fit_sets.evaluate's arithmetic over
    cgp_state_batch; cgp_fit_sets refuses (device=False) or restates the launch on the host."""

    def __init__(self, device=False):
        super().__init__()
        self.device = device
        self.refused, self.launches, self.eval_calls = 0, 0, 0

    def cgp_fit_eval_sets(self, Xs, ys, w, lower, upper, step, set_of):
        self.eval_calls += 1
        W = np.atleast_2d(np.asarray(w, dtype=np.float64))
        k, P = W.shape
        lower, upper = np.broadcast_to(lower, (k, P)), np.broadcast_to(upper, (k, P))
        hi = np.minimum(W + step, upper)
        lo = np.maximum(W - step, lower)
        pts = np.repeat(W[:, None, :], 1 + 2 * P, axis=1)
        for j in range(P):
            pts[:, 1 + 2 * j, j] = hi[:, j]
            pts[:, 2 + 2 * j, j] = lo[:, j]
        f, st = np.empty((k, 1 + 2 * P)), np.empty((k, 1 + 2 * P), dtype=np.int32)
        for b in range(k):
            c = int(np.asarray(set_of)[b])
            val, _, _, _, s = self.cgp_state_batch(Xs[c], ys[c], cgp.rows_from_ww(pts[b]))
            f[b], st[b] = np.where(np.isfinite(val), val, cgp.NONFINITE), s
        return f[:, 0], (f[:, 1::2] - f[:, 2::2]) / (hi - lo), st[:, 0]

    def cgp_fit_sets(self, Xs, ys, set_of, state, step, max_evals, look=16, trace=False, T=None):
        if not self.device:
            self.refused += 1
            raise api.CcgpError(-4, "the stand-in has no device refinement")
        self.launches += 1
        state = np.array(state, dtype=np.float64)
        A = state.shape[0]
        P = (state.shape[1] - api.FIT_HEADER) // 16
        max_evals = np.broadcast_to(np.asarray(max_evals), (A,))
        evals = np.zeros(A, dtype=np.int32)
        for a in range(A):
            lo, hi = state[a, api.FIT_HEADER + 4 * P:][:P].copy(), state[a, api.FIT_HEADER + 5 * P:][:P].copy()
            while evals[a] < max_evals[a] and state[a, api.FIT_CODE] == api.FIT_RUNNING:
                f, g, st = self.cgp_fit_eval_sets(Xs, ys, api.fit_trial(state[a])[None], lo[None], hi[None], step, [set_of[a]])
                api.fit_feed(state[a], f[0], g[0], st[0] == 0)
                evals[a] += 1
        return dict(state=state, evals=evals, failed=0)


def _problem(n, d, C=2, S=2):
    """C seeded sets of one shape, S starts per set from a seeded hypercube in the set's own box, as CGP takes them."""
    rng = np.random.default_rng(100 * n + d)
    Xs = np.stack([cgp.standardise(rng.random((n, d)))[0] for _ in range(C)])
    ys = np.stack([np.sin(3.0 * X.sum(axis=1)) + 0.3 * X[:, 0] ** 2 + 0.05 * rng.standard_normal(n) for X in Xs])
    box = [cgp.bounds(X) for X in Xs]
    starts = np.concatenate([box[c][0] + cgp.lhd(S, d + 3, rng) * (box[c][1] - box[c][0]) for c in range(C)])
    owner = np.repeat(np.arange(C), S)
    lowers, uppers = np.stack([box[c][0] for c in owner]), np.stack([box[c][1] for c in owner])
    return Xs, ys, starts, lowers, uppers, owner


def _lockstep(h, Xs, ys, lowers, uppers, owner):
    def evaluate(W, live):
        return h.cgp_fit_eval_sets(Xs, ys, W, lowers[live], uppers[live], STEP, owner[live])
    return evaluate


@pytest.fixture(scope="module")
def reference():
    out = {}
    for n, d in SHAPES:
        Xs, ys, starts, lowers, uppers, owner = _problem(n, d)
        out[n, d] = design.minimize_starts(_lockstep(Fake(), Xs, ys, lowers, uppers, owner), starts, lowers=lowers, uppers=uppers,
                                           pass_live=True, maxit=6)
    return out


@pytest.mark.parametrize("n,d", SHAPES)
def test_refused_call_runs_the_twin(n, d, reference):
    Xs, ys, starts, lowers, uppers, owner = _problem(n, d)
    want = reference[n, d]
    h = Fake()
    got = cgp.refine_starts_device(h, Xs, ys, starts, lowers, uppers, owner, STEP, maxit=6)
    _same(got, want)
    assert h.refused == 1 and got["calls"] == h.eval_calls == want["calls"]   # every twin call carries every running start
    assert (want["calls_per_start"] > 1).all() and np.isfinite(want["f"]).all()


def test_segments_look_and_launch_change_nothing(reference):
    n, d = SHAPES[0]
    Xs, ys, starts, lowers, uppers, owner = _problem(n, d)
    want = reference[n, d]
    for seg in (1, 7):
        _same(cgp.refine_starts_device(Fake(), Xs, ys, starts, lowers, uppers, owner, STEP, maxit=6, seg=seg), want)
    _same(cgp.refine_starts_device(Fake(), Xs, ys, starts, lowers, uppers, owner, STEP, maxit=6, on_device=False), want)
    h = Fake(device=True)
    got = cgp.refine_starts_device(h, Xs, ys, starts, lowers, uppers, owner, STEP, maxit=6, seg=16, look=1)
    _same(got, want)
    assert got["calls"] == h.launches == -(-int(want["calls_per_start"].max()) // 16) and h.refused == 0
    for bad in (dict(seg=0), dict(look=0), dict(look=65)):
        with pytest.raises(ValueError):
            cgp.refine_starts_device(Fake(), Xs, ys, starts, lowers, uppers, owner, STEP, **bad)


def test_cgp_on_device_returns_cgps_fields():
    rng = np.random.default_rng(3)
    X = rng.random((5, 1))
    y = np.sin(4.0 * X[:, 0]) + 0.02 * rng.standard_normal(5)
    want = cgp.CGP(cgp_ref.NumpyHandle(), X, y, num_starts=2)
    h = Fake()
    got = cgp.CGP(h, X, y, num_starts=2, on_device=True, look=4)
    assert h.refused == 1 and set(got) == set(want)
    for k in want:
        if k in ("calls", "refinement_calls", "seconds"):
            continue
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() and type(got[k]) is type(want[k]), k
    assert got["refinement_calls"] == want["refinement_calls"]   # on the twin a call still carries every running start
