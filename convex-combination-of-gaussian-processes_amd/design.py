"""Multi-start maximum-entropy design search (Entropy.optim / Batch.Entropy.optim, Batch Sequential ME Design.R:886-948).

The reference runs R's optim(method = "L-BFGS-B") from n.starts Latin-hypercube starts, one start after another, on
the criterion -det(R.mixed(D)) with finite-difference gradients: 2 n d + 1 criterion values per gradient, each a
separate evaluation.  Here the starts run side by side in LOCKSTEP: every call of `evaluate` carries the current
trial point of every start that is still running -- a first trial or a backtrack alike -- so one device launch serves
up to S designs, and the gradient is the analytic one (ccgp_mixed_logdet_grad_designs).

The objective is -log det R rather than the reference's -det R.  The two have the same argmin and the same stationary
points (log is increasing and det R > 0 wherever the criterion is defined), and -log det does not underflow: the Schur
determinant of a 7-point second batch at (p, theta1, theta2) = (0.5, 1, 4) is already 4.6e-4, and it shrinks as the
designs grow.

The method is a box-constrained limited-memory quasi-Newton iteration, per start:
  * active set: a variable at a bound whose gradient points out of the box is frozen for the iteration;
  * direction: the L-BFGS two-loop recursion over the free variables (memory m = 5), steepest descent on the free
    variables when the memory is empty or the quasi-Newton direction is not a descent direction;
  * step: a projected backtracking (Armijo) line search, x(t) = clip(x + t p, lower, upper), so every iterate lies
    inside the bounds exactly.  A trial the evaluator reports as failed (status != 0) or non-finite is infeasible:
    the line search backs off from it.
Stopping rules follow R's optim defaults for L-BFGS-B: maxit = 100 iterations, factr = 1e7 (stop when the relative
reduction of f in an iteration is <= factr * eps), pgtol = 0 (stop when the projected gradient is <= pgtol).

Every start's arithmetic is its own (1-D arrays, no reduction across starts), and the evaluator treats each design
independently, so the result for a start does not depend on which other starts share the calls.
"""
from __future__ import annotations

import numpy as np

_EPS = float(np.finfo(np.float64).eps)


def _dot(a, b):
    # numpy's pairwise sum: the same bits for the same operands wherever the arrays happen to sit in memory
    return float(np.add.reduce(a * b))


def latin_hypercube(n, d, rng):
    """A random Latin hypercube of n points in [0, 1]^d: each column has one point in each of the n strata.
    (The reference uses lhs::optimumLHS, an optimised LHS that cannot be reproduced without R.)"""
    u = rng.random((n, d))
    perm = np.stack([rng.permutation(n) for _ in range(d)], axis=1)
    return (perm + u) / n


class _Start:
    """State of one start: the current iterate, the L-BFGS memory and the line search in progress."""

    def __init__(self, x0, lower, upper, m, maxit, factr, pgtol, max_backtracks):
        self.x = np.clip(np.asarray(x0, dtype=np.float64).ravel(), lower, upper)
        self.lo, self.hi = lower, upper
        self.m, self.maxit, self.factr, self.pgtol = m, maxit, factr, pgtol
        self.max_backtracks = max_backtracks
        self.f = np.inf
        self.g = None
        self.S, self.Y = [], []
        self.iterations = 0
        self.converged = False
        self.message = ""
        self.running = True
        self.trial = self.x.copy()   # the first call evaluates the start itself
        self.first = True

    # ---- projected gradient and search direction -------------------------------------------------------------
    def _free(self, x, g):
        at_lo = (x <= self.lo) & (g > 0.0)
        at_hi = (x >= self.hi) & (g < 0.0)
        return ~(at_lo | at_hi)

    def _pg_norm(self, x, g):
        return float(np.max(np.abs(np.clip(x - g, self.lo, self.hi) - x))) if x.size else 0.0

    def _direction(self):
        free = self._free(self.x, self.g)
        q = np.where(free, self.g, 0.0)
        alphas = []
        pairs = []
        for s, y in zip(reversed(self.S), reversed(self.Y)):   # newest first
            sf, yf = np.where(free, s, 0.0), np.where(free, y, 0.0)
            sy = _dot(sf, yf)
            if sy <= _EPS * _dot(yf, yf) or sy <= 0.0:
                continue
            rho = 1.0 / sy
            a = rho * _dot(sf, q)
            q = q - a * yf
            alphas.append(a)
            pairs.append((sf, yf, rho))
        if pairs:
            sf, yf, rho = pairs[0]
            q = q * ((1.0 / rho) / _dot(yf, yf))
        for (sf, yf, rho), a in zip(reversed(pairs), reversed(alphas)):   # oldest first
            b = rho * _dot(yf, q)
            q = q + (a - b) * sf
        p = -q
        gd = _dot(self.g, p)
        if not pairs or not gd < 0.0:
            self.S, self.Y = [], []
            p = -np.where(free, self.g, 0.0)
            pairs = []
        return p, not pairs

    def _begin_iteration(self):
        self.p, steepest = self._direction()
        pn = float(np.sqrt(_dot(self.p, self.p)))
        if pn == 0.0:   # every variable frozen or a zero gradient: a Kuhn-Tucker point
            self.converged, self.running = True, False
            self.message = "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL"
            return
        self.t = min(1.0, 1.0 / pn) if steepest else 1.0
        self.backtracks = 0
        self.trial = np.clip(self.x + self.t * self.p, self.lo, self.hi)

    # ---- one evaluation result ---------------------------------------------------------------------------------
    def feed(self, f, g, ok):
        f = float(f)
        ok = bool(ok) and np.isfinite(f) and bool(np.all(np.isfinite(g)))
        if self.first:
            self.first = False
            if not ok:
                self.running = False
                self.message = "the start itself cannot be evaluated"
                return
            self.f, self.g = f, np.array(g, dtype=np.float64).ravel()
            if self._pg_norm(self.x, self.g) <= self.pgtol:
                self.converged, self.running = True, False
                self.message = "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL"
                return
            self._begin_iteration()
            return
        step = self.trial - self.x
        slope = _dot(self.g, step)
        if ok and f <= self.f + 1e-4 * min(slope, 0.0):
            self._accept(f, np.array(g, dtype=np.float64).ravel())
            return
        # backtrack: safeguarded quadratic interpolation on an infeasible-free trial, halving otherwise
        self.backtracks += 1
        if self.backtracks > self.max_backtracks or not np.any(step):
            if self.S:   # the quasi-Newton model misled the search: forget it and try steepest descent once more
                self.S, self.Y = [], []
                self._begin_iteration()
                return
            self.running = False
            self.message = "ABNORMAL_TERMINATION_IN_LNSRCH"
            return
        t = self.t
        if ok:
            dphi = slope / t
            denom = 2.0 * (f - self.f - dphi * t)
            tq = -dphi * t * t / denom if denom > 0.0 else 0.5 * t
            t = min(max(tq, 0.1 * t), 0.5 * t)
        else:
            t = 0.5 * t
        self.t = t
        self.trial = np.clip(self.x + t * self.p, self.lo, self.hi)

    def _accept(self, f, g):
        s, y = self.trial - self.x, g - self.g
        if _dot(s, y) > _EPS * _dot(y, y):
            self.S.append(s)
            self.Y.append(y)
            if len(self.S) > self.m:
                self.S.pop(0)
                self.Y.pop(0)
        f_old = self.f
        self.x, self.f, self.g = self.trial.copy(), f, g
        self.iterations += 1
        if (f_old - f) <= self.factr * _EPS * max(abs(f_old), abs(f), 1.0):
            self.converged, self.running = True, False
            self.message = "CONVERGENCE: REL_REDUCTION_OF_F <= FACTR*EPSMCH"
            return
        if self._pg_norm(self.x, self.g) <= self.pgtol:
            self.converged, self.running = True, False
            self.message = "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL"
            return
        if self.iterations >= self.maxit:
            self.running = False
            self.message = "NEW_X: maxit reached"
            return
        self._begin_iteration()


def minimize_starts(evaluate, starts, lower=-1.0, upper=1.0, m=5, maxit=100, factr=1e7, pgtol=0.0, max_backtracks=30,
                    lowers=None, uppers=None, pass_live=False):
    """Minimise f from every start in lockstep.

    evaluate(X[k, ...]) -> (f[k], grad[k, ...], status[k]) evaluates k points of the shape of one start; a status != 0
    or a non-finite value marks a point as infeasible.  starts: [S, ...].  Returns a dict with x [S, ...] (the last
    accepted iterate of each start), f [S] (inf where the start itself could not be evaluated), converged [S],
    iterations [S], message [S], calls (the number of evaluate calls) and calls_per_start [S] (the calls a start took
    part in: what `calls` would be had it run alone).

    lower / upper: a scalar or one array of the shape of a start, shared by all starts.  lowers / uppers ([S, ...], both or
    neither) give every start its own box instead -- the starts of several problems in one run, each under its problem's
    bounds.  A start's trajectory depends on its own box and its own evaluations only, so it is the trajectory of a run
    that holds that start alone under lower = lowers[s], upper = uppers[s].  pass_live: evaluate is called as
    evaluate(X, live) with the indices (into starts) of the k starts whose points X holds, in ascending order."""
    starts = np.asarray(starts, dtype=np.float64)
    S, shape = starts.shape[0], starts.shape[1:]
    if (lowers is None) != (uppers is None):
        raise ValueError("minimize_starts: lowers and uppers come together")
    if lowers is not None:
        lowers, uppers = np.asarray(lowers, dtype=np.float64), np.asarray(uppers, dtype=np.float64)
        if lowers.shape != starts.shape or uppers.shape != starts.shape:
            raise ValueError("minimize_starts: lowers and uppers must have the shape of starts")
        box = [(lowers[s].ravel(), uppers[s].ravel()) for s in range(S)]
    else:
        box = [(lower, upper)] * S
    st = [_Start(starts[s], box[s][0], box[s][1], m, maxit, factr, pgtol, max_backtracks) for s in range(S)]
    calls = 0
    per_start = np.zeros(S, dtype=np.int64)
    while True:
        live = [s for s in range(S) if st[s].running]
        if not live:
            break
        X = np.stack([st[s].trial.reshape(shape) for s in live])
        f, g, status = evaluate(X, np.array(live)) if pass_live else evaluate(X)
        calls += 1
        per_start[live] += 1
        for k, s in enumerate(live):
            st[s].feed(f[k], np.asarray(g[k]), status[k] == 0)
    return dict(x=np.stack([st[s].x.reshape(shape) for s in range(S)]),
                f=np.array([st[s].f for s in range(S)]),
                converged=np.array([st[s].converged for s in range(S)]),
                iterations=np.array([st[s].iterations for s in range(S)]),
                message=[st[s].message for s in range(S)],
                calls=calls, calls_per_start=per_start)


_FIT_MESSAGES = ("", "CONVERGENCE: REL_REDUCTION_OF_F <= FACTR*EPSMCH", "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL",
                 "NEW_X: maxit reached", "ABNORMAL_TERMINATION_IN_LNSRCH", "the start itself cannot be evaluated")


def minimize_starts_device(handle, starts, K, params_row, D_old=None, ld_offset=0.0, lower=-1.0, upper=1.0, maxit=100,
                           factr=1e7, pgtol=0.0, max_backtracks=30, on_device=True, seg=512, evaluate=None):
    """minimize_starts for the design criterion with the iteration itself on the device: the objective is
    f = -(log det R(D_old U x) - ld_offset) under the parameter row params_row (K components), and one launch of
    ccgp_design_fit carries every running start through up to `seg` evaluations (one workgroup per start: the design-gradient
    instance, the step of _Start restated in csrc/fit_logic.h with memory 5) until none is running.  starts: [S, n_free, d];
    lower / upper: a scalar or one array of the shape of a start.

    The iterate is the design, so nothing lies between the stepper and the evaluator: x, f, converged, iterations, message
    and calls_per_start are, bit for bit, what minimize_starts returns over handle.mixed_logdet_grad_designs with
    f = -(ld - ld_offset), g = -grad.  `calls` counts device calls: launches, or on the twin the evaluator calls.

    on_device=False drives the same states through the host twin -- every evaluation through ccgp_design_fit_eval (or through
    `evaluate`, minimize_starts' evaluator, where one is given), every step through ccgp_fit_feed -- and leaves the same
    states; the driver falls back to it by itself where the device call says CCGP_EUNSUPPORTED and the evaluator still serves
    the shape (a design-gradient carve that has no room for the start's words).  Beyond 64 free coordinates no such state
    exists: minimize_starts runs over the same evaluator.  Where the evaluator itself refuses (n > 128, the Matern and spline
    families) its error is the caller's."""
    from . import api

    starts = np.asarray(starts, dtype=np.float64)
    if starts.ndim != 3:
        raise ValueError("minimize_starts_device: starts must be [S, n_free, d]")
    S, nfree, d = starts.shape
    nv = nfree * d
    seg = int(seg)
    if seg < 1 or seg > api.FIT_MAX_EVALS:
        raise ValueError("minimize_starts_device: seg must lie in 1 .. %d" % api.FIT_MAX_EVALS)
    lo = np.broadcast_to(np.asarray(lower, dtype=np.float64), (nfree, d)).ravel()
    hi = np.broadcast_to(np.asarray(upper, dtype=np.float64), (nfree, d)).ravel()
    if evaluate is None:
        def evaluate(X):
            return handle.design_fit_eval(X, K, params_row, D_old, ld_offset)
    device = bool(on_device)
    if nv > 64:   # the stepper's state ends at 64 variables (csrc/fit_logic.h): minimize_starts itself over the twin's evaluator
        return minimize_starts(evaluate, starts, lower, upper, 5, maxit, factr, pgtol, max_backtracks)
    state = np.stack([api.fit_begin(s.ravel(), lo, hi, maxit, factr, pgtol, max_backtracks) for s in starts]) if S else \
        np.zeros((0, api.FIT_HEADER + 16 * nv))
    calls = 0
    while True:
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        if device:
            try:
                r = handle.design_fit(nfree, d, K, params_row, state[live], seg, D_old, ld_offset)
            except api.CcgpError as e:
                if e.code != -4:   # CCGP_EUNSUPPORTED: this shape has no device search; the twin carries it
                    raise
                device = False
                continue
            state[live] = r["state"]
            calls += 1
        else:
            for _ in range(seg):
                run = live[state[live, api.FIT_CODE] == api.FIT_RUNNING]
                if run.size == 0:
                    break
                f, g, st = evaluate(api.fit_trial(state[run]).reshape(run.size, nfree, d))
                calls += 1
                for k, a in enumerate(run):
                    api.fit_feed(state[a], f[k], np.asarray(g[k]).ravel(), st[k] == 0)
    code = state[:, api.FIT_CODE].astype(np.int64)
    return dict(x=api.fit_x(state).reshape(S, nfree, d), f=state[:, api.FIT_F].copy(),
                converged=(code == api.FIT_CONV_REDUCTION) | (code == api.FIT_CONV_PROJ_GRAD),
                iterations=state[:, api.FIT_ITERATIONS].astype(np.int64), message=[_FIT_MESSAGES[c] for c in code],
                calls=calls, calls_per_start=state[:, api.FIT_EVALS].astype(np.int64))


def make_starts(n_starts, n, d, rng):
    """-1 + 2 LHS(n, d) per start (BSQ:899, BSQ:935), from a seeded numpy generator."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    return np.stack([-1.0 + 2.0 * latin_hypercube(n, d, rng) for _ in range(n_starts)])
