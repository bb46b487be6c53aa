"""Host-side counterpart of the reference's inference layer: `laplace`, `Metro`,
`factors.frame`, `prediction`, `compare.GP`, `Combined.GP.fit` on top of the device evaluator.

This layer is sequential and RNG-driven in the reference (HX:483-540, HX:686-725); it is re-hosted
so that the hot path has a complete caller, and `Metro(..., speculate=m)` puts the sequential chain
on the BATCHED device path without changing a bit of it (prefetching Metropolis).  Every likelihood /
prediction it needs goes through libccgp (`rsurface.CombinedGP`).  RNG contract: numpy
`Generator` (PCG64) seeded by the caller -- R's Mersenne-Twister stream cannot be reproduced
without R, so agreement with the reference is statistical, never bitwise.

Reference behaviours kept on purpose (they shape the output):
  * only ACCEPTED proposals are stored and counted (`samp[k,] <- theta.candidate`, HX:515-522);
  * the proposal covariance is sqrt(2) * V_laplace (HX:511);
  * the Geweke stop rule looks at `samp[(k-samp.size):(k-1)]` (k already incremented: exactly samp.size
    accepted draws), which indexes the N x p matrix as a vector, i.e. the FIRST parameter's chain only
    (HX:530);
  * the predictive interval is the empirical quantile of one rnorm draw per posterior draw
    (HX:696-699), type-7 quantiles.
Third-party pieces restated from their definitions: LearnBayes::laplace (optim Nelder-Mead +
finite-difference Hessian), coda::geweke.diag (first 10 % vs last 50 %, spectral density at
zero from an AIC-selected AR fit), mlegp's sigma2 (ordinary-kriging MLE; here a deterministic
L-BFGS on the concentrated likelihood instead of mlegp's randomised simplex restarts).
"""
from __future__ import annotations

import math

import numpy as np

from . import api


# ----------------------------------------------------------------------------- priors / Jacobian (host)
def log_jacobian(theta_t):
    """-phi - 2 log(1 + e^-phi) + psi1 + psi2 [+ zeta]  (HX:461, ANI:459); vectorised over rows."""
    t = np.atleast_2d(np.asarray(theta_t, dtype=np.float64))
    val = -t[:, 2] - 2.0 * np.log1p(np.exp(-t[:, 2])) + t[:, 0] + t[:, 1]
    if t.shape[1] == 4:
        val = val + t[:, 3]
    return val


def log_prior(theta_t, script, prior_pars=None):
    """HX:462 / ADV:467, GV:450, ISO:453 = BSQ:450, ANI:462; vectorised over rows."""
    t = np.atleast_2d(np.asarray(theta_t, dtype=np.float64))
    psi1, psi2 = t[:, 0], t[:, 1]
    th1, th2 = np.exp(psi1), np.exp(psi2)
    if script in ("HX", "ADV"):
        a1, b1, a2, b2 = prior_pars
        return -(a1 + 1.0) * psi1 - b1 / th1 - (a2 + 1.0) * psi2 - b2 / th2
    if script == "GV":
        return -4.0 * psi1 - 1.0 / th1 - 6.0 * psi2 - 75.0 / th2
    if script in ("ISO", "BSQ", "D1"):   # D1:636 = ISO:453
        return -4.0 * psi1 - 2.0 / th1 - 6.0 * psi2 - 16.0 / th2
    if script == "ANI":
        zeta = t[:, 3]
        return -psi1 - psi1 ** 2 / 2.0 - psi2 - psi2 ** 2 / 2.0 - 4.0 * zeta - 4.0 / np.exp(zeta)
    raise ValueError(script)


def transformed_to_draws(theta_t):
    """(psi1, psi2, phi[, zeta]) rows -> (p, theta1, theta2[, lambda]) rows (HX:631-636)."""
    t = np.atleast_2d(np.asarray(theta_t, dtype=np.float64))
    cols = [1.0 / (1.0 + np.exp(-t[:, 2])), np.exp(t[:, 0]), np.exp(t[:, 1])]
    if t.shape[1] == 4:
        cols.append(np.exp(t[:, 3]))
    return np.stack(cols, axis=1)


def logpost_batch(gp, D_train, theta_t, y, sigma2, prior_pars=None):
    """`logpost(...)$val` for MANY transformed draws in one device call -> (val, beta).
    Rows whose covariance cannot be factorised give NaN (the reference's NA, HX:454-455).
    The Gaussian-kernel scripts go through ccgp_logpost_batch, whose Jacobian and prior arithmetic is the C code of the
    one-at-a-time ccgp_logpost: a value is the same bits whichever call produced it (the chain of Metro(speculate = m), the
    R shim's ccgp_R_metro_steps and the sequential chain are then the same chain)."""
    t = np.atleast_2d(np.asarray(theta_t, dtype=np.float64))
    cfg = getattr(gp, "cfg", None)
    if cfg is not None and hasattr(gp.h, "logpost_batch") and gp.script in ("HX", "ADV", "GV", "ISO", "BSQ", "ANI"):
        val, beta, _, _ = gp.h.logpost_batch(D_train, y, sigma2, cfg["prior"], t, prior_pars)
        return val, beta
    draws = transformed_to_draws(t)
    params = gp.draws_to_params(D_train, draws)
    ll, beta, _ = gp.h.loglik_batch(D_train, y, 2, params, sigma2, api.MEAN_PROFILE_BETA, 0.0)
    return ll + log_jacobian(t) + log_prior(t, gp.script, prior_pars), beta


# ----------------------------------------------------------------------------- LearnBayes::laplace
def _hessian_vars(fn_sets, modes, hess_step):
    """The covariance -H^-1 at each row of modes [C, p], H by central differences: the points of all modes go out as ONE
    fn_sets(rows, set_of) call.  Where H is not negative definite the covariance falls back to H's diagonal."""
    C, p = modes.shape
    idx = [(i, j) for i in range(p) for j in range(i, p)]
    pts = []
    for mode in modes:
        for i, j in idx:
            for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                x = mode.copy()
                x[i] += si * hess_step
                x[j] += sj * hess_step
                pts.append(x)
    vals = np.asarray(fn_sets(np.asarray(pts), np.repeat(np.arange(C), 4 * len(idx))), dtype=np.float64).reshape(C, -1, 4)
    out = []
    for c in range(C):
        H = np.zeros((p, p))
        for (i, j), v in zip(idx, vals[c]):
            H[i, j] = H[j, i] = (v[0] - v[1] - v[2] + v[3]) / (4.0 * hess_step ** 2)
        try:
            var = -np.linalg.inv(H)
            np.linalg.cholesky(var)
        except np.linalg.LinAlgError:
            var = np.diag(1.0 / np.maximum(-np.diag(H), 1e-6))   # not negative definite: fall back to its diagonal
        out.append(var)
    return out


def laplace(fn_batch, start, hess_step=1e-3, maxiter=2000):
    """Posterior mode by Nelder-Mead and covariance = -H^-1 from central differences
    (LearnBayes::laplace -> optim(..., hessian = TRUE); HX:493).  `fn_batch(rows) -> values`."""
    from scipy.optimize import minimize

    start = np.asarray(start, dtype=np.float64)

    def neg(x):
        v = float(fn_batch(x[None])[0])
        return 1e300 if not math.isfinite(v) else -v

    res = minimize(neg, start, method="Nelder-Mead",
                   options=dict(xatol=1e-6, fatol=1e-9, maxiter=maxiter, maxfev=maxiter))
    var = _hessian_vars(lambda rows, set_of: fn_batch(rows), res.x[None], hess_step)[0]
    return dict(mode=res.x, var=var, converged=bool(res.success), value=-float(res.fun))


# ----------------------------------------------------------------------------- coda::geweke.diag
def _spectrum0_ar(x):
    """Spectral density at frequency zero from an AR(p) fit, p chosen by AIC (coda::spectrum0.ar)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    xc = x - x.mean()
    v0 = float(xc @ xc) / n
    if v0 == 0.0:
        return 0.0
    pmax = min(n - 1, int(10 * math.log10(n)))
    r = np.array([float(xc[: n - k] @ xc[k:]) / n for k in range(pmax + 1)])
    best = (n * math.log(v0), 0, v0, np.zeros(0))
    phi = np.zeros(0)
    var = v0
    for p in range(1, pmax + 1):          # Levinson-Durbin
        kappa = (r[p] - float(phi @ r[p - 1:0:-1])) / var if p > 1 else r[1] / r[0]
        phi = np.concatenate([phi - kappa * phi[::-1], [kappa]])
        var = var * (1.0 - kappa ** 2)
        if var <= 0:
            break
        aic = n * math.log(var) + 2 * p
        if aic < best[0]:
            best = (aic, p, var, phi.copy())
    _, p, var, phi = best
    var_pred = var * n / max(n - (p + 1), 1)
    return var_pred / (1.0 - phi.sum()) ** 2


def geweke_z(x, frac1=0.1, frac2=0.5):
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    a = x[: max(int(math.floor(frac1 * n)), 2)]
    b = x[n - max(int(math.floor(frac2 * n)), 2):]
    va, vb = _spectrum0_ar(a) / a.size, _spectrum0_ar(b) / b.size
    if not (va + vb > 0):
        raise FloatingPointError("degenerate chain")
    return (a.mean() - b.mean()) / math.sqrt(va + vb)


def geweke_window(samp, k, samp_size):
    """`samp[(k-samp.size):(k-1)]` of HX:530 with R's k (one past the last accepted draw, 1-based):
    the last samp.size accepted values of the first parameter."""
    return samp[k - samp_size:k, 0]


# ----------------------------------------------------------------------------- Metro / factors.frame
class _Chain:
    """The state of one chain of HX:483-540 and everything about it that does not evaluate: the random numbers of a proposal
    (draw_pair), what a proposal does given its value (consume), the tree of candidates the chain can reach over its next m
    proposals (tree) and the walk through it once the values are known (walk).  Metro drives one of these with one
    evaluator call per step, Metro_sets many of them with one call per step for all: same code, same chain."""

    def __init__(self, est, l0, N, samp_size, batch_size, alpha, rng, max_proposals):
        self.est = est
        self.cov = math.sqrt(2.0) * est["var"]
        p = est["mode"].size
        self.zero = np.zeros(p)
        self.samp = np.zeros((N, p))
        self.betas = np.zeros(N)
        self.N, self.samp_size, self.batch_size, self.alpha, self.rng = N, samp_size, batch_size, alpha, rng
        self.theta, self.l, self.k, self.pv, self.proposals, self.batches = est["mode"].copy(), l0, 0, 0.0, 0, 0
        self.max_proposals = max_proposals or 200 * N
        self.state0 = rng.bit_generator.state
        self.pending = []                     # pre-drawn (u, e) pairs not yet consumed

    def draw_pair(self):
        # same stream as `u <- runif(1); rmnorm(1, theta.old, cov)` (HX:507-511): the proposal is
        # theta.old + e with e ~ N(0, cov), and adding the mean afterwards is what numpy does too
        u = self.rng.random()
        return u, self.rng.multivariate_normal(self.zero, self.cov)

    def running(self):
        return self.k < self.N and self.pv < self.alpha and self.proposals < self.max_proposals

    def consume(self, u, cand, l_cand, b_cand):
        """One proposal of HX:505-535 given its value.  Returns True when it was accepted."""
        from scipy.stats import norm

        self.proposals += 1
        if not (math.isfinite(l_cand) and (l_cand - self.l) > math.log(u)):
            return False
        k = self.k
        self.samp[k] = cand
        self.betas[k] = b_cand
        self.theta, self.l, self.k = cand, l_cand, k + 1
        k += 1
        if k >= self.samp_size and k % self.batch_size == 0:
            try:   # first parameter's chain over the last samp_size accepted draws (HX:530, GV:518)
                z = geweke_z(geweke_window(self.samp, k, self.samp_size))
                self.pv = float(2.0 * (1.0 - norm.cdf(abs(z))))
            except Exception:
                self.pv = 0.0
        return True

    def propose(self):
        """The sequential step: one (u, candidate)."""
        u, e = self.draw_pair()
        return u, self.theta + e

    def tree(self, m):
        """The 2^m - 1 candidates reachable over the next m proposals, level by level."""
        while len(self.pending) < m:
            self.pending.append(self.draw_pair())
        # level t holds the 2^t candidates reachable after t proposals; history bits: 1 = accepted
        states, levels = np.asarray(self.theta, dtype=float)[None, :], []
        for t in range(m):
            cands = states + self.pending[t][1]              # same additions as the sequential chain: same bits
            levels.append(cands)
            states = np.stack([states, cands], axis=1).reshape(2 * states.shape[0], -1)   # (s0, c0, s1, c1, ...)
        return levels

    def walk(self, levels, l_all, b_all):
        """The accept / reject walk over a tree whose values (level after level) are l_all, b_all."""
        idx, off, used = 0, 0, 0
        for t in range(len(levels)):
            if not self.running():
                break
            acc = self.consume(self.pending[t][0], levels[t][idx], float(l_all[off + idx]), float(b_all[off + idx]))
            used += 1
            off += 1 << t
            idx = 2 * idx + (1 if acc else 0)
        self.pending = self.pending[used:]

    def rewind(self):
        """After speculation: leave the generator where the sequential chain leaves it, exactly `proposals` pairs drawn."""
        self.rng.bit_generator.state = self.state0
        for _ in range(self.proposals):
            self.draw_pair()

    def result(self, who="Metro"):
        k = self.k
        if k < self.samp_size:
            raise RuntimeError("%s: only %d accepted draws after %d proposals" % (who, k, self.proposals))
        return dict(sample=self.samp[k - self.samp_size:k].copy(), beta=self.betas[k - self.samp_size:k].copy(), accepted=k,
                    proposals=self.proposals, laplace=self.est, geweke_p=self.pv, device_batches=self.batches)


def _prior_pars(gp, theta1_pars, theta2_pars):
    """(a1, b1, a2, b2) for the scripts whose prior takes its parameters from the caller (HX, ADV); None for the others."""
    if gp.script in ("HX", "ADV"):
        return (*np.ravel(theta1_pars)[:2], *np.ravel(theta2_pars)[:2])
    return None


def Metro(gp, start, N, samp_size, batch_size, alpha, D_train, sigma2, y, theta1_pars=None,
          theta2_pars=None, rng=None, max_proposals=None, speculate=0, logpost_fn=None):
    """HX:483-540 (and its per-script copies).  Returns dict(sample[samp_size, p], beta[samp_size],
    accepted, proposals, laplace).

    speculate = m > 1 evaluates the chain m proposals at a time ("prefetching" Metropolis): the
    random numbers of the next m proposals are drawn first, the 2^m - 1 candidates the chain can
    reach over those proposals (one per accept/reject history) go through the device evaluator as ONE
    batch, and the accept/reject walk then only reads values.  Every candidate is evaluated by the
    same kernel on its own workgroup, so the chain -- and the generator state it leaves behind -- is
    bit-for-bit the sequential one; only the number of device round trips drops m-fold
    (the sequential caller on the batched path).  `logpost_fn(rows) -> (val, beta)`
    replaces the device evaluator (tests)."""
    rng = np.random.default_rng(rng)
    if logpost_fn is None:
        pars = _prior_pars(gp, theta1_pars, theta2_pars)

        def logpost_fn(rows):
            return logpost_batch(gp, D_train, rows, y, sigma2, pars)

    est = laplace(lambda rows: logpost_fn(rows)[0], start)
    ch = _Chain(est, float(logpost_fn(est["mode"][None])[0][0]), N, samp_size, batch_size, alpha, rng, max_proposals)
    m = int(speculate)
    if m <= 1:
        while ch.running():
            u, cand = ch.propose()
            l_cand, b_cand = logpost_fn(cand[None])
            ch.batches += 1
            ch.consume(u, cand, float(l_cand[0]), float(b_cand[0]))
    else:
        while ch.running():
            levels = ch.tree(m)
            l_all, b_all = logpost_fn(np.concatenate(levels, axis=0))
            ch.batches += 1
            ch.walk(levels, l_all, b_all)
        ch.rewind()
    return ch.result()


def logpost_sets_batch(gp, D_trains, theta_t, ys, sigma2s, set_of, prior_pars=None):
    """logpost_batch over many training sets of one shape: row b of theta_t on set set_of[b], ONE device call
    (ccgp_logpost_sets) -> (val, beta), each value with the bits logpost_batch gives it on its set alone."""
    val, beta, _, _ = gp.h.logpost_sets(D_trains, ys, sigma2s, gp.cfg["prior"], theta_t, set_of, prior_pars)
    return val, beta


def _device_sets_evaluator(gp, D_trains, ys, sigma2s, theta1_pars, theta2_pars):
    """`(rows, set_of) -> (val, beta)` over logpost_sets_batch with the sets stacked once."""
    pars = _prior_pars(gp, theta1_pars, theta2_pars)
    Xs = np.stack([np.asarray(D, dtype=np.float64) for D in D_trains])
    Y = np.stack([np.asarray(y, dtype=np.float64).ravel() for y in ys])
    return lambda rows, set_of: logpost_sets_batch(gp, Xs, rows, Y, sigma2s, set_of, pars)


def laplace_sets(fn_sets, starts, hess_step=1e-3, maxiter=2000):
    """laplace for C sets in lockstep.  `fn_sets(rows, set_of) -> values` evaluates row b on set set_of[b]; starts is [C, p].
    The search is a Nelder-Mead written here (coefficients 1, 2, 1/2, 1/2; the initial simplex and the stop rule -- xatol
    1e-6, fatol 1e-9 -- are those of the search laplace runs): per iteration the reflection, expansion and both contraction
    points of every unfinished set go out as ONE call, the shrink steps of the sets that need one as a second; then the
    central-difference Hessian points of all sets go out as one call.  Every decision of a set reads that set's values
    only, so its result has the same bits alone and among others.  Returns one dict per set with laplace's keys, plus the
    iterations and evaluations the set took."""
    starts = np.atleast_2d(np.asarray(starts, dtype=np.float64))
    C, p = starts.shape
    xatol, fatol = 1e-6, 1e-9

    def neg(rows, set_of):
        v = np.asarray(fn_sets(np.asarray(rows), np.asarray(set_of, dtype=np.int64)), dtype=np.float64)
        return np.where(np.isfinite(v), -v, 1e300)

    sim = np.empty((C, p + 1, p))
    for c in range(C):
        sim[c, 0] = starts[c]
        for k in range(p):
            x = starts[c].copy()
            x[k] = (1.0 + 0.05) * x[k] if x[k] != 0.0 else 0.00025
            sim[c, k + 1] = x
    fsim = neg(sim.reshape(-1, p), np.repeat(np.arange(C), p + 1)).reshape(C, p + 1)
    iters, evals, done = np.zeros(C, dtype=int), np.full(C, p + 1), np.zeros(C, dtype=bool)
    converged = np.zeros(C, dtype=bool)
    for c in range(C):
        o = np.argsort(fsim[c], kind="stable")
        sim[c], fsim[c] = sim[c][o], fsim[c][o]
    while True:
        for c in range(C):
            if done[c]:
                continue
            if np.max(np.abs(sim[c, 1:] - sim[c, 0])) <= xatol and np.max(np.abs(fsim[c, 0] - fsim[c, 1:])) <= fatol:
                done[c] = converged[c] = True
            elif iters[c] >= maxiter or evals[c] >= maxiter:
                done[c] = True
        live = [c for c in range(C) if not done[c]]
        if not live:
            break
        rows = []
        for c in live:
            xbar, worst = sim[c, :-1].sum(axis=0) / p, sim[c, -1]
            rows += [2.0 * xbar - worst, 3.0 * xbar - 2.0 * worst, 1.5 * xbar - 0.5 * worst, 0.5 * xbar + 0.5 * worst]
        f = neg(rows, np.repeat(live, 4)).reshape(-1, 4)
        shrink = []
        for j, c in enumerate(live):
            (xr, xe, xoc, xic), (fr, fe, foc, fic) = rows[4 * j:4 * j + 4], f[j]
            iters[c] += 1
            evals[c] += 4
            if fr < fsim[c, 0]:
                sim[c, -1], fsim[c, -1] = (xe, fe) if fe < fr else (xr, fr)
            elif fr < fsim[c, -2]:
                sim[c, -1], fsim[c, -1] = xr, fr
            elif fr < fsim[c, -1] and foc <= fr:
                sim[c, -1], fsim[c, -1] = xoc, foc
            elif fr >= fsim[c, -1] and fic < fsim[c, -1]:
                sim[c, -1], fsim[c, -1] = xic, fic
            else:
                shrink.append(c)
        if shrink:
            for c in shrink:
                sim[c, 1:] = sim[c, 0] + 0.5 * (sim[c, 1:] - sim[c, 0])
            fs = neg(np.concatenate([sim[c, 1:] for c in shrink]), np.repeat(shrink, p)).reshape(-1, p)
            for j, c in enumerate(shrink):
                fsim[c, 1:] = fs[j]
                evals[c] += p
        for c in live:
            o = np.argsort(fsim[c], kind="stable")
            sim[c], fsim[c] = sim[c][o], fsim[c][o]
    var = _hessian_vars(fn_sets, sim[:, 0], hess_step)
    return [dict(mode=sim[c, 0].copy(), var=var[c], converged=bool(converged[c]), value=-float(fsim[c, 0]),
                 iterations=int(iters[c]), evaluations=int(evals[c])) for c in range(C)]


def Metro_sets(gp, starts, N, samp_size, batch_size, alpha, D_trains, sigma2s, ys, theta1_pars=None, theta2_pars=None,
               rngs=None, max_proposals=None, speculate=0, laplace=None, logpost_sets_fn=None):
    """Metro for C training sets of one shape in lockstep: one generator per chain (rngs[c]) and ONE device call per step
    that carries the candidates of every chain still running -- C (2^m - 1) of them with speculate = m.  A chain that stops
    (Geweke, N, max_proposals) leaves the batch.  Each chain is Metro's chain for its set and generator, bit for bit, and
    leaves its generator where Metro leaves it.  laplace: ready estimates, one per set (laplace's dicts); without them
    laplace_sets runs from starts [C, p].  `logpost_sets_fn(rows, set_of) -> (val, beta)` replaces the device evaluator.
    Returns dict(chains: one Metro result per set -- its device_batches counts the steps the chain took part in --,
    device_batches: the calls this function made for the chains, laplace_calls: those of the Laplace stage)."""
    C = len(D_trains)
    rngs = [np.random.default_rng(r) for r in (rngs if rngs is not None else [None] * C)]
    if len(rngs) != C:
        raise ValueError("Metro_sets takes one generator per set")
    laplace_calls = 0
    if logpost_sets_fn is None:
        logpost_sets_fn = _device_sets_evaluator(gp, D_trains, ys, sigma2s, theta1_pars, theta2_pars)

    def evaluate(rows, set_of):
        return logpost_sets_fn(np.asarray(rows), np.asarray(set_of, dtype=np.int64))

    def counted(rows, set_of):
        nonlocal laplace_calls
        laplace_calls += 1
        return evaluate(rows, set_of)[0]

    if laplace is None:
        ests = laplace_sets(counted, starts)
    else:
        ests = list(laplace)
        if len(ests) != C:
            raise ValueError("Metro_sets takes one Laplace estimate per set")
    l0 = evaluate(np.stack([e["mode"] for e in ests]), np.arange(C))[0]
    chains = [_Chain(ests[c], float(l0[c]), N, samp_size, batch_size, alpha, rngs[c], max_proposals) for c in range(C)]
    batches, m = 0, int(speculate)
    per = (1 << m) - 1
    while True:
        live = [c for c in range(C) if chains[c].running()]
        if not live:
            break
        if m <= 1:
            pairs = [chains[c].propose() for c in live]
            l_all, b_all = evaluate(np.stack([cand for _, cand in pairs]), live)
        else:
            trees = [chains[c].tree(m) for c in live]
            l_all, b_all = evaluate(np.concatenate([np.concatenate(t, axis=0) for t in trees], axis=0), np.repeat(live, per))
        batches += 1
        for j, c in enumerate(live):
            chains[c].batches += 1
            if m <= 1:
                chains[c].consume(pairs[j][0], pairs[j][1], float(l_all[j]), float(b_all[j]))
            else:
                chains[c].walk(trees[j], l_all[j * per:(j + 1) * per], b_all[j * per:(j + 1) * per])
    if m > 1:
        for ch in chains:
            ch.rewind()
    return dict(chains=[ch.result("Metro_sets (set %d)" % c) for c, ch in enumerate(chains)], device_batches=batches,
                laplace_calls=laplace_calls)


# ----------------------------------------------------------------------------- chains on the device
class _BlockChain(_Chain):
    """_Chain with the random numbers of its proposals drawn ahead in blocks, which is what lets the accept / reject walk run
    where the evaluator is.  Stream contract: proposals t = 0, 1, ... use, block after block, u = rng.random(block) and then
    z = rng.standard_normal((block, p)); the increment is e_t = L z_t with L the Cholesky factor of sqrt(2) V (computed
    once), each component summed left to right with elementwise numpy operations (no BLAS), and log u_t is math.log on the
    host.  Numbers a segment did not use stay pending for the next one."""

    def __init__(self, est, l0, b0, N, samp_size, batch_size, alpha, rng, max_proposals, block):
        super().__init__(est, l0, N, samp_size, batch_size, alpha, rng, max_proposals)
        self.beta = b0
        self.block = int(block)
        self.L = np.linalg.cholesky(self.cov)
        p = self.zero.size
        self.pend_e, self.pend_logu, self.blocks = np.zeros((0, p)), np.zeros(0), 0

    def fill(self, m):
        """At least m pending proposals, where the chain may still use that many."""
        p = self.zero.size
        while self.pend_logu.size < m:
            u = self.rng.random(self.block)
            z = self.rng.standard_normal((self.block, p))
            e = np.empty((self.block, p))
            for i in range(p):
                acc = self.L[i, 0] * z[:, 0]
                for j in range(1, i + 1):
                    acc = acc + self.L[i, j] * z[:, j]
                e[:, i] = acc
            logu = np.array([math.log(v) if v > 0.0 else -math.inf for v in u])
            self.pend_e, self.pend_logu = np.concatenate([self.pend_e, e]), np.concatenate([self.pend_logu, logu])
            self.blocks += 1

    def rewind(self):
        """Leave the generator where the contract says: after exactly ceil(proposals / block) blocks."""
        self.rng.bit_generator.state = self.state0
        for _ in range(-(-self.proposals // self.block)):
            self.rng.random(self.block)
            self.rng.standard_normal((self.block, self.zero.size))

    def request(self, seg):
        """(proposals, acceptances) the next segment may use: up to seg proposals, stopping at the next acceptance count
        consume() would look at -- k >= samp_size and k % batch_size == 0 -- or at N."""
        n_prop = min(int(seg), self.max_proposals - self.proposals)
        nxt = max(self.samp_size, self.k + 1)
        stop_k = min(self.N, -(-nxt // self.batch_size) * self.batch_size)
        self.fill(n_prop)
        return n_prop, stop_k - self.k

    def absorb(self, used, draws, vals, betas):
        """What a segment did: `used` proposals, the accepted draws in order.  Then the Geweke rule as consume() applies it."""
        from scipy.stats import norm

        a = len(vals)
        self.samp[self.k:self.k + a] = draws
        self.betas[self.k:self.k + a] = betas
        self.proposals += int(used)
        self.pend_e, self.pend_logu = self.pend_e[used:], self.pend_logu[used:]
        if not a:
            return
        self.theta, self.l, self.beta, self.k = np.array(draws[-1], dtype=np.float64), float(vals[-1]), float(betas[-1]), self.k + a
        k = self.k
        if k >= self.samp_size and k % self.batch_size == 0:
            try:
                z = geweke_z(geweke_window(self.samp, k, self.samp_size))
                self.pv = float(2.0 * (1.0 - norm.cdf(abs(z))))
            except Exception:
                self.pv = 0.0


def _twin_sets_evaluator(gp, D_trains, ys, sigma2s, theta1_pars, theta2_pars):
    """`(rows, set_of) -> (val, beta)` over ccgp_chain_logpost_sets: the evaluation a device chain makes, on the host side."""
    pars = _prior_pars(gp, theta1_pars, theta2_pars)
    Xs = np.stack([np.asarray(D, dtype=np.float64) for D in D_trains])
    Y = np.stack([np.asarray(y, dtype=np.float64).ravel() for y in ys])

    def fn(rows, set_of):
        val, beta, _, _ = gp.h.chain_logpost_sets(Xs, Y, sigma2s, gp.cfg["prior"], rows, set_of, pars)
        return val, beta

    return fn


def _host_segments(chains, live, reqs, evaluate):
    """The segments of the live chains one proposal at a time: one evaluator call per step for every chain still inside its
    segment.  Same decisions as the kernel, in Python: isfinite(val) and val - l > log u."""
    state = {c: dict(theta=np.array(chains[c].theta, dtype=np.float64), l=chains[c].l, t=0, draws=[], vals=[], betas=[]) for c in live}
    calls = 0
    while True:
        go = [c for c in live if state[c]["t"] < reqs[c][0] and len(state[c]["vals"]) < reqs[c][1]]
        if not go:
            break
        cands = [state[c]["theta"] + chains[c].pend_e[state[c]["t"]] for c in go]
        val, beta = evaluate(np.stack(cands), go)
        calls += 1
        for j, c in enumerate(go):
            s = state[c]
            v = float(val[j])
            if math.isfinite(v) and (v - s["l"]) > chains[c].pend_logu[s["t"]]:
                s["theta"], s["l"] = cands[j], v
                s["draws"].append(cands[j]); s["vals"].append(v); s["betas"].append(float(beta[j]))
            s["t"] += 1
    for c in live:
        s = state[c]
        chains[c].absorb(s["t"], np.array(s["draws"]).reshape(len(s["vals"]), chains[c].zero.size), s["vals"], s["betas"])
    return calls


def Metro_device_sets(gp, starts, N, samp_size, batch_size, alpha, D_trains, sigma2s, ys, theta1_pars=None, theta2_pars=None,
                      rngs=None, max_proposals=None, laplace=None, block=256, seg=2048, on_device=True,
                      logpost_sets_fn=None):
    """Metro for C training sets of one shape with the chains RESIDENT ON THE DEVICE: one launch (ccgp_metro_segments_sets)
    carries every live chain through up to `seg` proposals -- candidate, Jacobian and prior, likelihood and the accept /
    reject step all in the kernel, one workgroup per chain -- and comes back only where the Geweke rule looks at the chain.
    Stream contract (not Metro's: the proposals are drawn in vectorised blocks, so these are different chains with the same
    law).  Chain c owns rngs[c]; its proposals t = 0, 1, ... use numbers drawn in blocks of `block`: u = rng.random(block),
    then z = rng.standard_normal((block, p)); e_t = L z_t with L the Cholesky factor of sqrt(2) V computed once, L z_t by
    elementwise numpy operations in a fixed order; log u on the host.  Unused numbers stay pending for the next segment, so
    a chain depends on `block` and on nothing else about how it is cut into launches (seg, the other chains), and leaves its
    generator after exactly ceil(proposals / block) blocks.
    Stop logic is Metro's: a segment stops at the next acceptance count k with k >= samp_size and k % batch_size == 0, at N,
    or at max_proposals; the host then applies the Geweke rule exactly as Metro does.  The Laplace stage and the starting
    values go through ccgp_chain_logpost_sets, the host twin of the kernel's evaluation.
    on_device=False runs the same driver one proposal at a time through that twin (or through logpost_sets_fn(rows, set_of)
    -> (val, beta)): the exact reference for the device chain, bit for bit, and what the driver falls back to where the
    device refuses the shape (n > 128; the 1-D families, unless gp was made with fused=True and n <= 32: then the kernel takes
    them and the chains stay on the device).  Returns Metro_sets' dict: chains (one Metro result per set),
    device_batches (the calls made for the chains), laplace_calls."""
    C = len(D_trains)
    rngs = [np.random.default_rng(r) for r in (rngs if rngs is not None else [None] * C)]
    if len(rngs) != C:
        raise ValueError("Metro_device_sets takes one generator per set")
    if logpost_sets_fn is not None:
        on_device = False
    else:
        logpost_sets_fn = _twin_sets_evaluator(gp, D_trains, ys, sigma2s, theta1_pars, theta2_pars)
    laplace_calls = 0

    def evaluate(rows, set_of):
        return logpost_sets_fn(np.asarray(rows), np.asarray(set_of, dtype=np.int64))

    def counted(rows, set_of):
        nonlocal laplace_calls
        laplace_calls += 1
        return evaluate(rows, set_of)[0]

    if laplace is None:
        ests = laplace_sets(counted, starts)
    else:
        ests = list(laplace)
        if len(ests) != C:
            raise ValueError("Metro_device_sets takes one Laplace estimate per set")
    l0, b0 = evaluate(np.stack([e["mode"] for e in ests]), np.arange(C))
    chains = [_BlockChain(ests[c], float(l0[c]), float(b0[c]), N, samp_size, batch_size, alpha, rngs[c], max_proposals, block)
              for c in range(C)]
    if on_device:
        pars = _prior_pars(gp, theta1_pars, theta2_pars)
        Xs = np.stack([np.asarray(D, dtype=np.float64) for D in D_trains])
        Y = np.stack([np.asarray(y, dtype=np.float64).ravel() for y in ys])
    batches = 0
    while True:
        live = [c for c in range(C) if chains[c].running()]
        if not live:
            break
        reqs = {c: chains[c].request(seg) for c in live}
        if on_device:
            T = max(r[0] for r in reqs.values())
            p = chains[live[0]].zero.size
            steps, logu = np.zeros((len(live), T, p)), np.zeros((len(live), T))
            for j, c in enumerate(live):
                steps[j, :reqs[c][0]], logu[j, :reqs[c][0]] = chains[c].pend_e[:reqs[c][0]], chains[c].pend_logu[:reqs[c][0]]
            try:
                r = gp.h.metro_segments_sets(Xs, Y, sigma2s, gp.cfg["prior"], live, np.stack([chains[c].theta for c in live]),
                                             [chains[c].l for c in live], steps, logu, [reqs[c][0] for c in live],
                                             [reqs[c][1] for c in live], pars, [chains[c].beta for c in live])
            except api.CcgpError as e:
                if e.code != -4:   # CCGP_EUNSUPPORTED: this shape has no device chain; the twin carries it
                    raise
                on_device = False
                continue
            batches += 1
            for j, c in enumerate(live):
                a = int(r["accepted"][j])
                chains[c].batches += 1
                chains[c].absorb(int(r["used"][j]), r["draws"][j, :a], r["draw_val"][j, :a], r["draw_beta"][j, :a])
        else:
            for c in live:
                chains[c].batches += 1
            batches += _host_segments(chains, live, reqs, evaluate)
    for ch in chains:
        ch.rewind()
    return dict(chains=[ch.result("Metro_device_sets (set %d)" % c) for c, ch in enumerate(chains)], device_batches=batches,
                laplace_calls=laplace_calls)


def Metro_device(gp, start, N, samp_size, batch_size, alpha, D_train, sigma2, y, theta1_pars=None, theta2_pars=None, rng=None,
                 max_proposals=None, laplace=None, block=256, seg=2048, on_device=True, logpost_fn=None):
    """Metro_device_sets' C = 1 case: one chain on one training set -> Metro's result dict.  `logpost_fn(rows) -> (val, beta)`
    replaces the device evaluator (and keeps the chain on the host)."""
    fn = None if logpost_fn is None else (lambda rows, set_of: logpost_fn(rows))
    r = Metro_device_sets(gp, None if start is None else np.asarray(start, dtype=np.float64)[None], N, samp_size, batch_size,
                          alpha, [D_train], [sigma2], [y], theta1_pars, theta2_pars, [rng], max_proposals,
                          None if laplace is None else [laplace], block, seg, on_device, fn)
    return r["chains"][0]


def _twin_nm_segment(evaluate, owner, state, seg):
    """What one launch of laplace_search_sets does, on the host twin: every search of `state` [A, W] (changed in place) takes
    up to `seg` evaluations, all running searches' trial points in one evaluator call per step.  A search depends on its own
    evaluations only, so the cut into steps changes no bit.  Returns evals[A]."""
    A = state.shape[0]
    evals = np.zeros(A, dtype=np.int64)
    for _ in range(int(seg)):
        live = np.flatnonzero(state[:, api.NM_CODE] == api.NM_RUNNING)
        if live.size == 0:
            break
        val = np.asarray(evaluate(api.nm_trial(state[live]), owner[live])[0], dtype=np.float64)
        for k, a in enumerate(live):
            api.nm_feed(state[a], val[k])
        evals[live] += 1
    return evals


def laplace_device_sets(gp, D_trains, ys, sigma2s, starts, theta1_pars=None, theta2_pars=None, hess_step=1e-3, maxiter=2000,
                        on_device=True, seg=512, logpost_sets_fn=None):
    """laplace_sets over the twin evaluator (ccgp_chain_logpost_sets) with the Nelder-Mead search itself on the device: one
    launch of ccgp_laplace_search_sets carries every running search through up to `seg` evaluations (one workgroup per search:
    the chain instance's evaluation, the step of laplace_sets restated in csrc/nm_logic.h), until none is running; then the
    central-difference Hessian points of all sets go out as ONE ccgp_chain_logpost_sets call, as laplace_sets sends them.
    The search asks for one value at a time -- the reflection, then what the reflected value calls for -- where laplace_sets
    sends all four trial points of an iteration; its decisions are laplace_sets' decisions on the same values, so mode, var,
    converged, value and iterations are laplace_sets' bits, and `evaluations` is the count laplace_sets charges (p + 1, + 4
    per iteration, + p per shrink), which its maxiter rule reads.  starts is [C, p].
    on_device=False runs the same driver with every evaluation through the twin and every step through ccgp_nm_feed: the
    exact reference for the device search, and what the driver falls back to by itself where the device call says
    CCGP_EUNSUPPORTED (n > 128; the Matern and spline families, unless gp was made with fused=True and n <= 32).
    `logpost_sets_fn(rows, set_of) -> (val, beta)` replaces the
    twin evaluator and keeps the search on the host.
    Returns one dict per set with laplace_sets' keys, plus fed: the evaluations the search made, and calls: the launches the
    set took part in + 1 (on the twin: its evaluator calls + 1)."""
    starts = np.atleast_2d(np.asarray(starts, dtype=np.float64))
    C, p = starts.shape
    if C < 1 or len(D_trains) != C or len(ys) != C or len(sigma2s) != C:
        raise ValueError("laplace_device_sets: one design, response, sigma2 and start per set, at least one set")
    seg = int(seg)
    if seg < 1 or seg > api.NM_MAX_EVALS:
        raise ValueError("laplace_device_sets: seg must lie in 1 .. %d" % api.NM_MAX_EVALS)
    if int(maxiter) < 0:
        raise ValueError("laplace_device_sets: maxiter must not be negative")
    device = bool(on_device) and logpost_sets_fn is None
    if logpost_sets_fn is None:
        logpost_sets_fn = _twin_sets_evaluator(gp, D_trains, ys, sigma2s, theta1_pars, theta2_pars)
        q = 4 if gp.cfg["prior"] == api.PRIOR_ANI else 3
        if p != q:
            raise ValueError("laplace_device_sets: starts must be [C, %d] for this script" % q)

    def evaluate(rows, set_of):
        return logpost_sets_fn(np.asarray(rows), np.asarray(set_of, dtype=np.int64))

    if device:
        pars = _prior_pars(gp, theta1_pars, theta2_pars)
        Xs = np.stack([np.asarray(D, dtype=np.float64) for D in D_trains])
        Y = np.stack([np.asarray(y, dtype=np.float64).ravel() for y in ys])
    owner = np.arange(C)
    state = np.stack([api.nm_begin(x, 1e-6, 1e-9, maxiter) for x in starts])
    calls = np.zeros(C, dtype=np.int64)
    while True:
        live = np.flatnonzero(state[:, api.NM_CODE] == api.NM_RUNNING)
        if live.size == 0:
            break
        if device:
            try:
                r = gp.h.laplace_search_sets(Xs, Y, sigma2s, gp.cfg["prior"], owner[live], state[live], seg, pars)
            except api.CcgpError as e:
                if e.code != -4:   # CCGP_EUNSUPPORTED: this shape has no device search; the twin carries it
                    raise
                device = False
                continue
            state[live] = r["state"]
            calls[live] += 1
        else:
            sub = state[live]
            calls[live] += _twin_nm_segment(evaluate, owner[live], sub, seg)
            state[live] = sub
    modes = np.stack([api.nm_simplex(s)[0][0] for s in state])
    var = _hessian_vars(lambda rows, set_of: evaluate(rows, set_of)[0], modes, hess_step)
    return [dict(mode=modes[c].copy(), var=var[c], converged=bool(state[c, api.NM_CODE] == api.NM_CONVERGED),
                 value=float(api.nm_simplex(state[c])[1][0]), iterations=int(state[c, api.NM_ITERATIONS]),
                 evaluations=int(state[c, api.NM_CHARGED]), fed=int(state[c, api.NM_FED]), calls=int(calls[c]) + 1)
            for c in range(C)]


def laplace_device(gp, D_train, y, sigma2, start, theta1_pars=None, theta2_pars=None, hess_step=1e-3, maxiter=2000,
                   on_device=True, seg=512, logpost_fn=None):
    """laplace_device_sets' C = 1 case: one search on one training set -> its dict.  `logpost_fn(rows) -> (val, beta)`
    replaces the twin evaluator (and keeps the search on the host)."""
    fn = None if logpost_fn is None else (lambda rows, set_of: logpost_fn(rows))
    return laplace_device_sets(gp, [D_train], [y], [sigma2], np.asarray(start, dtype=np.float64)[None], theta1_pars,
                               theta2_pars, hess_step, maxiter, on_device, seg, fn)[0]


def factors_frame(gp, start, N, samp_size, batch_size, alpha_geweke, D_train, sigma2, y_train,
                  net_samp_size, theta1_pars=None, theta2_pars=None, rng=None, speculate=0):
    """HX:625-644 without materialising R.Inv per draw: returns the retained posterior draws
    (p, theta1, theta2[, lambda]) and their beta; the device recomputes the factor when predicting
    (rsurface.CombinedGP.factors_frame_from_draws builds the reference's wide frame on request)."""
    s = Metro(gp, start, N, samp_size, batch_size, alpha_geweke, D_train, sigma2, y_train, theta1_pars,
              theta2_pars, rng, speculate=speculate)
    keep = slice(samp_size - net_samp_size, samp_size)
    return dict(draws=transformed_to_draws(s["sample"][keep]), beta=s["beta"][keep], chain=s)


# ----------------------------------------------------------------------------- prediction / compare.GP
def _add_cgp_columns(table, gp, D_test, D_train, y_train, cgp):
    """compare.GP's CGP columns (GV:654-660): CGP(D.train, y.train), then predict.CGP(cgp, D.test, PI = TRUE)."""
    from . import cgp as cgp_mod
    if isinstance(cgp, dict) and "est" in cgp:
        est = cgp["est"]   # a fitted model (cgp.CGP's or cgp.CGP_sets' dict): nothing is fitted here
    else:
        est = cgp_mod.CGP(gp.h, D_train, y_train, **(cgp if isinstance(cgp, dict) else {}))
    pred = cgp_mod.predict_CGP(gp.h, est, D_test, PI=True)
    table.update(y_hat_CGP=pred["Yp"], LL_CGP=pred["Y_low"], UL_CGP=pred["Y_up"], CGP=est)
    return table


def _t_interval(y_hat, var, alpha, n):
    """y_hat -+ qt(1 - alpha / 2, n - 1) sqrt(max(var, 0)): the interval of both single-GP forms."""
    from scipy.stats import t as student_t
    delta = student_t.ppf(1.0 - alpha / 2.0, n - 1) * np.sqrt(np.maximum(var, 0.0))
    return y_hat - delta, y_hat + delta


def prediction_single(handle, D_train, D_new, y_train, MLE, alpha, nu=None, fused_predict=False):
    """prediction.single of the 1-D scripts (D1:548-567 = D1F:872-889) on the device: y.hat.single, and LL / UL.Single with
    single.var from CIs.single (D1:527-539), whose post.stdev.single^2 = Q / (n - 1) post.var.single / sigma2 (D1:504-516) is
    ccgp_krige_predict_batch's VAR_UNBIASED.  With nu: one Matern(nu) component at the scalar MLE["theta"] (what matern_MLEs
    returns).  Without: a Gaussian single GP whose MLE["theta"] holds d scales (ordinary_kriging_fit's).  beta is the
    profile beta at theta, as MLEs() forms it (D1:467).  fused_predict=True (with nu): the call runs with
    OPT_FAMILY_FUSED_PREDICT on (n <= 32: the register-resident evaluator in place of the blocked sweep, equal to rounding).
    Returns dict(y_hat_single, LL_single, UL_single, single_var)."""
    D = np.asarray(D_train, dtype=np.float64)
    D = D.reshape(-1, 1) if D.ndim == 1 else D
    Dn = np.asarray(D_new, dtype=np.float64).reshape(-1, D.shape[1])
    y = np.asarray(y_train, dtype=np.float64).ravel()
    theta = np.atleast_1d(np.asarray(MLE["theta"], dtype=np.float64)).ravel()
    if theta.size != D.shape[1]:
        raise ValueError("MLE['theta'] must hold one scale per input dimension")
    h = handle
    if nu is not None:
        from .rsurface import _FamilyHandle
        h = _FamilyHandle(getattr(handle, "_handle", handle), api.KERNEL_MATERN, float(nu), fused_predict=fused_predict)
    mean, var, _, _, st = h.krige_predict_batch(D, y, 1, np.concatenate([[1.0], theta])[None], None, Dn, api.VAR_UNBIASED)
    if st[0] != 0:
        raise RuntimeError("prediction_single: the correlation matrix could not be factorised (pivot %d)" % st[0])
    lo, hi = _t_interval(mean[0], var[0], alpha, D.shape[0])
    return dict(y_hat_single=mean[0].copy(), LL_single=lo, UL_single=hi, single_var=var[0].copy())


def _single_model(gp, D_train, y_train, single):
    """The single-GP comparator of compare_GP and leave_one_out: the model `single` gives (theta, sigma2[, beta], or est = a
    fit routine's dict, which goes into the table as it is) or, without one, the fit on the device (matern_MLEs for a 1-D gp,
    ordinary_kriging_fit otherwise; further keys of `single` go to it).  Returns (model, handle, D, sigma2 argument,
    variance form): the 1-D scripts take the unbiased form under the Matern family, the others the plug-in form.  A 1-D gp
    made with fused_predict=True hands that on to the single GP's handle."""
    base = getattr(gp.h, "_handle", gp.h)
    given = dict(single) if isinstance(single, dict) else {}
    model = {k: given.pop(k) for k in ("theta", "sigma2", "beta") if k in given}
    if "est" in given:
        model = given.pop("est")
    if hasattr(gp, "nu"):
        from .rsurface import _FamilyHandle
        D = np.asarray(D_train, dtype=np.float64).reshape(-1, 1)
        if "theta" not in model:
            model = matern_MLEs(base, D, y_train, gp.nu, **given)
        h = _FamilyHandle(base, api.KERNEL_MATERN, float(gp.nu), fused_predict=getattr(gp, "fused_predict", False))
        return model, h, D, None, api.VAR_UNBIASED
    D = np.asarray(D_train, dtype=np.float64)
    if "theta" not in model or "sigma2" not in model:
        model = ordinary_kriging_fit(base, D, y_train, **given)
    return model, base, D, [model["sigma2"]], api.VAR_PLUGIN


def _add_single_columns(table, gp, D_test, alpha, D_train, y_train, single):
    """compare.GP's single-GP columns.  The 2-D / emulator scripts: mlegp + predict.gp(se.fit = TRUE), fit -+ se.fit
    qt(1 - alpha / 2, n - 1) (GV:662-666, ANI:679-683, ISO:665-669, ADV:733-737, BSQ:664-668) -- the plug-in variance.  The
    1-D scripts: MLEs() + prediction.single (D1:548-567) -- the unbiased form, which also gives single_var."""
    model, h, D, s2, form = _single_model(gp, D_train, y_train, single)
    if hasattr(gp, "nu"):   # h is the Matern(nu) handle already
        table.update(prediction_single(h, D, np.asarray(D_test, dtype=np.float64).reshape(-1, 1), y_train, model, alpha))
        table["single"] = model
        return table
    theta = np.asarray(model["theta"], dtype=np.float64).ravel()
    mean, var, _, _, st = h.krige_predict_batch(D, y_train, 1, np.concatenate([[1.0], theta])[None], s2, D_test, form)
    if st[0] != 0:
        raise RuntimeError("compare_GP: the single GP's correlation matrix could not be factorised (pivot %d)" % st[0])
    lo, hi = _t_interval(mean[0], var[0], alpha, D.shape[0])
    table.update(y_hat_single=mean[0].copy(), LL_single=lo, UL_single=hi, single=model)
    return table


def _cgp_on_device(cgp, device_cgp):
    """The cgp argument with device_cgp folded in: a fit that is still to be made gets on_device=True."""
    if not device_cgp or not cgp or (isinstance(cgp, dict) and "est" in cgp):
        return cgp
    return dict(cgp if isinstance(cgp, dict) else {}, on_device=True)


def compare_GP(gp, D_test, alpha, y_test, draws, D_train, sigma2, y_train, rng=None, exact=False, cgp=False, single=False,
               device_cgp=False):
    """HX:713-725 + prediction HX:686-703 (GV:620-646 adds Quant.Combined): one row per test point
    (y.hat.Combined, Quant.Combined, LL.Combined, UL.Combined, y.true).  exact=True takes Quant and the interval from
    the exact posterior predictive on the device (gp.prediction) instead of sampling one variate per draw: rng is
    ignored, the tables stay on the device, and the keys are the same without mean / var.  cgp (default off; True, or a dict
    of cgp.CGP's keyword arguments) adds the table's CGP model (GV:654-660): y_hat_CGP, LL_CGP, UL_CGP and the fit as CGP;
    cgp=dict(est=<a dict of cgp.CGP or cgp.CGP_sets>) takes a fitted model instead of fitting.  device_cgp (default off): that
    fit's refinement runs on the device (cgp.CGP(on_device=True)): the same model bit for bit.
    single (default off) adds the ordinary-kriging model: True fits it on the device (ordinary_kriging_fit; for a 1-D gp
    matern_MLEs), a dict(theta=..., sigma2=...) or dict(est=<a dict of ordinary_kriging_fit>) takes a given model, and
    further keys go to the fit.  It adds y_hat_single,
    LL_single, UL_single = y_hat -+ qt(1 - alpha / 2, n - 1) sqrt(max(var, 0)) -- var in the plug-in form for the 2-D /
    emulator scripts, in the unbiased form (and returned as single_var) for the 1-D scripts -- and the model as single."""
    if single:
        table = compare_GP(gp, D_test, alpha, y_test, draws, D_train, sigma2, y_train, rng, exact, cgp, device_cgp=device_cgp)
        return _add_single_columns(table, gp, D_test, alpha, D_train, y_train, single)
    if cgp:
        table = compare_GP(gp, D_test, alpha, y_test, draws, D_train, sigma2, y_train, rng, exact)
        return _add_cgp_columns(table, gp, D_test, D_train, y_train, _cgp_on_device(cgp, device_cgp))
    if exact:
        r = gp.prediction(D_test, alpha, draws, D_train, sigma2, y_train)
        return dict(y_hat=r["y_hat"], quant=r["Quant"], LL=r["LL"], UL=r["UL"],
                    y_true=np.asarray(y_test, dtype=np.float64))
    rng = np.random.default_rng(rng)
    t = gp.prediction_table(D_test, draws, D_train, sigma2, y_train)
    mean, var = t["mean"], t["var"]                      # [S, m]
    y_hat = mean.mean(axis=0)
    post = rng.normal(mean, np.sqrt(np.maximum(var, 0.0)))
    lo = np.quantile(post, alpha / 2.0, axis=0)
    hi = np.quantile(post, 1.0 - alpha / 2.0, axis=0)
    quant = (y_hat[None, :] <= post).mean(axis=0)
    return dict(y_hat=y_hat, quant=quant, LL=lo, UL=hi, y_true=np.asarray(y_test, dtype=np.float64),
                mean=mean, var=var)


def _fitted(arg):
    """The fitted model in a comparator argument of compare_GP (dict(est=...)), or None."""
    return arg["est"] if isinstance(arg, dict) and "est" in arg else None


def compare_GP_sets(gp, D_tests, alpha, y_tests, draws, D_trains, sigma2s, y_trains, cgp=None, single=None, counts=None):
    """compare_GP(..., exact=True, cgp=..., single=...) for many training sets at once: the list of its tables, set by set,
    equal in every key and bit.  The sets are grouped by (n, d, m) -- ragged test sets make one call per m -- and a group's
    Combined-GP columns come from ONE device call (gp.prediction_sets), its single-GP columns from one
    (krige_predict_batch_sets) and its CGP columns from one (cgp.predict_CGP_sets).  cgp / single: per-set lists of fitted
    models, dict(est=<a dict of cgp.CGP / cgp.CGP_sets>) and dict(est=<a dict of ordinary_kriging_fit>) -- nothing is fitted
    here; None (or a list of None) leaves the columns out, and a set whose entry is anything else (True, fit keywords)
    falls back to compare_GP for that set.  counts (a dict, optional): counts["calls"] receives the device calls made."""
    from . import cgp as cgp_mod
    C = len(D_trains)
    cgp = list(cgp) if cgp is not None else [None] * C
    single = list(single) if single is not None else [None] * C
    base = getattr(gp.h, "_handle", gp.h)
    tables, calls = [None] * C, 0
    groups = {}
    for i in range(C):
        ready = all(not arg or _fitted(arg) is not None for arg in (cgp[i], single[i]))
        if not ready or hasattr(gp, "nu"):   # a model still to be fitted, or a 1-D gp: the per-set path
            tables[i] = compare_GP(gp, D_tests[i], alpha, y_tests[i], draws[i], D_trains[i], sigma2s[i], y_trains[i], exact=True,
                                   cgp=cgp[i] or False, single=single[i] or False)
            calls += 1 + bool(cgp[i]) + bool(single[i])
            continue
        key = np.shape(D_trains[i]) + (np.atleast_2d(np.asarray(D_tests[i], dtype=np.float64)).shape[0],)
        groups.setdefault(key, []).append(i)
    for (n, d, m), idx in groups.items():
        Dt = [np.asarray(D_tests[i], dtype=np.float64).reshape(m, d) for i in idx]
        Dn = [np.asarray(D_trains[i], dtype=np.float64) for i in idx]
        yn = [np.asarray(y_trains[i], dtype=np.float64).ravel() for i in idx]
        pred = gp.prediction_sets(Dt, alpha, [draws[i] for i in idx], Dn, [sigma2s[i] for i in idx], yn)
        calls += 1
        for i, r in zip(idx, pred):
            tables[i] = dict(y_hat=r["y_hat"], quant=r["Quant"], LL=r["LL"], UL=r["UL"],
                             y_true=np.asarray(y_tests[i], dtype=np.float64))
        # the comparators in compare_GP's order: CGP first, then the single GP
        with_cgp = [j for j, i in enumerate(idx) if cgp[i]]
        if with_cgp:
            ests = [_fitted(cgp[idx[j]]) for j in with_cgp]
            preds = cgp_mod.predict_CGP_sets(gp.h, ests, [Dt[j] for j in with_cgp], PI=True)
            calls += 1   # the group's models have one shape and one m: predict_CGP_sets makes one call
            for j, est, p in zip(with_cgp, ests, preds):
                tables[idx[j]].update(y_hat_CGP=p["Yp"], LL_CGP=p["Y_low"], UL_CGP=p["Y_up"], CGP=est)
        with_single = [j for j, i in enumerate(idx) if single[i]]
        if with_single:
            models = [_fitted(single[idx[j]]) for j in with_single]
            rows = np.stack([np.concatenate([[1.0], np.asarray(mo["theta"], dtype=np.float64).ravel()]) for mo in models])
            mean, var, _, _, st = base.krige_predict_batch_sets(np.stack([Dn[j] for j in with_single]),
                                                                np.stack([yn[j] for j in with_single]), 1, rows,
                                                                np.arange(len(models)), [mo["sigma2"] for mo in models],
                                                                np.stack([Dt[j] for j in with_single]), api.VAR_PLUGIN)
            calls += 1
            if st.any():
                raise RuntimeError("compare_GP_sets: the single GP's correlation matrix could not be factorised (pivot %d)"
                                   % st[np.flatnonzero(st)[0]])
            for k, (j, mo) in enumerate(zip(with_single, models)):
                lo, hi = _t_interval(mean[k], var[k], alpha, n)
                tables[idx[j]].update(y_hat_single=mean[k].copy(), LL_single=lo, UL_single=hi, single=mo)
    if counts is not None:
        counts["calls"] = counts.get("calls", 0) + calls
    return tables


def _add_single_loo_columns(table, gp, alpha, D_train, y_train, single):
    """leave_one_out's single-GP columns: the model as _add_single_columns takes or fits it (ONCE, on all n points: the
    parameters stay fixed across the folds, as for the Combined GP's draws), then one ccgp_loo_batch row with K = 1 -- the
    plug-in variance for the 2-D / emulator scripts, the unbiased form for the 1-D scripts -- and the interval
    y_hat -+ qt(1 - alpha / 2, n - 2) sqrt(max(var, 0)): a fold has n - 1 points."""
    y = np.asarray(y_train, dtype=np.float64).ravel()
    model, h, D, s2, form = _single_model(gp, D_train, y, single)
    theta = np.atleast_1d(np.asarray(model["theta"], dtype=np.float64)).ravel()
    if theta.size != D.shape[1]:
        raise ValueError("the single GP's theta must hold one scale per input dimension")
    mean, var, _, _, st = h.loo_batch(D, y, 1, np.concatenate([[1.0], theta])[None], s2, form)
    if st[0] != 0:
        raise RuntimeError("leave_one_out: the single GP's correlation matrix could not be factorised (pivot %d)" % st[0])
    lo, hi = _t_interval(mean[0], var[0], alpha, D.shape[0] - 1)
    table.update(y_hat_single=mean[0].copy(), LL_single=lo, UL_single=hi, single=model)
    if hasattr(gp, "nu"):
        table["single_var"] = var[0].copy()
    return table


def leave_one_out(gp, alpha, draws, D_train, sigma2, y_train, single=False):
    """compare_GP(exact=True)'s table with the training points as their own test set: row i is the exact posterior
    predictive of y_i given the n - 1 other points under the posterior draws (gp.leave_one_out: one factorisation per draw,
    no refitting), y_true = y_train.  comparison_summary of it gives the Combined GP's leave-one-out RMSPE (what GV:199 calls
    rmscv for the CGP), interval coverage and mean quantile without a held-out set; `pit` holds F(y_i).  single as in
    compare_GP (True fits; a dict(theta=..., sigma2=...) or dict(est=<a dict of ordinary_kriging_fit>) gives the model) adds
    y_hat_single, LL_single, UL_single.  No CGP columns: its jackknife is
    cgp.CGP's Yjfp / rmscv and has no interval in the reference."""
    r = gp.leave_one_out(alpha, draws, D_train, sigma2, y_train)
    table = dict(y_hat=r["y_hat"], quant=r["Quant"], LL=r["LL"], UL=r["UL"],
                 y_true=np.asarray(y_train, dtype=np.float64).ravel(), pit=r["pit"])
    if single:
        _add_single_loo_columns(table, gp, alpha, D_train, y_train, single)
    return table


def _q_logdet_beta(h, D, y, rows):
    """(Q, log det R, beta, ok) per parameter row, Q = (y - beta)' R^-1 (y - beta), from two likelihood calls that differ in
    sigma2 only: ll(s) = -(n log 2pi + n log s + logdet + Q / s) / 2 at s = 1 and s = e.  ok: the row was factorised."""
    n = D.shape[0]
    a, beta, st = h.loglik_batch(D, y, 1, rows, 1.0)
    b, _, _ = h.loglik_batch(D, y, 1, rows, math.e)
    Q = (n - 2.0 * (a - b)) / (1.0 - 1.0 / math.e)
    return Q, -2.0 * a - n * math.log(2 * math.pi) - Q, beta, (st == 0) & np.isfinite(a)


def ordinary_kriging_sigma2(handle, D_train, y_train, starts=8, rng=0):
    """sigma2 of the ordinary-kriging MLE with one anisotropic Gaussian kernel -- what the scripts
    take from mlegp (`ord$sig2`, HX:759-760).  Deterministic multi-start L-BFGS on the concentrated
    log-likelihood using the device likelihood and its analytic gradient.  The surface is multimodal:
    on the Qian set 3 starts stop at sigma2 = 90.5 (log-lik -122.65), 8 starts find sigma2 = 64.2
    (-117.10), and only the latter makes the hyperprior grid pick the pair hard-coded at HX:774-775
    (tests/test_reference_pins_gpu.py).  mlegp itself restarts a randomised simplex and can stop short of
    the optimum (Ground-Vibrations set: its recorded fit has log-lik -112.79, this routine -110.37).
    Returns (sigma2, theta[d], beta)."""
    from scipy.optimize import minimize

    D = np.asarray(D_train, dtype=np.float64)
    y = np.asarray(y_train, dtype=np.float64).ravel()
    n, d = D.shape
    span = np.maximum(D.max(axis=0) - D.min(axis=0), 1e-12)

    def parts(theta):
        Q, logdet, beta, ok = _q_logdet_beta(handle, D, y, np.concatenate([[1.0], theta])[None])
        return (max(Q[0], 1e-300), logdet[0], beta[0]) if ok[0] else None

    def f(logth):
        theta = np.exp(logth)
        pr = parts(theta)
        if pr is None:
            return 1e300, np.zeros(d)
        Q, logdet, _ = pr
        s2 = Q / n
        val = -0.5 * (n * math.log(2 * math.pi) + n * math.log(s2) + logdet + n)
        _, _, g, st = handle.loglik_grad_batch(D, y, 1, np.concatenate([[1.0], theta])[None], s2)
        if st[0] != 0:
            return 1e300, np.zeros(d)
        return -val, -(g[0, 1:] * theta)                              # envelope theorem; chain rule to log theta

    best = None
    gen = np.random.default_rng(rng)
    for s in range(starts):
        x0 = np.log((1.0 if s == 0 else gen.uniform(0.2, 5.0, size=d)) / span ** 2)
        res = minimize(f, x0, jac=True, method="L-BFGS-B", bounds=[(-12.0, 12.0)] * d)
        if best is None or res.fun < best.fun:
            best = res
    theta = np.exp(best.x)
    Q, _, beta = parts(theta)
    return Q / n, theta, beta


def matern_MLEs(handle, D, y, nu, grid=96, lo=1e-3, hi=1e2, fused=False):
    """MLEs(D, y, nu) of the 1-D scripts (D1:455-471 = D1F:547-566): ordinary kriging with ONE Matern(nu) component;
    theta minimises log.likeli = log det R(theta) + n log sigma2.MLE(theta) (D1:424-444), then beta.MLE and sigma2.MLE
    at that theta (D1:467-468).  Combined.GP.fit feeds this sigma2 to the Combined-GP path (D1:994-995).

    The reference starts nlminb at runif(1) and retries until solve() succeeds; the optimiser's path is not
    reproducible (R's RNG), its optimum is.  Here the batched device likelihood (ccgp_loglik_batch, K = 1, Matern
    family) evaluates a log-spaced grid of `grid` scale parameters (scaled by the design's range) in two calls, which
    brackets the global minimum; a bounded scalar search refines it inside the bracket.  fused=True: the calls run with
    OPT_FAMILY_FUSED on (n <= 32: the register-resident evaluator in place of the blocked sweep, equal to rounding).
    Returns dict(beta, sigma2, theta)."""
    from scipy.optimize import minimize_scalar
    from . import api
    from .rsurface import _FamilyHandle

    D = np.asarray(D, dtype=np.float64).reshape(-1, 1)
    y = np.asarray(y, dtype=np.float64).ravel()
    n = D.shape[0]
    h = _FamilyHandle(handle, api.KERNEL_MATERN, float(nu), fused)
    span = max(float(D.max() - D.min()), 1e-12)

    def parts(thetas):
        """(Q, logdet, beta) per theta, NaN where the row failed or Q is not positive."""
        Q, logdet, beta, ok = _q_logdet_beta(h, D, y, np.stack([np.ones_like(thetas), thetas], axis=1))
        bad = ~ok | ~(Q > 0)
        return np.where(bad, np.nan, Q), np.where(bad, np.nan, logdet), beta

    def objective(thetas):
        Q, logdet, _ = parts(np.atleast_1d(np.asarray(thetas, dtype=np.float64)))
        with np.errstate(invalid="ignore", divide="ignore"):
            return logdet + n * np.log(Q / n)

    th = span * np.exp(np.linspace(math.log(lo), math.log(hi), grid))
    f = objective(th)
    if not np.isfinite(f).any():
        raise RuntimeError("matern_MLEs: the likelihood failed at every scale parameter of the search grid")
    i = int(np.nanargmin(f))
    a = th[max(i - 1, 0)]
    b = th[min(i + 1, grid - 1)]
    res = minimize_scalar(lambda t: float(np.nan_to_num(objective(math.exp(t))[0], nan=1e300)),
                          bounds=(math.log(a), math.log(b)), method="bounded", options=dict(xatol=1e-10))
    theta = math.exp(res.x) if res.fun <= f[i] else float(th[i])
    Q, _, beta = parts(np.array([theta]))
    return dict(beta=float(beta[0]), sigma2=float(Q[0] / n), theta=float(theta))


def matern_MLEs_sets(handle, Ds, ys, nu, grid=96, lo=1e-3, hi=1e2):
    """matern_MLEs for C designs of one shape in lockstep, on the analytic gradient of the Matern(nu) family
    (OPT_FAMILY_FUSED_GRAD, which this function sets for its own calls: d = 1, n <= 32).

    1. ONE profile_batch_sets(grad=True) call with C x grid rows: matern_MLEs' own grid for every set (log-spaced, scaled
       by the set's range).  2. Per set the grid's best point and its two neighbours are three starts of
    design.minimize_starts in log theta, each under the bracket [left neighbour, right neighbour] as its own box; the
    objective is -l_p and its gradient -g_theta theta (chain rule to log theta; g_theta is the gradient at the point's own
    (beta, sigma2): envelope theorem).  All sets run in lockstep: each step is ONE sets call carrying every start still
    running.  3. One final sets call at the C best points.  A start's trajectory depends on its own evaluations only and a
    row's bits on its own set only, so a set's result is the one it has alone.

    Returns, per set, dict(beta, sigma2, theta, loglik, calls) -- loglik the profiled log-likelihood l_p at theta, calls the
    device calls the set took part in (grid and final call included); the group made max(calls) of them.  Sets of one
    shape only (ValueError otherwise); a set whose likelihood fails on the whole grid raises RuntimeError."""
    from .design import minimize_starts
    from .rsurface import _FamilyHandle

    Ds = [np.asarray(D, dtype=np.float64).reshape(-1, 1) for D in Ds]
    ys = [np.asarray(y, dtype=np.float64).ravel() for y in ys]
    C = len(Ds)
    if C < 1 or len(ys) != C:
        raise ValueError("matern_MLEs_sets: one response per design, at least one set")
    if any(D.shape != Ds[0].shape for D in Ds) or any(y.shape[0] != Ds[0].shape[0] for y in ys):
        raise ValueError("matern_MLEs_sets: the sets of one call have one shape")
    grid = int(grid)
    h = _FamilyHandle(handle, api.KERNEL_MATERN, float(nu), fused_grad=True)
    Xs, Y = np.stack(Ds), np.stack(ys)

    def profile(thetas, set_of):
        rows = np.stack([np.ones_like(thetas), thetas], axis=1)
        return h.profile_batch_sets(Xs, Y, 1, rows, np.asarray(set_of, dtype=np.int32), grad=True)

    spans = np.array([max(float(D.max() - D.min()), 1e-12) for D in Ds])
    th = spans[:, None] * np.exp(np.linspace(math.log(lo), math.log(hi), grid))[None, :]
    ll, _, _, _, st = profile(th.ravel(), np.repeat(np.arange(C), grid))
    f = np.where((st == 0) & np.isfinite(ll), -ll, np.nan).reshape(C, grid)
    x0, lows, ups = [], [], []
    for c in range(C):
        if not np.isfinite(f[c]).any():
            raise RuntimeError("matern_MLEs_sets: the likelihood failed at every scale parameter of the search grid of set %d" % c)
        i = int(np.nanargmin(f[c]))
        a, b = max(i - 1, 0), min(i + 1, grid - 1)
        x0 += [math.log(th[c, i]), math.log(th[c, a]), math.log(th[c, b])]
        lows += [math.log(th[c, a])] * 3
        ups += [math.log(th[c, b])] * 3
    owner = np.repeat(np.arange(C), 3)

    def evaluate(logth, live):
        theta = np.exp(logth[:, 0])
        ll, _, _, g, st = profile(theta, owner[live])
        return -ll, -(g[:, 1:] * theta[:, None]), st

    def col(v):
        return np.asarray(v, dtype=np.float64)[:, None]

    res = minimize_starts(evaluate, col(x0), lowers=col(lows), uppers=col(ups), pass_live=True)
    best = []
    for c in range(C):
        fs = res["f"][3 * c:3 * c + 3]
        best.append(3 * c + int(np.argmin(np.where(np.isfinite(fs), fs, np.inf))))
    thetas = np.exp(res["x"][best, 0])
    ll, s2, beta, _, _ = profile(thetas, np.arange(C))
    return [dict(beta=float(beta[c]), sigma2=float(s2[c]), theta=float(thetas[c]), loglik=float(ll[c]),
                 calls=int(res["calls_per_start"][3 * c:3 * c + 3].max()) + 2) for c in range(C)]


def kriging_starts(D_train, starts=8, rng=0, extra_starts=None):
    """The start points of ordinary_kriging_sigma2 as rows of log theta -- the same generator drawn in the same order: start 0
    is 1 / span^2, the others uniform(0.2, 5) / span^2 -- with `extra_starts` (rows of theta) appended."""
    D = np.asarray(D_train, dtype=np.float64)
    d = D.shape[1]
    span = np.maximum(D.max(axis=0) - D.min(axis=0), 1e-12)
    gen = np.random.default_rng(rng)
    rows = [np.log((1.0 if s == 0 else gen.uniform(0.2, 5.0, size=d)) / span ** 2) * np.ones(d) for s in range(starts)]
    if extra_starts is not None:
        rows += [np.log(t) for t in np.atleast_2d(np.asarray(extra_starts, dtype=np.float64))]
    return np.stack(rows)


def ordinary_kriging_fit(handle, D_train, y_train, starts=8, rng=0, extra_starts=None):
    """The ordinary-kriging MLE with one anisotropic Gaussian kernel (`mlegp(...)$sig2`, HX:759-760; the 1-D scripts' MLEs,
    D1:455-471) with the whole objective on the device: ccgp_profile_batch returns the likelihood with sigma2 concentrated
    out, sigma2 itself and the gradient from ONE factorisation per point, and design.minimize_starts drives all starts in
    lockstep, so every evaluator call is one device call that carries every start still running.

    Variables: log theta in [-12, 12]^d; objective -l_p, gradient -g_theta theta (chain rule to log theta; g_theta is the
    mode-0 gradient at the point's own (beta, sigma2): envelope theorem).  Starts: kriging_starts -- those of
    ordinary_kriging_sigma2, then `extra_starts` (rows of theta).  Returns dict(sigma2, theta[d], beta, loglik of the best
    start -- sigma2, beta and loglik as a final value-only call at theta gives them -- f[S], x[S, d] (log theta) and converged[S]
    per start, calls: the number of profile_batch calls, the final one included, and evaluations: the points they carried)."""
    D = np.asarray(D_train, dtype=np.float64)
    y = np.asarray(y_train, dtype=np.float64).ravel()

    def profile(rows, set_of, grad):
        ll, s2, beta, g, st = handle.profile_batch(D, y, 1, rows, grad=grad)
        return (ll, g, st) if grad else (ll, s2, beta)

    return _kriging_fit_sets("ordinary_kriging_fit", "", profile, [D], [rng], starts, extra_starts)[0]


def _kriging_fit_sets(who, of_set, profile, Ds, seeds, starts, extra_starts):
    """The lockstep fit behind ordinary_kriging_fit (C = 1) and ordinary_kriging_fit_sets: the kriging_starts of every set
    through ONE design.minimize_starts, then one value-only call at the C best points.  profile(rows, set_of, grad)
    evaluates row b on set set_of[b] -> (ll, gradient, status) with grad, (ll, sigma2, beta) without.  who and of_set (a format of
    the set's index, or empty) word the error.  Returns one dict per set."""
    from .design import minimize_starts

    C = len(Ds)
    x0 = [kriging_starts(Ds[c], starts, seeds[c], extra_starts) for c in range(C)]
    S = x0[0].shape[0]
    owner = np.repeat(np.arange(C), S)
    points = np.zeros(C, dtype=np.int64)

    def evaluate(logth, live):
        theta = np.exp(logth)
        ll, g, st = profile(np.concatenate([np.ones((theta.shape[0], 1)), theta], axis=1), owner[live], True)
        np.add.at(points, owner[live], 1)
        return -ll, -(g[:, 1:] * theta), st

    res = minimize_starts(evaluate, np.concatenate(x0), lower=-12.0, upper=12.0, pass_live=True)
    best = []
    for c in range(C):
        f = res["f"][c * S:(c + 1) * S]
        if not np.isfinite(f).any():
            raise RuntimeError("%s: the likelihood failed at every start%s" % (who, of_set and of_set % c))
        best.append(c * S + int(np.argmin(np.where(np.isfinite(f), f, np.inf))))
    thetas = np.exp(res["x"][best])
    ll, s2, beta = profile(np.concatenate([np.ones((C, 1)), thetas], axis=1), np.arange(C), False)
    out = []
    for c in range(C):
        sl = slice(c * S, (c + 1) * S)
        out.append(dict(sigma2=float(s2[c]), theta=thetas[c], beta=float(beta[c]), loglik=float(ll[c]), f=res["f"][sl],
                        x=res["x"][sl], converged=res["converged"][sl], calls=int(res["calls_per_start"][sl].max()) + 1,
                        evaluations=int(points[c]) + 1))
    return out


def ordinary_kriging_fit_sets(handle, D_trains, y_trains, starts=8, rng=0, extra_starts=None):
    """ordinary_kriging_fit for C training sets of one shape in lockstep -> a list with, per set, the dict
    ordinary_kriging_fit(handle, D_trains[c], y_trains[c], starts, rng, extra_starts) returns, bit for bit.

    Every set draws its kriging_starts from its own generator (rng: one seed for every set, as C separate fits would take
    it, or a list of C).  The starts of all sets run through ONE design.minimize_starts, and each evaluator call is ONE
    ccgp_profile_batch_sets that carries every start of every set still running; the final value-only evaluation of the C
    best points is one call of the value-only form.  Starts are independent of each other -- a start's trajectory depends on
    its own evaluations only, and a row's bits on its own set only -- so a set's starts take the steps they take alone, and
    the number of gradient calls of the group is the LARGEST per-set count, not the sum.  Each dict's calls / evaluations
    are that set's own (the calls its starts took part in, the final one included): the group made max(calls) device
    calls."""
    Ds = [np.asarray(D, dtype=np.float64) for D in D_trains]
    ys = [np.asarray(y, dtype=np.float64).ravel() for y in y_trains]
    C = len(Ds)
    if C < 1 or len(ys) != C:
        raise ValueError("ordinary_kriging_fit_sets: one response per design, at least one set")
    if any(D.ndim != 2 or D.shape != Ds[0].shape for D in Ds) or any(y.shape[0] != Ds[0].shape[0] for y in ys):
        raise ValueError("ordinary_kriging_fit_sets: the sets of one call have one shape (n, d)")
    seeds = list(rng) if isinstance(rng, (list, tuple)) else [rng] * C
    if len(seeds) != C:
        raise ValueError("ordinary_kriging_fit_sets: rng is one seed, or one per set")
    Xs, Y = np.stack(Ds), np.stack(ys)

    def profile(rows, set_of, grad):
        ll, s2, beta, g, st = handle.profile_batch_sets(Xs, Y, 1, rows, set_of, grad=grad)
        return (ll, g, st) if grad else (ll, s2, beta)

    return _kriging_fit_sets("ordinary_kriging_fit_sets", " of set %d", profile, Ds, seeds, starts, extra_starts)


def _twin_fit_segment(handle, Xs, Y, owner, state, seg):
    """What one launch of profile_fit_sets does, on the host twin: every start of `state` [A, W] (changed in place) takes up to
    `seg` evaluations, all running starts' trial points in one profile_fit_eval_sets call per step.  A start depends on its
    own evaluations only, so the cut into steps changes no bit.  Returns evals[A]."""
    from . import api

    A = state.shape[0]
    evals = np.zeros(A, dtype=np.int64)
    for _ in range(int(seg)):
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        f, g, _, _, _, st = handle.profile_fit_eval_sets(Xs, Y, api.fit_trial(state[live]), owner[live])
        for k, a in enumerate(live):
            api.fit_feed(state[a], f[k], g[k], st[k] == 0)
        evals[live] += 1
    return evals


def ordinary_kriging_fit_device_sets(handle, D_trains, y_trains, starts=8, rng=0, extra_starts=None, on_device=True, seg=512):
    """ordinary_kriging_fit_sets with the quasi-Newton iteration itself on the device: one launch of ccgp_profile_fit_sets
    carries every running start of every set through up to `seg` evaluations (one workgroup per start: the profiled-gradient
    instance, the step of design._Start restated in csrc/fit_logic.h), until none is running; then one value-only
    ccgp_profile_fit_eval_sets at the C best points.  Starts: kriging_starts under the bounds [-12, 12], as
    ordinary_kriging_fit_sets draws them (rng: one seed for every set, or a list of C).

    The fit has a contract of its own: theta = exp(log theta) comes from the portable exp the kernel runs, not numpy's, so
    it is the same method and the same optimum as ordinary_kriging_fit, not its bits.  What it keeps bit for bit is its host
    twin: on_device=False runs the same driver with every evaluation through ccgp_profile_fit_eval_sets and every step
    through ccgp_fit_feed, and leaves the same states.  The driver falls back to the twin by itself where the device call
    says CCGP_EUNSUPPORTED (n > 128, the Matern and spline families).

    Returns one dict per set with ordinary_kriging_fit_sets' keys: sigma2, theta[d], beta, loglik of the best start (as the
    final value-only call gives them), f[S], x[S, d], converged[S], calls = launches + 1 (on the twin: the evaluator calls
    the set's starts took part in, + 1), evaluations = the points evaluated on the set, the final one included."""
    from . import api

    Ds = [np.asarray(D, dtype=np.float64) for D in D_trains]
    ys = [np.asarray(y, dtype=np.float64).ravel() for y in y_trains]
    C = len(Ds)
    if C < 1 or len(ys) != C:
        raise ValueError("ordinary_kriging_fit_device_sets: one response per design, at least one set")
    if any(D.ndim != 2 or D.shape != Ds[0].shape for D in Ds) or any(y.shape[0] != Ds[0].shape[0] for y in ys):
        raise ValueError("ordinary_kriging_fit_device_sets: the sets of one call have one shape (n, d)")
    seeds = list(rng) if isinstance(rng, (list, tuple)) else [rng] * C
    if len(seeds) != C:
        raise ValueError("ordinary_kriging_fit_device_sets: rng is one seed, or one per set")
    seg = int(seg)
    if seg < 1 or seg > api.FIT_MAX_EVALS:
        raise ValueError("ordinary_kriging_fit_device_sets: seg must lie in 1 .. %d" % api.FIT_MAX_EVALS)
    Xs, Y = np.stack(Ds), np.stack(ys)
    x0 = np.concatenate([kriging_starts(Ds[c], starts, seeds[c], extra_starts) for c in range(C)])
    S = x0.shape[0] // C
    owner = np.repeat(np.arange(C), S)
    state = np.stack([api.fit_begin(x, -12.0, 12.0) for x in x0])
    evals = np.zeros(C * S, dtype=np.int64)
    calls = np.zeros(C, dtype=np.int64)
    device = bool(on_device)
    while True:
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        if device:
            try:
                r = handle.profile_fit_sets(Xs, Y, owner[live], state[live], seg)
            except api.CcgpError as e:
                if e.code != -4:   # CCGP_EUNSUPPORTED: this shape has no device fit; the twin carries it
                    raise
                device = False
                continue
            state[live] = r["state"]
            evals[live] += r["evals"]
            calls[np.unique(owner[live])] += 1
        else:
            sub = state[live]
            took = _twin_fit_segment(handle, Xs, Y, owner[live], sub, seg)
            state[live] = sub
            evals[live] += took
            for c in np.unique(owner[live]):   # every step carried every running start: a set's calls are its longest start's
                calls[c] += int(took[owner[live] == c].max())
    f_all, x_all = state[:, api.FIT_F].copy(), api.fit_x(state)
    code = state[:, api.FIT_CODE].astype(np.int64)
    best = []
    for c in range(C):
        f = f_all[c * S:(c + 1) * S]
        if not np.isfinite(f).any():
            raise RuntimeError("ordinary_kriging_fit_device_sets: the likelihood failed at every start of set %d" % c)
        best.append(c * S + int(np.argmin(np.where(np.isfinite(f), f, np.inf))))
    fb, _, thetas, s2, beta, _ = handle.profile_fit_eval_sets(Xs, Y, x_all[best], np.arange(C), grad=False)
    out = []
    for c in range(C):
        sl = slice(c * S, (c + 1) * S)
        out.append(dict(sigma2=float(s2[c]), theta=np.array(thetas[c]), beta=float(beta[c]), loglik=float(-fb[c]), f=f_all[sl],
                        x=x_all[sl], converged=(code[sl] == api.FIT_CONV_REDUCTION) | (code[sl] == api.FIT_CONV_PROJ_GRAD),
                        calls=int(calls[c]) + 1, evaluations=int(evals[sl].sum()) + 1))
    return out


def ordinary_kriging_fit_device(handle, D_train, y_train, starts=8, rng=0, extra_starts=None, on_device=True, seg=512):
    """ordinary_kriging_fit_device_sets for one training set: its C = 1 case, field for field."""
    return ordinary_kriging_fit_device_sets(handle, [D_train], [y_train], starts, rng, extra_starts, on_device, seg)[0]


def matern_profile(handle, D, y, nu, thetas, fused_grad=False):
    """log.likeli of the 1-D scripts (D1:424-444) for an array of scale parameters in ONE value-only device call under the
    Matern(nu) family: log det R(theta) + n log sigma2.MLE(theta), with beta.MLE and sigma2.MLE (D1:411-415) at each theta.
    fused_grad=True: the call runs with OPT_FAMILY_FUSED_GRAD on (n <= 32: the register-resident evaluator in place of the
    blocked sweep, equal to rounding).  Returns dict(loglikeli, beta, sigma2, status), NaN where the factorisation failed."""
    from .rsurface import _FamilyHandle

    D = np.asarray(D, dtype=np.float64).reshape(-1, 1)
    y = np.asarray(y, dtype=np.float64).ravel()
    n = D.shape[0]
    thetas = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
    h = _FamilyHandle(handle, api.KERNEL_MATERN, float(nu), fused_grad=fused_grad)
    ll, s2, beta, _, st = h.profile_batch(D, y, 1, np.stack([np.ones_like(thetas), thetas], axis=1), grad=False)
    return dict(loglikeli=-2.0 * ll - n * math.log(2.0 * math.pi) - n, beta=beta, sigma2=s2, status=st)


def Combined_GP_fit(gp, D_train, y_train, D_new, start, N_max, samp_size, alpha_geweke, batch_size,
                    alpha=0.05, net_samp_size=None, y_new=None, sigma2=None, theta1_pars=None,
                    theta2_pars=None, rng=None, speculate=0):
    """ISO:736-783 / ANI:730-777 / D1:989-1016 minus the plots: sigma2 (ordinary kriging) ->
    posterior draws (laplace + Metro) -> predictions with intervals at D.new."""
    rng = np.random.default_rng(rng)
    if sigma2 is None:
        if getattr(gp, "script", "") in ("D1", "D1F") or hasattr(gp, "nu"):
            # the 1-D scripts take sigma2 from their own Matern MLEs() (D1:455-471, D1:994-995)
            base = getattr(gp.h, "_handle", gp.h)
            sigma2 = matern_MLEs(base, D_train, y_train, gp.nu)["sigma2"]
        else:
            sigma2, _, _ = ordinary_kriging_sigma2(gp.h, D_train, y_train)
    net = net_samp_size or samp_size
    ff = factors_frame(gp, start, N_max, samp_size, batch_size, alpha_geweke, D_train, sigma2, y_train, net,
                       theta1_pars, theta2_pars, rng, speculate=speculate)
    y_new = np.full(np.asarray(D_new).shape[0], np.nan) if y_new is None else y_new
    table = compare_GP(gp, D_new, alpha, y_new, ff["draws"], D_train, sigma2, y_train, rng)
    table.update(sigma2=sigma2, draws=ff["draws"], beta=ff["beta"], chain=ff["chain"])
    return table


def write_results_table(path, table, D_test, input_names, comparators=("single", "CGP")):
    """The file compare.GP's result is written to (`write.table(as.matrix(Comp.obj), file = fname)`,
    GV:759-761): the test inputs, y.hat / Quant / LL / UL of the Combined GP, the comparator models'
    columns and y.true -- same columns, order and number format as `Results/Size 50 Results 1.txt`, so the two files can be
    diffed.  A comparator c whose y_hat_c / LL_c / UL_c the table holds (compare_GP(..., cgp=True) adds CGP's) is written;
    (compare_GP(..., single=True) adds the single GP's: mlegp's variance form is ccgp_krige_predict_batch's VAR_PLUGIN);
    one it does not hold is NA."""
    from .tables import write_table
    D_test = np.asarray(D_test, dtype=np.float64)
    m = D_test.shape[0]
    cols = [D_test, table["y_hat"][:, None], table["quant"][:, None], table["LL"][:, None], table["UL"][:, None]]
    names = list(input_names) + ["y.hat.Combined", "Quant.Combined", "LL.Combined", "UL.Combined"]
    for c in comparators:
        keys = ["y_hat_%s" % c, "LL_%s" % c, "UL_%s" % c]
        if all(k in table for k in keys):
            cols.append(np.stack([np.asarray(table[k], dtype=np.float64) for k in keys], axis=1))
        else:
            cols.append(np.full((m, 3), np.nan))
        names += ["y.hat.%s" % c, "LL.%s" % c, "UL.%s" % c]
    cols.append(np.asarray(table["y_true"], dtype=np.float64)[:, None])
    names.append("y.true")
    write_table(path, np.hstack(cols), names)
    return names


def comparison_summary(table):
    """Comparison.Summary (ANI:703-721, D1:886-899): RMSPE and interval coverage of the Combined GP, and of every comparator
    whose columns the table holds (rmspe_single / coverage_single, rmspe_CGP / coverage_CGP)."""
    y = np.asarray(table["y_true"], dtype=np.float64)
    e = y - table["y_hat"]
    cover = np.mean((y >= table["LL"]) & (y <= table["UL"]))
    out = dict(rmspe=float(np.sqrt(np.mean(e ** 2))), coverage=float(cover),
               mean_quantile=float(np.mean(table["quant"])))
    for c in ("single", "CGP"):
        keys = ["y_hat_%s" % c, "LL_%s" % c, "UL_%s" % c]
        if all(k in table for k in keys):
            yh, lo, hi = (np.asarray(table[k], dtype=np.float64) for k in keys)
            out["rmspe_%s" % c] = float(np.sqrt(np.mean((y - yh) ** 2)))
            out["coverage_%s" % c] = float(np.mean((y >= lo) & (y <= hi)))
    return out


# ----------------------------------------------------------------------------- the simulation study (GV:689-762)
def group_sets(sets):
    """The indices of `sets` (tuples whose first entry is the training design) grouped by the design's shape (n, d), in
    order of first appearance: the sets of a group can be fitted in lockstep."""
    groups = {}
    for i, s in enumerate(sets):
        D = np.asarray(s[0])
        if D.ndim != 2:
            raise ValueError("set %d: the training design must be n x d" % i)
        groups.setdefault(D.shape, []).append(i)
    return groups


def stack_tables(tables):
    """The rows of several compare_GP tables under one another: every per-test-point column they all hold."""
    first = tables[0]
    cols = [k for k in first if isinstance(first[k], np.ndarray) and first[k].ndim == 1 and first[k].size == first["y_true"].size]
    cols = [k for k in cols if all(k in t for t in tables)]
    return {k: np.concatenate([np.asarray(t[k], dtype=np.float64) for t in tables]) for k in cols}


def study(gp, sets, alpha, N, samp_size, batch_size, alpha_geweke, net_samp_size=None, start=None, sigma2s=None,
          theta1_pars=None, theta2_pars=None, rngs=None, max_proposals=None, speculate=0, laplace=None, cgp=False,
          single=False, out_dir=None, input_names=None, logpost_sets_fn=None, compare_fn=None, lockstep_fits=True,
          device_chains=False, device_fits=False, device_laplace=False, device_cgp=False, lockstep_predict=False):
    """The reference's simulation study (GV:689-762 declares nine training sets and fits one): every set of `sets` -- a list
    of (D_train, y_train, D_test, y_test) -- fitted and compared, the sets of one shape (n, d) in lockstep.  Per group:
    sigma2 per set from ordinary_kriging_fit (or sigma2s[i] as given), then laplace_sets and Metro_sets with one generator
    per set (rngs[i]; one device call per step for all the group's chains).  Per set: the retained draws (the last
    net_samp_size of the chain, factors_frame's), compare_GP(..., exact=True, cgp=cgp, single=single) and
    comparison_summary.  laplace: ready estimates per set.  start: one transformed start for all sets ((1, 1, 0) as GV:692
    by default, a zero appended where the script has a fourth parameter), or one per set.  out_dir: one results table per
    set through write_results_table (`results_<i>.txt`, i from 1; input_names default x1 ..).  logpost_sets_fn(group
    indices) -> evaluator and compare_fn replace the device (tests).
    lockstep_fits (default on): the comparator fits run in lockstep across the sets of a group as well -- sigma2 from
    ordinary_kriging_fit_sets for the sets whose sigma2 was not given; with single=True that same fitted model goes to
    compare_GP instead of being fitted a second time (a dict of fit keywords in `single` asks for a fit of its own, also in
    lockstep); with cgp the models come from cgp.CGP_sets (a cgp dict's keywords passed on; a seed in `rng` is every set's
    seed, as it is cgp.CGP's per call; a Generator in `rng` is one stream advancing from set to set, so those CGP fits stay
    in compare_GP, set after set) -- and compare_GP only predicts.  Tables, summaries, sigma2, draws and chains have the
    same bits either way.  The per-set loop stays for a 1-D (Matern) gp, whose comparator is matern_MLEs, where compare_fn
    or logpost_sets_fn replaces the device, and with lockstep_fits=False.
    device_chains (default off): the Metro part of each group goes through Metro_device_sets -- chains resident on the
    device, many proposals per launch, with that function's own stream contract (so other chains than Metro_sets', same
    law); the Laplace stage then runs on its twin evaluator, and speculate is not used.
    device_fits (default off): the sigma2 / single-GP fits of each group go through ordinary_kriging_fit_device_sets -- the
    quasi-Newton iteration resident on the device, every start of every set in one launch -- with that function's own
    contract (the same method and optimum as ordinary_kriging_fit_sets, not its bits).
    device_laplace (default off): the Laplace stage of each group goes through laplace_device_sets -- the Nelder-Mead search
    resident on the device, every set's search in one launch, over the twin evaluator.  Its estimates are laplace_sets' over
    that evaluator bit for bit, so with device_chains=True the tables are those of device_chains=True alone.
    device_cgp (default off): the CGP fits' refinement runs on the device (cgp.CGP_sets / cgp.CGP with on_device=True): the
    same models bit for bit, so the tables are those of device_cgp=False.
    lockstep_predict (default off): the prediction stage runs in lockstep as well -- without compare_fn and for a gp that is
    not 1-D, the tables come from compare_GP_sets: per group of sets of one shape (n, d, m) one device call for the Combined
    GP, one for the single GP and one for the CGP, a comparator going that way only when its model is already fitted (in
    lockstep, or given); any other set falls back to compare_GP.  calls["predict"] counts the prediction calls on the device
    in either mode: per set one per model of its table, per group one per model with lockstep_predict.  (This changes what the
    default reports: it used to count one per set whatever the comparators; with a compare_fn it still does.)  Tables,
    summaries and result files are those of lockstep_predict=False bit for bit.
    Returns dict(tables, summaries, pooled: comparison_summary of the stacked tables, sigma2, draws, beta, chains,
    groups: {(n, d): indices}, calls and seconds: device calls and wall time of the sigma2, single, cgp, laplace, metro and
    predict parts; per set the single and cgp fits happen inside compare_GP, so their seconds are part of predict's and
    their calls are read from the fitted models)."""
    import time

    sets = list(sets)
    if not sets:
        raise ValueError("study: no sets")
    cgp = _cgp_on_device(cgp, device_cgp)
    C = len(sets)
    groups = group_sets(sets)
    net = net_samp_size or samp_size
    rngs = list(rngs) if rngs is not None else [None] * C
    if len(rngs) != C or (sigma2s is not None and len(sigma2s) != C) or (laplace is not None and len(laplace) != C):
        raise ValueError("study: rngs, sigma2s and laplace hold one entry per set")
    npar = gp.cfg["npar"] if hasattr(gp, "cfg") else 3
    if start is None:
        start = np.concatenate([[1.0, 1.0, 0.0], np.zeros(npar - 3)])
    starts = np.broadcast_to(np.asarray(start, dtype=np.float64), (C, np.shape(start)[-1]))
    lockstep = bool(lockstep_fits) and compare_fn is None and logpost_sets_fn is None and not hasattr(gp, "nu")
    predict_sets = bool(lockstep_predict) and compare_fn is None and not hasattr(gp, "nu")
    own_compare = compare_fn is None   # compare_GP itself: one device call per model of the table
    compare_fn = compare_fn or compare_GP
    fit_sets = ordinary_kriging_fit_device_sets if device_fits else ordinary_kriging_fit_sets
    fit_one = ordinary_kriging_fit_device if device_fits else ordinary_kriging_fit
    calls = dict(sigma2=0, single=0, cgp=0, laplace=0, metro=0, predict=0)
    secs = dict(sigma2=0.0, single=0.0, cgp=0.0, laplace=0.0, metro=0.0, predict=0.0)
    s2 = [None] * C if sigma2s is None else [float(v) for v in sigma2s]
    chains, tables, summaries = [None] * C, [None] * C, [None] * C
    single_of, cgp_of = [single] * C, [cgp] * C   # what compare_GP is told per set
    cgp_in_compare = bool(cgp)   # compare_GP fits the CGP itself
    t0 = time.perf_counter()
    if lockstep:
        base = getattr(gp.h, "_handle", gp.h)
        given = dict(single) if isinstance(single, dict) else {}
        has_model = "est" in given or ("theta" in given and "sigma2" in given)
        fit_kw = {k: v for k, v in given.items() if k not in ("theta", "sigma2", "beta", "est")}
        for shape, idx in groups.items():
            # the sigma2 fit IS the single GP's fit when the latter asks for nothing of its own
            share = bool(single) and not has_model and not fit_kw
            todo = [i for i in idx if s2[i] is None or share]
            if not todo:
                continue
            part = "sigma2" if any(s2[i] is None for i in todo) else "single"   # every sigma2 given: the single GP's fit alone
            t0 = time.perf_counter()
            fits = fit_sets(base, [sets[i][0] for i in todo], [sets[i][1] for i in todo])
            calls[part] += max(f["calls"] for f in fits)
            for i, f in zip(todo, fits):
                if s2[i] is None:
                    s2[i] = f["sigma2"]
                if share:
                    single_of[i] = dict(est=f)
            secs[part] += time.perf_counter() - t0   # the time goes where the calls go
        t0 = time.perf_counter()
        if single and not has_model and fit_kw:
            for shape, idx in groups.items():
                fits = fit_sets(base, [sets[i][0] for i in idx], [sets[i][1] for i in idx], **fit_kw)
                calls["single"] += max(f["calls"] for f in fits)
                for i, f in zip(idx, fits):
                    single_of[i] = dict(est=f)
        secs["single"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        cgp_kw = dict(cgp) if isinstance(cgp, dict) else {}
        # a Generator in the dict is ONE stream that cgp.CGP advances from set to set: only the per-set loop (compare_GP, in
        # set order) reproduces it.  A seed is a fresh default_rng(seed) per CGP call, which is CGP_sets' rngs=[seed] * C.
        cgp_lockstep = bool(cgp) and "est" not in cgp_kw and not isinstance(cgp_kw.get("rng"), np.random.Generator)
        if cgp_lockstep:
            from . import cgp as cgp_mod
            seed = cgp_kw.pop("rng", 0)
            for shape, idx in groups.items():
                ests = cgp_mod.CGP_sets(base, [sets[i][0] for i in idx], [sets[i][1] for i in idx],
                                        rngs=[seed] * len(idx), **cgp_kw)
                calls["cgp"] += ests[0]["calls"]
                for i, e in zip(idx, ests):
                    cgp_of[i] = dict(est=e)
        secs["cgp"] = time.perf_counter() - t0
        cgp_in_compare = bool(cgp) and "est" not in cgp_kw and not cgp_lockstep   # the one stream, set after set
    else:
        for i in range(C):
            if s2[i] is None:
                okf = fit_one(getattr(gp.h, "_handle", gp.h), sets[i][0], sets[i][1])
                s2[i] = okf["sigma2"]
                calls["sigma2"] += okf["calls"]
        secs["sigma2"] = time.perf_counter() - t0
    for shape, idx in groups.items():
        D_trains = [np.asarray(sets[i][0], dtype=np.float64) for i in idx]
        ys = [np.asarray(sets[i][1], dtype=np.float64).ravel() for i in idx]
        g_s2 = [s2[i] for i in idx]
        fn = logpost_sets_fn(idx) if logpost_sets_fn is not None else None
        if fn is None:
            make = _twin_sets_evaluator if device_chains else _device_sets_evaluator
            fn = make(gp, D_trains, ys, g_s2, theta1_pars, theta2_pars)
        count = dict(n=0)

        def counted(rows, set_of, fn=fn, count=count):
            count["n"] += 1
            return fn(rows, set_of)

        t0 = time.perf_counter()
        if laplace is not None:
            ests = [laplace[i] for i in idx]
        elif device_laplace:
            ests = laplace_device_sets(gp, D_trains, ys, g_s2, starts[idx], theta1_pars, theta2_pars,
                                       logpost_sets_fn=fn if logpost_sets_fn is not None else None)
            count["n"] = max(e["calls"] for e in ests)
        else:
            ests = laplace_sets(lambda rows, set_of: counted(rows, set_of)[0], starts[idx])
        secs["laplace"] += time.perf_counter() - t0
        calls["laplace"] += count["n"]
        t0 = time.perf_counter()
        if device_chains:
            r = Metro_device_sets(gp, None, N, samp_size, batch_size, alpha_geweke, D_trains, g_s2, ys, theta1_pars, theta2_pars,
                                  [rngs[i] for i in idx], max_proposals, laplace=ests,
                                  logpost_sets_fn=fn if logpost_sets_fn is not None else None)
        else:
            r = Metro_sets(gp, None, N, samp_size, batch_size, alpha_geweke, D_trains, g_s2, ys, theta1_pars, theta2_pars,
                           [rngs[i] for i in idx], max_proposals, speculate, laplace=ests, logpost_sets_fn=fn)
        secs["metro"] += time.perf_counter() - t0
        calls["metro"] += r["device_batches"] + 1   # the chains' starting values are one call
        for j, i in enumerate(idx):
            chains[i] = r["chains"][j]
    keep = slice(samp_size - net, samp_size)
    draws = [transformed_to_draws(ch["sample"][keep]) for ch in chains]
    betas = [ch["beta"][keep] for ch in chains]
    t0 = time.perf_counter()
    if predict_sets:
        made = {}
        tables = compare_GP_sets(gp, [s[2] for s in sets], alpha, [s[3] for s in sets], draws, [s[0] for s in sets], s2,
                                 [s[1] for s in sets], cgp=cgp_of, single=single_of, counts=made)
        calls["predict"] = made["calls"]
    for i, (D_train, y_train, D_test, y_test) in enumerate(sets):
        if not predict_sets:
            tables[i] = compare_fn(gp, D_test, alpha, y_test, draws[i], D_train, s2[i], y_train, exact=True, cgp=cgp_of[i],
                                   single=single_of[i])
            calls["predict"] += 1 + (bool(cgp_of[i]) + bool(single_of[i]) if own_compare else 0)
        summaries[i] = comparison_summary(tables[i])
        # the fits compare_GP made itself
        if not lockstep and single and isinstance(tables[i].get("single"), dict):
            calls["single"] += int(tables[i]["single"].get("calls", 0))
        if cgp_in_compare and isinstance(tables[i].get("CGP"), dict):
            calls["cgp"] += int(tables[i]["CGP"].get("calls", 0))
    secs["predict"] = time.perf_counter() - t0
    if out_dir is not None:
        import os
        os.makedirs(out_dir, exist_ok=True)
        for i, (D_train, _, D_test, _) in enumerate(sets):
            names = input_names or ["x%d" % (k + 1) for k in range(np.asarray(D_test).shape[1])]
            write_results_table(os.path.join(out_dir, "results_%d.txt" % (i + 1)), tables[i], D_test, names)
    return dict(tables=tables, summaries=summaries, pooled=comparison_summary(stack_tables(tables)), sigma2=s2, draws=draws,
                beta=betas, chains=chains, groups={k: list(v) for k, v in groups.items()}, calls=calls, seconds=secs)
