"""The composite GP of Ba & Joseph as every script carries it: CGP (GV:58-236) and predict.CGP (GV:245-317), the third model of
compare.GP's table (GV:654-660), with its objective on the device.

The reference evaluates var.MLE.DK (GV:102-133) -- three correlation matrices, five solve(Q) -- at 505 Latin-hypercube
candidates one after another, refines the num_starts best with optim(method = "L-BFGS-B") on finite differences, one
evaluation per call, and then runs n more five-solve fits for the jackknife.  Here

  * the 505 candidates are ONE call of ccgp_cgp_state_batch;
  * the num_starts refinements run in lockstep through design.minimize_starts under the reference's per-variable bounds.  The
    gradient is by central differences clipped at the bounds, so an evaluator call is one device call that carries, for every
    start still running, its trial point and the 2 (p + 3) points around it;
  * the jackknife is one call of n rows with skip = 0 .. n-1;
  * the final state and every prediction come from ccgp_cgp_predict.

Difference step.  R's optim differences with ndeps = 1e-3.  The objective is smooth in the box (five fixed reweighting
passes, no data-dependent iteration), its values carry a rounding error of about n eps cond(Q) <= 1e-10, and a central
difference with step h has truncation error h^2 f''' / 6 and rounding error 1e-10 / h: h = 1e-5 leaves both near 1e-5 of a
gradient whose entries are of order 1 to 100, where 1e-3 leaves a truncation error of 1e-6 |f'''| that moved the optimum's
predictions by 0.01 rms on the Ground-Vibrations set (0.001 with 1e-5).  `step` is an argument.

CGP_sets fits the models of many training sets of one shape in lockstep (a simulation study's comparator): the same three
steps with the rows of every set in each device call (ccgp_cgp_state_batch_sets).

on_device=True (CGP and CGP_sets, default off) keeps the refinement on the device (refine_starts_device over
ccgp_cgp_fit_sets): rounds of two launches, the gated evaluation of every running start's 1 + 2 (p + 3) rows and one wave per
start that differences them, steps the start (csrc/fit_logic.h) and writes its next rows, `look` rounds between the host's
looks.  Every operation between stepper and evaluator is exactly rounded on both sides (csrc/cgp_fit_logic.h), so the fit is
the default's bit for bit.

The final optim run from `beststart` (GV:155-157) is not repeated: it starts where that start's refinement started, every
evaluation depends on its own row only (not on the batch it travels in), so the lockstep run of that start IS that run.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .design import _FIT_MESSAGES, minimize_starts

N_CANDIDATE_BASE = 500      # n_candidate = 500 + num_starts (GV:136)
NONFINITE = 1e6             # GV:130-131


def _plain(handle):
    return getattr(handle, "_handle", handle)


def standardise(X):
    """(Stand_DD, scales) of GV:68-70."""
    X = np.asarray(X, dtype=np.float64)
    lo = X.min(axis=0)
    scales = X.max(axis=0) - lo
    return (X - lo) / scales, scales


def bounds(Xs, nugget_l=0.001, theta_l=None, alpha_l=None, kappa_u=None):
    """(lower, upper) of (lambda, Stand_theta[p], kappa, bw), GV:77-89."""
    n, p = Xs.shape
    iu = np.triu_indices(n, 1)
    d2 = ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(-1)[iu]
    inv = float(np.mean(1.0 / d2))
    theta_l = 1e-4 if theta_l is None else float(theta_l)
    alpha_l = math.log(10.0 ** 2) * inv if alpha_l is None else float(alpha_l)
    kappa_u = math.log(10.0 ** 6) * inv if kappa_u is None else float(kappa_u)
    if theta_l > alpha_l:
        raise ValueError("CGP: the lower bound of theta exceeds its upper bound alpha_l")
    lower = np.concatenate([[nugget_l], np.full(p, theta_l), [alpha_l], [0.0]])
    upper = np.concatenate([[1.0], np.full(p, alpha_l), [kappa_u], [1.0]])
    return lower, upper


def rows_from_ww(ww):
    """(lambda, Stand_theta, kappa, bw) -> the device's (lambda, theta, alpha = kappa + theta, bw), GV:103-107."""
    ww = np.atleast_2d(np.asarray(ww, dtype=np.float64))
    p = ww.shape[1] - 3
    return np.concatenate([ww[:, :1 + p], ww[:, 1:1 + p] + ww[:, 1 + p:2 + p], ww[:, 2 + p:]], axis=1)


def lhd(N, k, rng):
    """LHD of GV:137-142 from a seeded numpy generator: a random permutation of the N cell midpoints per column."""
    return (np.stack([rng.permutation(N) for _ in range(k)], axis=1) + 0.5) / N


def CGP(handle, X, y, nugget_l=0.001, num_starts=5, theta_l=None, alpha_l=None, kappa_u=None, rng=0, step=1e-5,
        on_device=False, look=16):
    """CGP(X, yobs, ...) of GV:58-236 -> dict with the reference's fields (lambda, theta, alpha, bandwidth, Sig_matrix: its
    diagonal, sf, res2, temp_matrix, mu, tau2, beststart, objval, rmscv, Yp_jackknife, X, yobs), the fit's bounds, and
    calls / evaluations: device calls and the parameter rows they carried (seconds: host clock around the three steps).  invQ
    is not returned: predict_CGP solves with the factor the device keeps.  It is _fit_sets' C = 1 case over
    ccgp_cgp_state_batch.  on_device: the refinement through refine_starts_device (`look` rounds between the host's looks):
    every field the same bits except calls, refinement_calls and seconds."""
    h = _plain(handle)

    def state(designs, Y, rows, set_of, skip):
        return h.cgp_state_batch(designs[0], Y[0], rows, skip=skip)

    return _fit_sets("CGP", "", h, state, [X], [y], [rng], nugget_l, num_starts, theta_l, alpha_l, kappa_u, step, on_device,
                     look)[0]


def CGP_sets(handle, Xs, ys, nugget_l=0.001, num_starts=5, theta_l=None, alpha_l=None, kappa_u=None, rngs=None, step=1e-5,
             on_device=False, look=16):
    """CGP for C training sets of one shape in lockstep -> a list with, per set, the dict CGP(handle, Xs[c], ys[c], ...,
    rng=rngs[c]) returns: every field bit for bit except calls, evaluations, refinement_calls and seconds.

      * the candidates of all sets are ONE call of ccgp_cgp_state_batch_sets, each set's LHD from its own generator (rngs[c],
        default seed 0 each, as CGP's);
      * the num_starts refinements of all sets run through ONE design.minimize_starts with per-start bounds (a set's box is
        its own: cgp.bounds), so an evaluator call is one device call for every start of every set still running;
      * the jackknife of all sets is one call of C n rows with skip;
      * the final state per set is ccgp_cgp_predict, unchanged.
    A start's trajectory depends on its own evaluations only and a row's bits on its own set only, so each set's fit is the
    fit it has alone.  calls and refinement_calls are the group's device calls (the same in every dict), evaluations the
    rows of the set itself, seconds the group's.  on_device: the refinement of all sets through refine_starts_device, as CGP's."""
    h = _plain(handle)
    rngs = [0] * len(Xs) if rngs is None else list(rngs)

    def state(designs, Y, rows, set_of, skip):
        return h.cgp_state_batch_sets(designs, Y, rows, set_of, skip=skip)

    return _fit_sets("CGP_sets", " of set %d", h, state, Xs, ys, rngs, nugget_l, num_starts, theta_l, alpha_l, kappa_u, step,
                     on_device, look)


def refine_starts_device(handle, Xs, ys, starts, lowers, uppers, set_of, step, look=16, maxit=100, factr=1e7, pgtol=0.0,
                         max_backtracks=30, on_device=True, seg=512, evaluate=None):
    """minimize_starts for the CGP objective with the iteration itself on the device: start s = (lambda, theta, kappa, bw)
    [S, p + 3] runs on the standardised training set set_of[s] of Xs [C, n, p], ys [C, n] under its own box lowers[s],
    uppers[s], and one call of ccgp_cgp_fit_sets carries every running start through up to `seg` evaluations -- two launches
    per evaluation, `look` evaluations between the host's looks -- until none is running.

    x, f, converged, iterations, message and calls_per_start are, bit for bit, what minimize_starts returns over the
    lockstep evaluator (central differences of `step` clipped at the box over ccgp_cgp_state_batch_sets).  `calls` counts
    device calls: calls of ccgp_cgp_fit_sets, or on the twin the evaluator calls.

    on_device=False drives the same states through the host twin -- every evaluation through ccgp_cgp_fit_eval_sets, every
    step through ccgp_fit_feed -- and leaves the same states; the driver falls back to it by itself where the device call
    says CCGP_EUNSUPPORTED (too many rows for one launch, a workspace limit the rows do not fit under).  Beyond 64 variables
    no such state exists: minimize_starts runs over `evaluate` (minimize_starts' evaluator with pass_live), which the caller
    then has to give."""
    from . import api

    starts = np.asarray(starts, dtype=np.float64)
    S, nv = starts.shape
    set_of = np.asarray(set_of, dtype=np.int64).reshape(S)
    lowers = np.broadcast_to(np.asarray(lowers, dtype=np.float64), (S, nv))
    uppers = np.broadcast_to(np.asarray(uppers, dtype=np.float64), (S, nv))
    seg, look = int(seg), int(look)
    if seg < 1 or seg > api.FIT_MAX_EVALS:
        raise ValueError("refine_starts_device: seg must lie in 1 .. %d" % api.FIT_MAX_EVALS)
    if look < 1 or look > 64:
        raise ValueError("refine_starts_device: look must lie in 1 .. 64")
    if nv > 64:   # the stepper's state ends at 64 variables (csrc/fit_logic.h): minimize_starts itself over the lockstep evaluator
        if evaluate is None:
            raise ValueError("refine_starts_device: more than 64 variables need minimize_starts' evaluator")
        return minimize_starts(evaluate, starts, m=5, maxit=maxit, factr=factr, pgtol=pgtol, max_backtracks=max_backtracks,
                               lowers=lowers, uppers=uppers, pass_live=True)
    state = np.stack([api.fit_begin(starts[s], lowers[s], uppers[s], maxit, factr, pgtol, max_backtracks)
                      for s in range(S)]) if S else np.zeros((0, api.FIT_HEADER + 16 * nv))
    device = bool(on_device)
    calls = 0
    while True:
        live = np.flatnonzero(state[:, api.FIT_CODE] == api.FIT_RUNNING)
        if live.size == 0:
            break
        if device:
            try:
                r = handle.cgp_fit_sets(Xs, ys, set_of[live], state[live], step, seg, look)
            except api.CcgpError as e:
                if e.code != -4:   # CCGP_EUNSUPPORTED: these starts have no device refinement; the twin carries them
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
                f, g, st = handle.cgp_fit_eval_sets(Xs, ys, api.fit_trial(state[run]), lowers[run], uppers[run], step, set_of[run])
                calls += 1
                for k, a in enumerate(run):
                    api.fit_feed(state[a], f[k], np.asarray(g[k]).ravel(), st[k] == 0)
    code = state[:, api.FIT_CODE].astype(np.int64)
    return dict(x=api.fit_x(state), f=state[:, api.FIT_F].copy(),
                converged=(code == api.FIT_CONV_REDUCTION) | (code == api.FIT_CONV_PROJ_GRAD),
                iterations=state[:, api.FIT_ITERATIONS].astype(np.int64), message=[_FIT_MESSAGES[c] for c in code],
                calls=calls, calls_per_start=state[:, api.FIT_EVALS].astype(np.int64))


def _fit_sets(who, of_set, h, state, Xs, ys, rngs, nugget_l, num_starts, theta_l, alpha_l, kappa_u, step, on_device=False,
              look=16):
    """The fit of C sets of one shape in lockstep: candidates, refinement, jackknife, final state.  state(designs[C, n, p],
    Y[C, n], rows, set_of, skip) -> (val, ..., loo, status) evaluates row b on set set_of[b]; skip is None except in the
    jackknife.  who and of_set (a format of the set's index, or empty) word the errors, those about the arguments' shapes
    included.  on_device: the refinement runs through refine_starts_device on h instead of minimize_starts over `state`; the
    rows it evaluates are counted from the starts' evaluation counts.  Returns one dict per set."""
    DDs = [np.asarray(X, dtype=np.float64) for X in Xs]
    yobs = [np.asarray(y, dtype=np.float64).ravel() for y in ys]
    C = len(DDs)
    if C < 1 or len(yobs) != C:
        raise ValueError("%s: one response per design, at least one set" % who)
    if any(D.ndim != 2 or D.shape != DDs[0].shape for D in DDs) or any(y.shape[0] != DDs[0].shape[0] for y in yobs):
        raise ValueError("%s: the sets of one call have one shape (n, p)" % who)
    if len(rngs) != C:
        raise ValueError("%s takes one generator per set" % who)
    gens = [r if isinstance(r, np.random.Generator) else np.random.default_rng(r) for r in rngs]
    n, p = DDs[0].shape
    n_par = p + 3
    std = [standardise(D) for D in DDs]
    box = [bounds(std[c][0], nugget_l, theta_l, alpha_l, kappa_u) for c in range(C)]
    XS, XD, Y = np.stack([s[0] for s in std]), np.stack(DDs), np.stack(yobs)
    count = dict(calls=0, rows=np.zeros(C, dtype=np.int64))

    def objective(ww, set_of):
        """var.MLE.DK at the rows of ww, row b on set set_of[b], in one device call -> (val with GV:130-131 applied, status)."""
        val, _, _, _, st = state(XS, Y, rows_from_ww(ww), set_of, None)
        count["calls"] += 1
        np.add.at(count["rows"], set_of, 1)
        return np.where(np.isfinite(val), val, NONFINITE), st

    n_cand = N_CANDIDATE_BASE + num_starts
    cand_pts = [box[c][0] + lhd(n_cand, n_par, gens[c]) * (box[c][1] - box[c][0]) for c in range(C)]     # GV:144-148
    clock = [time.perf_counter()]
    cand, _ = objective(np.concatenate(cand_pts), np.repeat(np.arange(C), n_cand))
    clock.append(time.perf_counter())
    Starts = []
    for c in range(C):
        order = np.argsort(cand[c * n_cand:(c + 1) * n_cand], kind="stable")[:num_starts]              # GV:150-151
        Starts.append(cand_pts[c][np.sort(order)])
    S = Starts[0].shape[0]
    owner = np.repeat(np.arange(C), S)
    lowers, uppers = np.stack([box[c][0] for c in owner]), np.stack([box[c][1] for c in owner])

    def evaluate(W, live):
        k = W.shape[0]
        hi = np.minimum(W + step, uppers[live])
        lo = np.maximum(W - step, lowers[live])
        pts = np.repeat(W[:, None, :], 1 + 2 * n_par, axis=1)
        for j in range(n_par):
            pts[:, 1 + 2 * j, j] = hi[:, j]
            pts[:, 2 + 2 * j, j] = lo[:, j]
        f, st = objective(pts.reshape(-1, n_par), np.repeat(owner[live], 1 + 2 * n_par))
        f = f.reshape(k, 1 + 2 * n_par)
        g = (f[:, 1::2] - f[:, 2::2]) / (hi - lo)
        return f[:, 0], g, st.reshape(k, -1)[:, 0]

    if on_device:
        res = refine_starts_device(h, XS, Y, np.concatenate(Starts), lowers, uppers, owner, step, look, evaluate=evaluate)
        if n_par <= 64:   # (beyond it `evaluate` ran and counted for itself)
            count["calls"] += res["calls"]
            np.add.at(count["rows"], owner, res["calls_per_start"] * (1 + 2 * n_par))
    else:
        res = minimize_starts(evaluate, np.concatenate(Starts), lowers=lowers, uppers=uppers, pass_live=True)   # GV:152-154
    clock.append(time.perf_counter())
    fitted = []
    for c in range(C):
        sl = slice(c * S, (c + 1) * S)
        f, x = res["f"][sl], res["x"][sl]
        if not np.isfinite(f).any():
            raise RuntimeError("%s: the objective failed at every start%s" % (who, of_set and of_set % c))
        best = int(np.argmin(np.where(np.isfinite(f), f, np.inf)))                                     # GV:155-157
        par = x[best]
        lam, st_theta, kappa, bw = float(par[0]), par[1:1 + p], float(par[1 + p]), float(par[2 + p])
        scales = std[c][1]
        theta = st_theta / scales ** 2                                                                 # GV:164-165
        alpha = (kappa + st_theta) / scales ** 2
        fitted.append(dict(best=best, par=par, lam=lam, theta=theta, alpha=alpha, bw=bw,
                           row=np.concatenate([[lam], theta, alpha, [bw]])))

    clock.append(time.perf_counter())
    rows = np.concatenate([np.repeat(ft["row"][None], n, axis=0) for ft in fitted])
    _, _, _, loo, jst = state(XD, Y, rows, np.repeat(np.arange(C), n), np.tile(np.arange(n), C))        # GV:166-198
    clock.append(time.perf_counter())
    count["calls"] += 1
    count["rows"] += n
    keeps = []
    for c in range(C):
        _, keep, status = h.cgp_predict(DDs[c], yobs[c], fitted[c]["row"], np.empty((0, p)))            # GV:200-221
        count["calls"] += 1
        count["rows"][c] += 1
        if status:
            raise RuntimeError("%s: the final state%s cannot be factorised (pivot %d)" % (who, of_set and of_set % c, status))
        keeps.append(keep)
    seconds = dict(candidates=clock[1] - clock[0], refinement=clock[2] - clock[1], jackknife=clock[4] - clock[3])
    out = []
    for c in range(C):
        sl = slice(c * S, (c + 1) * S)
        ft, keep, lo_c = fitted[c], keeps[c], loo[c * n:(c + 1) * n]
        rmscv = float(np.sqrt(np.sum((yobs[c] - lo_c) ** 2) / n))
        out.append(dict(X=DDs[c], yobs=yobs[c], **{"lambda": ft["lam"]}, theta=ft["theta"][None], alpha=ft["alpha"][None],
                        bandwidth=ft["bw"], Sig_matrix=keep["s"], sf=keep["sf"], res2=keep["res2"], temp_matrix=keep["temp"],
                        mu=keep["beta"], tau2=keep["tau2"], beststart=Starts[c][ft["best"]],
                        objval=float(res["f"][sl][ft["best"]]), rmscv=rmscv, Yp_jackknife=lo_c, lower=box[c][0],
                        upper=box[c][1], par=ft["par"], scales=std[c][1], starts=Starts[c], f_starts=res["f"][sl],
                        x_starts=res["x"][sl], converged=res["converged"][sl], jackknife_status=jst[c * n:(c + 1) * n],
                        calls=count["calls"], evaluations=int(count["rows"][c]), refinement_calls=res["calls"],
                        seconds=seconds))
    return out


def param_row(est):
    """The device's parameter row of a fitted model."""
    return np.concatenate([[est["lambda"]], np.ravel(est["theta"]), np.ravel(est["alpha"]), [est["bandwidth"]]])


def predict_CGP(handle, est, newdata, PI=False):
    """predict.CGP(object, newdata, PI) of GV:245-317 -> dict(Yp, gp, lp, v, Y_low, Y_up) as GV:314 returns it: without PI, lp
    stays 0 and the interval is None.  The state is rebuilt on the device from the model's parameters (five factorisations)
    rather than carried through the host."""
    U = np.asarray(newdata, dtype=np.float64)
    U = U.reshape(-1, est["X"].shape[1])
    out, _, status = _plain(handle).cgp_predict(est["X"], est["yobs"], param_row(est), U)
    if status:
        raise RuntimeError("predict_CGP: the state cannot be factorised (pivot %d)" % status)
    if not PI:
        return dict(Yp=out[:, 0], gp=out[:, 1], lp=np.zeros(U.shape[0]), v=out[:, 3], Y_low=None, Y_up=None)
    return dict(Yp=out[:, 0], gp=out[:, 1], lp=out[:, 2], v=out[:, 3], Y_low=out[:, 4], Y_up=out[:, 5])


def predict_CGP_sets(handle, ests, newdatas, PI=False):
    """predict_CGP for many fitted models at once: model i (a dict of CGP or CGP_sets) predicted at newdatas[i].  The models
    whose design has one shape (n, d) and whose test sets have one size m go to the device in ONE call
    (Handle.cgp_predict_sets), so ragged test sets make one call per m.  Returns the list of predict_CGP's dicts, in the
    models' order, each equal to predict_CGP(handle, ests[i], newdatas[i], PI) bit for bit."""
    ests = list(ests)
    if len(ests) != len(newdatas):
        raise ValueError("predict_CGP_sets: one newdata per model")
    Us = [np.asarray(u, dtype=np.float64).reshape(-1, e["X"].shape[1]) for e, u in zip(ests, newdatas)]
    groups = {}
    for i, (e, U) in enumerate(zip(ests, Us)):
        groups.setdefault(e["X"].shape + (U.shape[0],), []).append(i)
    res = [None] * len(ests)
    for (n, d, m), idx in groups.items():
        out, _, status = _plain(handle).cgp_predict_sets(np.stack([ests[i]["X"] for i in idx]),
                                                         np.stack([np.ravel(ests[i]["yobs"]) for i in idx]),
                                                         np.stack([param_row(ests[i]) for i in idx]), np.arange(len(idx)),
                                                         np.stack([Us[i] for i in idx]))
        if status.any():
            j = int(np.flatnonzero(status)[0])
            raise RuntimeError("predict_CGP_sets: the state of model %d cannot be factorised (pivot %d)" % (idx[j], status[j]))
        for j, i in enumerate(idx):
            o = out[j]
            if not PI:
                res[i] = dict(Yp=o[:, 0], gp=o[:, 1], lp=np.zeros(m), v=o[:, 3], Y_low=None, Y_up=None)
            else:
                res[i] = dict(Yp=o[:, 0], gp=o[:, 1], lp=o[:, 2], v=o[:, 3], Y_low=o[:, 4], Y_up=o[:, 5])
    return res
