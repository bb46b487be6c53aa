"""The multi-start max-entropy design search (ccgp_amd.design, Entropy.optim / Batch.Entropy.optim of Batch Sequential
ME Design.R:886-948) on a numpy fp64 evaluator: no device needed.  The pin is a recorded output of the reference:
`Initial ME Design.txt` (BSQ:988) is what Entropy.optim(14, 2, 0.5, 1, 4, 20) (the commented-out BSQ:986) computed,
and it is a Kuhn-Tucker point of log det R_mixed at the prior medians (BSQ:981-983)."""
import numpy as np
import pytest

from ccgp_amd import design
from design_ref import (BSQ_PRIOR, design_distance, initial_me_design, logdet_grad_general, mixed_R_general,
                        numpy_evaluator, params_row, projected_gradient)


def _scipy_best(starts, p, theta1, theta2, D_old=None):
    """scipy's L-BFGS-B (analytic gradient, numpy) from every start; the best -log det.  scipy's line search cannot
    step back from an infinite value, so a point whose R has no Cholesky factor reads as 1e10."""
    from scipy.optimize import minimize
    n_new, d = starts.shape[1:]
    old = np.zeros((0, d)) if D_old is None else np.asarray(D_old, dtype=np.float64)
    row = params_row(p, theta1, theta2, d)
    ld_old = np.linalg.slogdet(mixed_R_general(old, 2, row)[0])[1] if len(old) else 0.0

    def fg(x):
        D = np.vstack([old, x.reshape(n_new, d)])
        try:
            np.linalg.cholesky(mixed_R_general(D, 2, row)[0])
            ld, g = logdet_grad_general(D, 2, row, len(old))
        except np.linalg.LinAlgError:
            return 1e10, np.zeros(x.size)
        return -(ld - ld_old), -g.ravel()

    vals = [minimize(fg, s.ravel(), jac=True, method="L-BFGS-B", bounds=[(-1.0, 1.0)] * s.size).fun for s in starts]
    return min(vals)


def test_first_batch_finds_the_stored_initial_me_design():
    D0 = initial_me_design()
    p, t1, t2 = BSQ_PRIOR
    ev = numpy_evaluator(p, t1, t2)
    ld0 = -ev(D0[None])[0][0]
    res = design.minimize_starts(ev, design.make_starts(20, 14, 2, 0))
    best = int(np.argmin(res["f"]))
    assert -res["f"][best] >= ld0 - 1e-7, (-res["f"][best], ld0)
    assert design_distance(res["x"][best], D0) <= 1e-3
    # lockstep: far fewer calls than the 20 starts' evaluations one after another
    assert res["calls"] < int(res["iterations"].sum())


def test_stored_design_is_a_kuhn_tucker_point():
    D0 = initial_me_design()
    _, g, st = numpy_evaluator(*BSQ_PRIOR)(D0[None])
    assert st[0] == 0 and projected_gradient(D0, g[0]) <= 1e-4


def test_converged_starts_are_kuhn_tucker_points_and_iterates_stay_in_the_box():
    """factr = 1e4 here: at R's default 1e7 the relative-reduction rule stops some starts with projected gradients up to
    1e-3 -- L-BFGS-B itself does so with memory 5 (scipy, maxcor = 5: up to 1.2e-4 on these starts)."""
    calls = []
    ev = numpy_evaluator(*BSQ_PRIOR, calls=calls)
    res = design.minimize_starts(ev, design.make_starts(20, 14, 2, 0), factr=1e4)
    assert len(calls) == res["calls"] and all(c.shape[0] <= 20 for c in calls)
    trials = np.concatenate(calls)
    assert trials.min() >= -1.0 and trials.max() <= 1.0
    assert res["x"].min() >= -1.0 and res["x"].max() <= 1.0
    assert res["converged"].sum() >= 15
    for s in np.flatnonzero(res["converged"]):
        _, g, st = ev(res["x"][s][None])
        assert st[0] == 0 and projected_gradient(res["x"][s], g[0]) <= 1e-4, s


def test_a_start_gives_the_same_bits_alone_and_among_25():
    D0 = initial_me_design()
    ev = numpy_evaluator(*BSQ_PRIOR, D_old=D0)
    starts = design.make_starts(25, 7, 2, 1)
    many = design.minimize_starts(ev, starts)
    for s in (0, 11, 24):
        one = design.minimize_starts(ev, starts[s:s + 1])
        assert np.array_equal(one["x"][0], many["x"][s]) and np.array_equal(one["f"][0], many["f"][s])
        assert one["iterations"][0] == many["iterations"][s] and one["converged"][0] == many["converged"][s]


def test_first_batch_agrees_with_scipy_lbfgsb():
    starts = design.make_starts(20, 14, 2, 0)
    res = design.minimize_starts(numpy_evaluator(*BSQ_PRIOR), starts)
    want = _scipy_best(starts, *BSQ_PRIOR)
    assert abs(res["f"].min() - want) <= 1e-8 * abs(want), (res["f"].min(), want)


def test_second_batch_agrees_with_scipy_lbfgsb():
    """Batch.Entropy.optim(D.old, 7, 2, 0.5, 1, 4, 25) (BSQ:1023 with the prior medians)."""
    D0 = initial_me_design()
    starts = design.make_starts(25, 7, 2, 0)
    res = design.minimize_starts(numpy_evaluator(*BSQ_PRIOR, D_old=D0), starts)
    want = _scipy_best(starts, *BSQ_PRIOR, D_old=D0)
    assert abs(-want - (-7.67936)) <= 1e-5
    assert abs(res["f"].min() - want) <= 1e-8 * abs(want), (res["f"].min(), want)


def test_infeasible_trials_make_the_line_search_back_off():
    """An evaluator that fails (status != 0) whenever two rows come closer than 0.2: the search pulls the two rows of a
    2-point design together, so it keeps running into failures, and still never returns a failing design."""
    calls, bad = [], []

    def evaluate(X):
        calls.append(X.copy())
        diff = X[:, 1, :] - X[:, 0, :]
        f = np.sum(diff ** 2, axis=1)
        g = np.stack([-2.0 * diff, 2.0 * diff], axis=1)
        st = (np.sqrt(f) < 0.2).astype(np.int32)
        bad.append(int(st.sum()))
        return np.where(st == 0, f, np.nan), np.where(st[:, None, None] == 0, g, np.nan), st

    starts = np.array([[[-0.9, -0.8], [0.7, 0.9]], [[0.5, -1.0], [-1.0, 1.0]], [[0.0, 0.0], [1.0, 0.0]]])
    res = design.minimize_starts(evaluate, starts)
    assert sum(bad) > 0
    for s in range(3):
        f, _, st = evaluate(res["x"][s][None])
        assert st[0] == 0 and np.isfinite(f[0]) and f[0] < 0.2 ** 2 * 1.5
        assert np.array_equal(res["f"][s], f[0])


def test_a_start_that_cannot_be_evaluated_is_never_the_result():
    ev = numpy_evaluator(*BSQ_PRIOR)
    starts = design.make_starts(3, 14, 2, 0)
    starts[1, 3] = starts[1, 4]   # two coincident rows: R is singular
    res = design.minimize_starts(ev, starts)
    assert not np.isfinite(res["f"][1]) and not res["converged"][1] and np.isfinite(res["f"][[0, 2]]).all()


def test_starts_are_latin_hypercubes_in_the_box():
    S = design.make_starts(4, 14, 2, 123)
    assert S.shape == (4, 14, 2) and S.min() >= -1.0 and S.max() <= 1.0
    for s in S:
        for k in range(2):
            assert sorted(np.floor((s[:, k] + 1.0) / 2.0 * 14).astype(int)) == list(range(14))
    assert np.array_equal(S, design.make_starts(4, 14, 2, 123))


def test_one_dimensional_scripts_have_no_design_search():
    from ccgp_amd.rsurface import CombinedGP1D
    for name in ("Entropy_optim", "Batch_Entropy_optim"):
        with pytest.raises(NotImplementedError):
            getattr(CombinedGP1D, name)(None, 14, 2, 0.5, 1.0, 4.0, 20)
