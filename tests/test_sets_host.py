"""The lockstep inference of a simulation study (fit.laplace_sets, fit.Metro_sets, fit.study) without a GPU: the evaluator is
injected -- `logpost_sets_fn(rows, set_of)` backed by the oracle's logpost on Ground-Vibrations training sets (the first 12
points of size-50 sets 1 - 3 for the chains, which keeps an evaluation at a fraction of a millisecond; whole sets for the
Nelder-Mead comparison).  What is held: a chain in the batch is fit.Metro's chain for its set and generator bit for bit, a chain
that finishes leaves the batch and the others do not notice, a set's Laplace estimate has the same bits alone and among others,
the lockstep Nelder-Mead stops no lower than scipy's, and fit.study groups by shape."""
import numpy as np
import pytest

from conftest import load_gv
from ccgp_amd import fit
from oracle import ccgp_oracle as orc

# How much lower in log-posterior fit.laplace_sets' mode may sit than fit.laplace's (scipy's Nelder-Mead): ten times the
# largest gap seen over the 17 Ground-Vibrations sets with the oracle evaluator (scripts/study_nm_margin.py; profiles/study.md).
# The measured gap is 0 on every set -- the lockstep search takes scipy's initial simplex, coefficients, acceptance rules and
# stop rule, and on these sets it visits the same vertices -- so the margin is 0: no lower at all.
NM_LARGEST_GAP = 0.0
NM_MARGIN = 10.0 * NM_LARGEST_GAP
START = np.array([1.0, 1.0, 0.0])
SMALL = dict(N=120, samp_size=40, batch_size=10)


def _evaluator(sets, s2, log=None):
    def fn(rows, set_of):
        rows = np.atleast_2d(rows)
        if log is not None:
            log.append(np.array(set_of).copy())
        out = [orc.logpost(sets[c][0], r, sets[c][1], s2[c], "GV") for r, c in zip(rows, set_of)]
        return np.array([o["val"] for o in out]), np.array([o["beta"] for o in out])
    return fn


@pytest.fixture(scope="module")
def small_sets():
    """12 points of GV size-50 sets 1 - 3, sigma2 = var(y), fit.laplace per set and fit.Metro per set with seed set + 1."""
    sets = [tuple(a[:12] for a in load_gv(50, i)[:2]) for i in (1, 2, 3)]
    s2 = [float(np.var(y, ddof=1)) for _, y in sets]
    fn = _evaluator(sets, s2)
    ests, chains, after = [], [], []
    for c in range(3):
        def one(rows, c=c):
            return fn(rows, [c] * len(np.atleast_2d(rows)))
        ests.append(fit.laplace(lambda rows: one(rows)[0], START))
        rng = np.random.default_rng(c + 1)
        chains.append(fit.Metro(None, START, SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, None, None, None, rng=rng,
                                logpost_fn=one))
        after.append(rng.random())
    return sets, s2, ests, chains, after


def _run_sets(sets, s2, ests, which, m, log=None):
    rngs = [np.random.default_rng(c + 1) for c in which]
    sub = [sets[c] for c in which]
    r = fit.Metro_sets(None, None, SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, [s[0] for s in sub],
                       [s2[c] for c in which], [s[1] for s in sub], rngs=rngs, speculate=m, laplace=[ests[c] for c in which],
                       logpost_sets_fn=_evaluator(sub, [s2[c] for c in which], log))
    return r, rngs


@pytest.mark.parametrize("m", [0, 3])
def test_lockstep_chains_are_metros_chains(small_sets, m):
    sets, s2, ests, chains, after = small_sets
    log = []
    r, rngs = _run_sets(sets, s2, ests, [0, 1, 2], m, log)
    per_chain = []
    for c in range(3):
        got, want = r["chains"][c], chains[c]
        np.testing.assert_array_equal(want["laplace"]["mode"], ests[c]["mode"])
        np.testing.assert_array_equal(got["sample"], want["sample"])
        np.testing.assert_array_equal(got["beta"], want["beta"])
        assert (got["accepted"], got["proposals"], got["geweke_p"]) == (want["accepted"], want["proposals"], want["geweke_p"])
        assert rngs[c].random() == after[c]
        per_chain.append(got["device_batches"])
    assert r["device_batches"] == max(per_chain) < sum(per_chain)
    steps = log[1:]                                   # the first call holds the chains' starting values
    assert len(steps) == r["device_batches"]
    per = 1 if m == 0 else 2 ** m - 1
    for step in steps:                                # every step carries every running chain's whole tree, in set order
        assert len(step) % per == 0 and list(step) == sorted(step)


def test_a_finished_chain_leaves_the_batch_and_the_others_do_not_notice(small_sets):
    sets, s2, ests, chains, _ = small_sets
    log = []
    r, _ = _run_sets(sets, s2, ests, [0, 1, 2], 0, log)
    props = [ch["proposals"] for ch in r["chains"]]
    assert len(set(props)) > 1                        # the chains do stop at different steps
    for c in range(3):
        present = [c in step for step in log[1:]]
        assert present == [True] * props[c] + [False] * (len(present) - props[c])
    first = int(np.argmin(props))
    others = [c for c in range(3) if c != first]
    r2, _ = _run_sets(sets, s2, ests, others, 0)
    for j, c in enumerate(others):
        for k in ("sample", "beta"):
            np.testing.assert_array_equal(r2["chains"][j][k], r["chains"][c][k])
        assert r2["chains"][j]["proposals"] == props[c]


def test_a_sets_laplace_estimate_does_not_depend_on_the_other_sets(small_sets):
    sets, s2, _, _, _ = small_sets
    fn = _evaluator(sets, s2)
    log = []

    def vals(rows, set_of):
        log.append(len(rows))
        return fn(rows, set_of)[0]

    starts = np.stack([START, START + 0.1, START - 0.2])
    together = fit.laplace_sets(vals, starts)
    hessian_call = log[-1]
    assert hessian_call == 3 * 4 * 6                  # the central-difference points of all sets in one call
    assert max(log[1:-1]) <= 3 * 4                    # per iteration four points per unfinished set, or its shrink
    for c in range(3):
        alone = fit.laplace_sets(lambda rows, set_of: fn(rows, [c] * len(rows))[0], starts[c:c + 1])[0]
        for k in ("mode", "var"):
            np.testing.assert_array_equal(alone[k], together[c][k])
        assert (alone["value"], alone["converged"], alone["iterations"]) == (together[c]["value"], True, together[c]["iterations"])


@pytest.mark.parametrize("size,sample", [(50, 1), (50, 7), (90, 5)])
def test_the_lockstep_search_stops_no_lower_than_scipys(size, sample):
    D, y = load_gv(size, sample)[:2]
    s2 = float(np.var(y, ddof=1))

    def one(rows):
        return np.array([orc.logpost(D, r, y, s2, "GV")["val"] for r in np.atleast_2d(rows)])

    ref = fit.laplace(one, START)
    got = fit.laplace_sets(lambda rows, set_of: one(rows), START[None])[0]
    print("scipy %.15g  lockstep %.15g  gap %.3e" % (ref["value"], got["value"], ref["value"] - got["value"]))
    assert got["converged"] and ref["converged"]
    assert got["value"] >= ref["value"] - NM_MARGIN
    assert got["value"] == one(got["mode"][None])[0]  # the reported value is the value at the reported mode


def test_study_groups_by_shape_and_refuses_nothing_to_do():
    """Grouping is about shapes, not values: five sets of the two Ground-Vibrations shapes in mixed order, a quadratic
    log-posterior per set as the evaluator (its centre depends on the set), and a recording stand-in for compare_GP."""
    rng = np.random.default_rng(0)
    shapes = [(50, 9), (90, 9), (50, 9), (90, 9), (50, 9)]
    sets = [(rng.random(s), rng.random(s[0]), rng.random((4, s[1])), rng.random(4) + i) for i, s in enumerate(shapes)]
    asked, compared = [], []

    def factory(idx):
        asked.append(list(idx))
        assert len({sets[i][0].shape for i in idx}) == 1

        def fn(rows, set_of):
            centre = np.array([0.1 * idx[c] for c in set_of])[:, None]
            return -0.5 * ((np.atleast_2d(rows) - centre) ** 2).sum(axis=1) / 0.04, np.asarray(set_of, dtype=float)
        return fn

    def compare(gp, D_test, alpha, y_test, draws, D_train, sigma2, y_train, exact, cgp, single):
        i = int(round(y_test.min() // 1))
        compared.append((i, D_train.shape, sigma2))
        assert exact and draws.shape == (30, 3)
        m = len(y_test)
        return dict(y_hat=y_test + 0.1, quant=np.full(m, 0.5), LL=y_test - 1.0, UL=y_test + 1.0, y_true=y_test)

    r = fit.study(None, sets, 0.05, SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, net_samp_size=30,
                  sigma2s=[1.0 + i for i in range(5)], rngs=[1, 2, 3, 4, 5], logpost_sets_fn=factory, compare_fn=compare)
    assert asked == [[0, 2, 4], [1, 3]] and r["groups"] == {(50, 9): [0, 2, 4], (90, 9): [1, 3]}
    assert compared == [(i, (shapes[i][0], 9), 1.0 + i) for i in range(5)]
    for i in range(5):                                # every chain went back to its own set: its draws centre on 0.1 i
        assert abs(np.log(r["draws"][i][:, 1]).mean() - 0.1 * i) < 0.15
        assert (r["beta"][i] == (i // 2 if i % 2 == 0 else i // 2)).all()
    assert r["pooled"] == fit.comparison_summary({k: np.concatenate([t[k] for t in r["tables"]]) for k in r["tables"][0]})
    assert r["pooled"]["rmspe"] == pytest.approx(0.1) and r["calls"]["predict"] == 5 and r["calls"]["sigma2"] == 0
    alone = fit.study(None, [sets[2]], 0.05, SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, net_samp_size=30,
                      sigma2s=[3.0], rngs=[3], logpost_sets_fn=lambda idx: (lambda rows, set_of: factory([2])(rows, set_of)),
                      compare_fn=compare)
    np.testing.assert_array_equal(alone["draws"][0], r["draws"][2])     # a set's fit depends on that set only
    with pytest.raises(ValueError):
        fit.study(None, [], 0.05, 10, 5, 5, 0.5)
