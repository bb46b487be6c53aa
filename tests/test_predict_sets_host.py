"""fit.compare_GP_sets and fit.study(lockstep_predict=True) without a GPU, over host stand-ins (predict_sets_handles) whose sets
methods go set by set through the single-set ones: the tables of the per-set loop in every key and bit, the grouping by
(n, d, m), one device call per route and group, the fallback to compare_GP where a model is not given, and the bindings'
place in the C ABI."""
import os

import numpy as np
import pytest

from conftest import synthetic_design
from ccgp_amd import api, cgp, fit
from predict_sets_handles import HostGP, SetsPredictHandle

OWN = ("seconds",)


def _same_table(got, want):
    assert list(got) == list(want)               # the keys in compare_GP's order
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(got[k], v, err_msg=k)
        else:
            assert got[k] is v, k                # the fitted models go into the table as they are


@pytest.fixture(scope="module")
def sets():
    """Four sets: three of n = 12, d = 2 (two with six test points, one with four) and one of n = 9."""
    out = []
    for c, (n, m) in enumerate([(12, 6), (12, 4), (12, 6), (9, 6)]):
        X, y = synthetic_design(n, 2, 40 + c)
        Xt, yt = synthetic_design(m, 2, 70 + c)
        out.append((X, y * (1.0 + 0.2 * c) + 0.3 * c * X[:, 0], Xt, yt * (1.0 + 0.2 * c)))
    return out


@pytest.fixture(scope="module")
def host(sets):
    h = SetsPredictHandle()
    krige = [fit.ordinary_kriging_fit(h, s[0], s[1], starts=3, rng=c) for c, s in enumerate(sets)]
    cgps = [cgp.CGP(h, s[0], s[1], num_starts=2, rng=c + 5) for c, s in enumerate(sets)]
    return h, krige, cgps


def _args(sets):
    draws = [np.array([[0.5, 1.0, 9.0 + c], [0.4, 2.0, 7.0]]) for c in range(len(sets))]
    s2 = [1.0 + 0.1 * c for c in range(len(sets))]
    return [s[2] for s in sets], 0.05, [s[3] for s in sets], draws, [s[0] for s in sets], s2, [s[1] for s in sets]


def test_compare_gp_sets_returns_the_tables_of_the_per_set_loop(sets, host):
    h, krige, cgps = host
    gp = HostGP(h, api.PRIOR_GV)
    Dt, alpha, yt, draws, D, s2, y = _args(sets)
    cg, sg = [dict(est=e) for e in cgps], [dict(est=e) for e in krige]
    want = [fit.compare_GP(gp, Dt[i], alpha, yt[i], draws[i], D[i], s2[i], y[i], exact=True, cgp=cg[i], single=sg[i])
            for i in range(4)]
    before, gp.calls["prediction"], h.shapes[:] = dict(h.calls), 0, []
    counts = {}
    got = fit.compare_GP_sets(gp, Dt, alpha, yt, draws, D, s2, y, cgp=cg, single=sg, counts=counts)
    assert len(got) == 4
    for g, w in zip(got, want):
        _same_table(g, w)
    # three groups (n, d, m) = (12, 2, 6) x 2, (12, 2, 4), (9, 2, 6): one call per route and group, no single-set call
    assert gp.calls == dict(prediction=0, prediction_sets=3) and gp.groups == [(2, 6), (1, 4), (1, 6)]
    made = {k: h.calls.get(k, 0) - before.get(k, 0) for k in h.calls}
    assert made["cgp_predict_sets"] == 3 and made["krige_predict_batch_sets"] == 3 and made["cgp_predict"] == 0
    assert [s[0] for s in h.shapes] == ["cgp_predict_sets", "krige_predict_batch_sets"] * 3
    assert [s[1:] for s in h.shapes[:2]] == [(2, 12, 2, 2, 6)] * 2
    assert counts == dict(calls=9)
    # without comparators: the Combined GP's columns alone
    plain = fit.compare_GP_sets(gp, Dt, alpha, yt, draws, D, s2, y)
    for g, w in zip(plain, want):
        assert list(g) == ["y_hat", "quant", "LL", "UL", "y_true"]
        for k in g:
            np.testing.assert_array_equal(g[k], w[k])


def test_a_set_whose_model_is_not_given_falls_back_to_compare_gp(sets, host):
    h, krige, cgps = host
    gp = HostGP(h, api.PRIOR_GV)
    Dt, alpha, yt, draws, D, s2, y = _args(sets)
    cg = [dict(est=cgps[0]), dict(num_starts=2, rng=6), dict(est=cgps[2]), False]       # set 1's CGP is still to be fitted
    sg = [dict(est=krige[0]), dict(est=krige[1]), dict(est=krige[2]), dict(est=krige[3])]
    before = dict(h.calls)
    got = fit.compare_GP_sets(gp, Dt, alpha, yt, draws, D, s2, y, cgp=cg, single=sg)
    made = {k: h.calls.get(k, 0) - before.get(k, 0) for k in h.calls}
    # set 1 goes per set: its CGP is fitted there (the fit's own final state is a cgp_predict call) and then predicted
    assert gp.calls["prediction"] == 1 and made["cgp_predict"] == 2 and made["cgp_state_batch"] > 0
    assert made["cgp_predict_sets"] == 1 and made["krige_predict_batch_sets"] == 2                       # sets 0, 2 | 3
    want1 = fit.compare_GP(gp, Dt[1], alpha, yt[1], draws[1], D[1], s2[1], y[1], exact=True, cgp=cg[1], single=sg[1])
    assert list(got[1]) == list(want1)
    for k, v in want1.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(got[1][k], v, err_msg=k)
    assert "y_hat_CGP" not in got[3] and "y_hat_single" in got[3] and got[0]["CGP"] is cgps[0]


def test_study_with_the_prediction_in_lockstep_writes_the_same_files(sets, host, tmp_path):
    h = host[0]
    three = [sets[0], sets[2], sets[1]]           # two shapes (n, d, m): (12, 2, 6) twice and (12, 2, 4)
    arms = {}
    for on in (False, True):
        gp = HostGP(h, api.PRIOR_GV)
        before = dict(h.calls)
        arms[on] = fit.study(gp, three, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], cgp=dict(num_starts=2, rng=5),
                             single=True, lockstep_predict=on, out_dir=str(tmp_path / str(on)))
        arms[on]["made"] = {k: h.calls.get(k, 0) - before.get(k, 0) for k in h.calls}
        arms[on]["gp"] = dict(gp.calls)
    on, off = arms[True], arms[False]
    for i in range(3):
        assert list(on["tables"][i]) == list(off["tables"][i])
        for k, v in off["tables"][i].items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(on["tables"][i][k], v, err_msg=k)
        assert on["summaries"][i] == off["summaries"][i]
        with open(os.path.join(tmp_path, "True", "results_%d.txt" % (i + 1)), "rb") as a, \
                open(os.path.join(tmp_path, "False", "results_%d.txt" % (i + 1)), "rb") as b:
            assert a.read() == b.read()
    assert on["pooled"] == off["pooled"]
    assert off["gp"] == dict(prediction=3, prediction_sets=0) and on["gp"] == dict(prediction=0, prediction_sets=2)
    # (each CGP fit ends with one cgp_predict call for its final state: three in either arm)
    assert off["made"]["cgp_predict"] == 3 + 3 and on["made"]["cgp_predict"] == 3 and on["made"]["cgp_predict_sets"] == 2
    assert on["made"]["krige_predict_batch_sets"] == 2
    # two groups x three models = 6 device calls, against 3 sets x 3 models through compare_GP
    assert on["calls"]["predict"] == 6 and off["calls"]["predict"] == 9
    for k in ("sigma2", "single", "cgp", "laplace", "metro"):
        assert on["calls"][k] == off["calls"][k]
    # a comparator whose model is not fitted in lockstep stays in compare_GP, set after set
    gp = HostGP(h, api.PRIOR_GV)
    r = fit.study(gp, three, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], sigma2s=off["sigma2"],
                  cgp=dict(num_starts=2, rng=5), single=True, lockstep_fits=False, lockstep_predict=True)
    assert gp.calls == dict(prediction=3, prediction_sets=0)
    for i in range(3):
        np.testing.assert_array_equal(r["tables"][i]["y_hat_CGP"], off["tables"][i]["y_hat_CGP"])


def test_the_bindings_are_declared():
    for name, n_args in (("ccgp_predict_batch_sets", 17), ("ccgp_krige_predict_batch_sets", 19), ("ccgp_predict_summary_sets", 19),
                         ("ccgp_cgp_predict_sets", 14)):
        assert name in api.SIGNATURES and len(api.SIGNATURES[name][1]) == n_args, name
    for m in ("predict_batch_sets", "krige_predict_batch_sets", "predict_summary_sets", "cgp_predict_sets"):
        assert hasattr(api.Handle, m)
    h = api.Handle.__new__(api.Handle)    # no device: the shape checks fail before the handle is read
    Xs, ys = np.zeros((2, 5, 2)), np.zeros((2, 5))
    for bad in (lambda: h.predict_batch_sets(Xs, ys, [1.0, 1.0], 2, np.ones((3, 5)), [0, 1, 0], np.zeros((2, 4, 2))),
                lambda: h.predict_batch_sets(Xs, ys, [1.0, 1.0], 2, np.ones((3, 6)), [0, 1, 0], np.zeros((3, 4, 2))),
                lambda: h.krige_predict_batch_sets(Xs, ys, 1, np.ones((3, 3)), [0, 1], None, np.zeros((2, 4, 2)), api.VAR_UNBIASED),
                lambda: h.predict_summary_sets(Xs, ys, [1.0, 1.0], 2, np.ones((3, 6)), [0, 1, 0], np.zeros((2, 4, 3)), (0.1, 0.9))):
        with pytest.raises(ValueError):
            bad()
