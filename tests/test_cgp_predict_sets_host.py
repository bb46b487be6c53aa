"""cgp.predict_CGP_sets without a GPU, over a host stand-in (predict_sets_handles.PredictSetsHandle) whose sets method goes
row by row through cgp_predict: the same dicts as the per-model loop, the grouping by (n, d, m), one device call per group,
and the binding's place in the C ABI."""
import numpy as np
import pytest

from ccgp_amd import api, cgp
from predict_sets_handles import PredictSetsHandle


def _model(n, d, seed):
    rng = np.random.default_rng(seed)
    return {"X": rng.random((n, d)), "yobs": rng.standard_normal(n), "lambda": 0.1 + rng.random(), "theta": 1.0 + rng.random(d),
            "alpha": 5.0 + rng.random(d), "bandwidth": 0.5}


def _equal(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if want[k] is None:
            assert got[k] is None
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("PI", [False, True])
def test_the_dicts_of_the_per_model_loop_one_call_per_shape_and_test_size(PI):
    rng = np.random.default_rng(3)
    # five models: three of shape (12, 3) at 7 sites, one of that shape at 4 sites, one of shape (9, 2) at 7 sites
    ests = [_model(12, 3, 1), _model(9, 2, 2), _model(12, 3, 3), _model(12, 3, 4), _model(12, 3, 5)]
    news = [rng.random((7, 3)), rng.random((7, 2)), rng.random((4, 3)), rng.random((7, 3)), rng.random((7, 3))]
    loop_h, sets_h = PredictSetsHandle(), PredictSetsHandle()
    want = [cgp.predict_CGP(loop_h, e, u, PI=PI) for e, u in zip(ests, news)]
    got = cgp.predict_CGP_sets(sets_h, ests, news, PI=PI)
    assert len(got) == 5
    for g, w in zip(got, want):
        _equal(g, w)
    assert loop_h.calls["cgp_predict"] == 5 and loop_h.calls.get("cgp_predict_sets", 0) == 0
    assert sets_h.calls["cgp_predict"] == 0 and sets_h.calls["cgp_predict_sets"] == 3
    # (C, n, d, B, m) per call, groups in order of first appearance; every model is its own set
    assert [s[1:] for s in sets_h.shapes] == [(3, 12, 3, 3, 7), (1, 9, 2, 1, 7), (1, 12, 3, 1, 4)]
    assert sets_h.log == [("cgp_predict_sets", 3), ("cgp_predict_sets", 1), ("cgp_predict_sets", 1)]


def test_newdata_is_reshaped_as_predict_CGP_reshapes_it_and_lengths_must_match():
    e = _model(6, 2, 9)
    h = PredictSetsHandle()
    flat = np.arange(8.0) / 8.0           # four sites of two inputs, given flat
    _equal(cgp.predict_CGP_sets(h, [e], [flat], PI=True)[0], cgp.predict_CGP(h, e, flat, PI=True))
    assert cgp.predict_CGP_sets(h, [], []) == []
    with pytest.raises(ValueError):
        cgp.predict_CGP_sets(h, [e], [])


def test_a_state_that_cannot_be_factorised_raises_and_names_its_model():
    class Failing(PredictSetsHandle):
        def cgp_predict(self, X, y, row, Xtest):
            out, keep, _ = super().cgp_predict(X, y, row, Xtest)
            return (out * np.nan, None, 2) if np.ravel(row)[0] == 0.0 else (out, keep, 0)

    ests = [_model(6, 2, 1), dict(_model(6, 2, 2), **{"lambda": 0.0})]
    news = [np.zeros((3, 2)), np.zeros((3, 2))]
    with pytest.raises(RuntimeError, match="model 1 .*pivot 2"):
        cgp.predict_CGP_sets(Failing(), ests, news)
    with pytest.raises(RuntimeError, match="pivot 2"):
        cgp.predict_CGP(Failing(), ests[1], news[1])


def test_the_binding_is_declared_and_checks_its_shapes_before_the_library_is_asked():
    name = "ccgp_cgp_predict_sets"
    assert name in api.SIGNATURES and len(api.SIGNATURES[name][1]) == 14
    assert hasattr(api.Handle, "cgp_predict_sets")
    h = api.Handle.__new__(api.Handle)    # no device: every check below fails before the handle is read
    Xs, ys = np.zeros((2, 5, 2)), np.zeros((2, 5))
    for bad in (lambda: h.cgp_predict_sets(Xs[0], ys, np.ones((3, 6)), [0, 1, 0], np.zeros((2, 4, 2))),
                lambda: h.cgp_predict_sets(Xs, ys, np.ones((3, 5)), [0, 1, 0], np.zeros((2, 4, 2))),       # 2 d + 2 = 6 columns
                lambda: h.cgp_predict_sets(Xs, ys, np.ones((3, 6)), [0, 1], np.zeros((2, 4, 2))),          # one set per row
                lambda: h.cgp_predict_sets(Xs, ys, np.ones((3, 6)), [0, 1, 0], np.zeros((4, 2))),          # [C, m, d]
                lambda: h.cgp_predict_sets(Xs, ys, np.ones((3, 6)), [0, 1, 0], np.zeros((3, 4, 2))),       # one block per set
                lambda: h.cgp_predict_sets(Xs, ys, np.ones((3, 6)), [0, 1, 0], np.zeros((2, 4, 3)))):      # d inputs per site
        with pytest.raises(ValueError):
            bad()
