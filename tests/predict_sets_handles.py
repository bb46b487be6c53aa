"""Host stand-ins for api.Handle with the sets forms of the predictions, and for the CombinedGP surface on top of them.  Not a
test module.

The sets methods go set by set (row by row) through the single-set ones -- so a routine over them must return what the
per-set loop returns -- and record their calls: `calls` / `log` as in host_handles.SetsHandle (the single-set calls made
inside a sets method are not counted), `shapes`: one (method, C, n, d, B, m) per sets call, in order."""
import numpy as np

from host_handles import ClosedFormHandle, SetsHandle


class _PredictSets:
    def cgp_predict_sets(self, Xs, ys, params, set_of, Xtests):
        Xs, Xt, P = np.asarray(Xs, dtype=np.float64), np.asarray(Xtests, dtype=np.float64), np.atleast_2d(params)
        set_of = np.asarray(set_of)
        C, n, d = Xs.shape
        assert Xt.ndim == 3 and Xt.shape[0] == C and Xt.shape[2] == d and set_of.shape == (len(P),) and P.shape[1] == 2 * d + 2
        self._count("cgp_predict_sets", len(P))
        self.shapes.append(("cgp_predict_sets", C, n, d, len(P), Xt.shape[1]))
        out, keeps, st = np.empty((len(P), Xt.shape[1], 6)), [], np.zeros(len(P), dtype=np.int32)
        self.inner = True
        try:
            for b, c in enumerate(set_of):
                o, k, s = self.cgp_predict(Xs[c], ys[c], P[b], Xt[c])
                out[b], st[b] = o, s
                keeps.append(k)
        finally:
            self.inner = False
        return out, keeps, st

    def krige_predict_batch_sets(self, Xs, ys, K, params, set_of, sigma2, Xtests, form):
        Xs, Xt, P = np.asarray(Xs, dtype=np.float64), np.asarray(Xtests, dtype=np.float64), np.atleast_2d(params)
        set_of = np.asarray(set_of)
        C, n, d = Xs.shape
        assert Xt.ndim == 3 and Xt.shape[0] == C and Xt.shape[2] == d and set_of.shape == (len(P),)
        self._count("krige_predict_batch_sets", len(P))
        self.shapes.append(("krige_predict_batch_sets", C, n, d, len(P), Xt.shape[1]))
        rows = []
        self.inner = True
        try:
            for b, c in enumerate(set_of):
                rows.append(self.krige_predict_batch(Xs[c], ys[c], K, P[b:b + 1], [sigma2[b]], Xt[c], form))
        finally:
            self.inner = False
        return (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows]),
                None, np.concatenate([r[4] for r in rows]))


class PredictSetsHandle(_PredictSets, ClosedFormHandle):
    """ClosedFormHandle with cgp_predict_sets (its single-GP prediction is not part of the closed-form stand-in)."""

    def __init__(self):
        super().__init__()
        self.shapes = []


class SetsPredictHandle(_PredictSets, SetsHandle):
    """SetsHandle (the fp64 restatements) with cgp_predict_sets and krige_predict_batch_sets."""

    def __init__(self):
        super().__init__()
        self.shapes = []


class HostGP:
    """What compare_GP, compare_GP_sets and study ask of a CombinedGP, on a stand-in handle.  prediction_sets goes set by set
    through prediction; calls: how often each was asked; groups: the (sets, sites) of every prediction_sets call."""
    script = "GV"

    def __init__(self, h, prior):
        self.h, self.cfg = h, dict(prior=prior, npar=3)
        self.calls, self.groups, self.inner = dict(prediction=0, prediction_sets=0), [], False

    def prediction(self, D_test, alpha, draws, D_train, sigma2, y_train):
        if not self.inner:
            self.calls["prediction"] += 1
        m = len(D_test)
        centre = np.full(m, float(np.mean(y_train))) + float(np.mean(draws)) * np.asarray(D_test)[:, 0]
        half = np.sqrt(sigma2) * np.ones(m)
        return dict(y_hat=centre, Quant=np.full(m, 0.5), LL=centre - half, UL=centre + half)

    def prediction_sets(self, D_tests, alpha, draws, D_trains, sigma2s, y_trains, y_tests=None):
        self.calls["prediction_sets"] += 1
        assert len({np.shape(D) for D in D_trains}) == 1 and len({np.shape(D) for D in D_tests}) == 1
        self.groups.append((len(D_trains), len(D_tests[0])))
        self.inner = True
        try:
            each = zip(D_tests, draws, D_trains, sigma2s, y_trains)
            return [self.prediction(Dt, alpha, dr, D, s2, y) for Dt, dr, D, s2, y in each]
        finally:
            self.inner = False
