"""Host stand-ins for api.Handle that the tests of the host layers (fit, cgp) share.  Not a test module.

SetsHandle answers from the fp64 restatements of the device arithmetic; ClosedFormHandle answers from closed-form
objectives, which costs nothing and is enough where a test is about WHICH methods a routine calls, how often and with how
many rows.  Both record every call a routine makes (the calls a sets method makes inside itself are not counted)."""
import numpy as np

import cgp_ref
import krige_ref
import profile_ref
from ccgp_amd import api
from oracle import ccgp_oracle as orc


class SetsHandle:
    """profile_batch, cgp_state_batch, cgp_predict, krige_predict_batch and logpost_sets on the host; the *_sets methods go
    set by set through the single-set ones.  calls: single-set and sets calls made by a fit, each counted once; log: the
    same calls in order as (method, rows)."""

    def __init__(self):
        self.profile, self.cgp = profile_ref.NumpyHandle(), cgp_ref.NumpyHandle()
        self.memo = {}
        self.calls = dict(profile_batch=0, profile_batch_sets=0, cgp_state_batch=0, cgp_state_batch_sets=0, cgp_predict=0)
        self.log = []
        self.inner = False

    def _count(self, name, rows=1):
        if not self.inner:
            self.calls[name] = self.calls.get(name, 0) + 1
            self.log.append((name, int(rows)))

    def _rows(self, tag, fn, X, y, rows, extra):
        """fn(row index) per row, remembered by the bytes of (set, row, extra)."""
        key0 = (tag, np.ascontiguousarray(X).tobytes(), np.ascontiguousarray(y).tobytes())
        out = []
        for b in range(len(rows)):
            key = key0 + (rows[b].tobytes(), extra[b])
            if key not in self.memo:
                self.memo[key] = fn(b)
            out.append(self.memo[key])
        return out

    # ---- single-set calls
    def profile_batch(self, X, y, K, params, grad=False):
        self._count("profile_batch", len(np.atleast_2d(params)))
        X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
        P = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)

        def one(b):
            ll, s2, beta, g, st = self.profile.profile_batch(X, y, K, P[b:b + 1], grad=True)
            return ll[0], s2[0], beta[0], g[0], st[0]
        r = self._rows("profile%d" % K, one, X, y, P, [0] * len(P))
        g = np.stack([v[3] for v in r]) if grad else None
        return (np.array([v[0] for v in r]), np.array([v[1] for v in r]), np.array([v[2] for v in r]), g,
                np.array([v[4] for v in r], dtype=np.int32))

    def cgp_state_batch(self, X, y, params, skip=None):
        self._count("cgp_state_batch", len(np.atleast_2d(params)))
        X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
        P = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
        sk = [-1] * len(P) if skip is None else [int(s) for s in skip]

        def one(b):
            v = self.cgp.cgp_state_batch(X, y, P[b:b + 1], skip=None if skip is None else [sk[b]])
            return v[0][0], v[1][0], v[2][0], (np.nan if v[3] is None else v[3][0]), v[4][0]
        r = self._rows("cgp", one, X, y, P, sk)
        cols = [np.array([v[k] for v in r]) for k in range(4)]
        return cols[0], cols[1], cols[2], (None if skip is None else cols[3]), np.array([v[4] for v in r], dtype=np.int32)

    def cgp_predict(self, X, y, row, Xtest):
        self._count("cgp_predict")
        return self.cgp.cgp_predict(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel(), row, Xtest)

    def krige_predict_batch(self, X, y, K, params, sigma2, Xtest, form):
        assert form == api.VAR_PLUGIN and len(params) == 1
        r = krige_ref.device_restatement(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel(),
                                         np.asarray(params[0], dtype=np.float64), K, np.asarray(Xtest, dtype=np.float64))
        return r["mean"][None], (sigma2[0] * r["plug_unit"])[None], np.array([r["beta"]]), None, np.zeros(1, dtype=np.int32)

    def logpost_sets(self, Xs, ys, sigma2s, prior, theta_t, set_of, prior_pars=None):
        out = [orc.logpost(Xs[c], t, ys[c], sigma2s[c], "GV") for t, c in zip(np.atleast_2d(theta_t), set_of)]
        val, beta = np.array([o["val"] for o in out]), np.array([o["beta"] for o in out])
        return val, beta, val, np.zeros(len(out), dtype=np.int32)

    # ---- the sets calls: the single-set ones, set by set
    def _by_set(self, name, call, set_of, B, nout):
        self._count(name, B)
        set_of = np.asarray(set_of)
        assert set_of.shape == (B,)
        out = [None] * nout
        self.inner = True
        try:
            for c in np.unique(set_of):
                rows = np.flatnonzero(set_of == c)
                for k, v in enumerate(call(int(c), rows)):
                    if v is None:
                        continue
                    if out[k] is None:
                        out[k] = np.empty((B,) + v.shape[1:], dtype=v.dtype)
                    out[k][rows] = v
        finally:
            self.inner = False
        return tuple(out)

    def profile_batch_sets(self, Xs, ys, K, params, set_of, grad=True):
        P = np.atleast_2d(params)
        return self._by_set("profile_batch_sets", lambda c, rows: self.profile_batch(Xs[c], ys[c], K, P[rows], grad), set_of,
                            len(P), 5)

    def cgp_state_batch_sets(self, Xs, ys, params, set_of, skip=None):
        P = np.atleast_2d(params)
        sk = None if skip is None else np.asarray(skip)
        return self._by_set("cgp_state_batch_sets",
                            lambda c, rows: self.cgp_state_batch(Xs[c], ys[c], P[rows], None if sk is None else sk[rows]),
                            set_of, len(P), 5)


class ClosedFormHandle(SetsHandle):
    """SetsHandle with every single-set answer a closed form of the parameter row and of the set's mean response (so that
    two sets differ), plus logpost_batch, loo_batch and a logpost_sets that goes set by set like the other sets methods.
    The objectives are smooth with one optimum: a fit on them ends after a few dozen calls."""

    @staticmethod
    def _arrays(X, y, params):
        return (np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel(),
                np.atleast_2d(np.asarray(params, dtype=np.float64)))

    def profile_batch(self, X, y, K, params, grad=False):
        X, y, P = self._arrays(X, y, params)
        self._count("profile_batch", len(P))
        dev = np.log(P[:, K:]) - (0.5 + 0.1 * y.mean())
        g = np.concatenate([np.zeros((len(P), K)), -2.0 * dev / P[:, K:]], axis=1) if grad else None
        return (-np.sum(dev ** 2, axis=1), 1.0 + P[:, K:].sum(axis=1), np.full(len(P), y.mean()), g,
                np.zeros(len(P), dtype=np.int32))

    def cgp_state_batch(self, X, y, params, skip=None):
        X, y, P = self._arrays(X, y, params)
        self._count("cgp_state_batch", len(P))
        val = np.sum((P - 0.3 - 0.01 * y.mean()) ** 2, axis=1)
        loo = None if skip is None else 0.9 * y[np.asarray(skip, dtype=int)] + P[:, 0]
        return val, np.full(len(P), y.mean()), 1.0 + P[:, 0], loo, np.zeros(len(P), dtype=np.int32)

    def cgp_predict(self, X, y, row, Xtest):
        X, y, P = self._arrays(X, y, row)
        self._count("cgp_predict")
        Xt = np.asarray(Xtest, dtype=np.float64).reshape(-1, X.shape[1])
        out = np.repeat((Xt.sum(axis=1) + P[0, 0])[:, None], 6, axis=1) + np.arange(6)
        n = X.shape[0]
        return out, dict(s=np.full(n, P[0, 0]), res2=(y - y.mean()) ** 2, temp=y * P[0, -1], sf=2.0, beta=y.mean(),
                         tau2=1.0 + P[0, 0]), 0

    def logpost_batch(self, X, y, sigma2, prior, theta_t, prior_pars=None):
        X, y, T = self._arrays(X, y, theta_t)
        self._count("logpost_batch", len(T))
        val = -2.0 * np.sum((T - 0.1 * y.mean() * np.arange(1, T.shape[1] + 1)) ** 2, axis=1) - 0.5 * np.log(sigma2)
        return val, y.mean() + T[:, 0], val, np.zeros(len(T), dtype=np.int32)

    def logpost_sets(self, Xs, ys, sigma2s, prior, theta_t, set_of, prior_pars=None):
        T = np.atleast_2d(theta_t)
        return self._by_set("logpost_sets",
                            lambda c, rows: self.logpost_batch(Xs[c], ys[c], sigma2s[c], prior, T[rows], prior_pars),
                            set_of, len(T), 4)

    def krige_predict_batch(self, X, y, K, params, sigma2, Xtest, form):
        raise AssertionError("not part of the closed-form stand-in")

    def loo_batch(self, X, y, K, params, sigma2, form):
        X, y, P = self._arrays(X, y, params)
        self._count("loo_batch", len(P))
        mean = 0.9 * y[None] + P[:, K:].sum(axis=1)[:, None]
        var = (1.0 if sigma2 is None else np.asarray(sigma2, dtype=np.float64)[:, None]) * (1.0 + 0.0 * mean)
        return mean, var, np.full(len(P), y.mean()), np.ones(len(P)), np.zeros(len(P), dtype=np.int32)
