"""Reference for the composite GP of Ba & Joseph as the scripts carry it (CGP, GV:58-236; predict.CGP, GV:245-317), shared by
tests/test_cgp_ref.py (host), tests/test_gpu_cgp.py (device) and tests/golden/recover_cgp_gv.py.

A parameter row is (lambda, theta[d], alpha[d], bw) on the scale of the design it is evaluated on.  With G = exp(-D(theta)),
L = exp(-D(alpha)), Gbw = exp(-D(bw theta)), D(r)_ij = sum_k r_k (x_ik - x_jk)^2, the state is (GV:108-129)

    s = 1;  four times:  Q = G + lambda diag(sqrt s) L diag(sqrt s),  beta = 1'Q^-1 y / 1'Q^-1 1,  temp = Q^-1 (y - beta 1),
                         e = y - beta - G temp,  s = (Gbw e^2) / (Gbw 1),  sf = mean(s),  s /= sf;
    a fifth Q from the final s:  beta, temp,  tau2 = (y - beta 1)' temp / n,  val = log det Q + n log tau2.

With a held-out row (the jackknife, GV:167-198) the same runs on the n - 1 other points, and the held-out point is predicted
as predict.CGP would: v = (gbw'e^2 / gbw'1) / sf from the fourth pass, q = g + lambda sqrt(v) sqrt(s) * l, beta + q'temp.

Every solve goes through one LDL' written here (unit lower L, pivots d), in the dtype asked for: np.float64, or np.longdouble
as the oracle's long-double routines do it.  A pivot <= n eps (the device's rule for a solve() the reference would refuse)
stops the evaluation: status = the pivot's 1-based index, NaN everywhere.

NumpyHandle stands in for api.Handle.cgp_state_batch / cgp_predict so that cgp.CGP runs without a device.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def corr(A, B, rate):
    """exp(-sum_k rate_k (a_k - b_k)^2) for the rows of A against the rows of B (Stand_PSI GV:96-101, GV:289-291)."""
    diff = A[:, None, :] - B[None, :, :]
    return np.exp(-((diff * diff) * rate).sum(-1))


def ldl(Q, tol):
    """Q = L diag(d) L' without pivoting -> (L with unit diagonal, d, 0), or (None, None, k) at the first pivot k (1-based)
    that is not > tol."""
    n = Q.shape[0]
    A = Q.copy()
    dv = np.empty(n, dtype=Q.dtype)
    for k in range(n):
        piv = A[k, k]
        if not piv > tol:
            return None, None, k + 1
        dv[k] = piv
        col = A[k + 1:, k].copy()
        lk = col / piv
        A[k + 1:, k + 1:] -= np.outer(lk, col)
        A[k + 1:, k] = lk
    Lm = np.tril(A, -1)
    Lm[np.diag_indices(n)] = 1
    return Lm, dv, 0


def forward(Lm, B):
    """L^-1 B (B: [n] or [n, r])."""
    Z = np.array(B, dtype=Lm.dtype, copy=True)
    for k in range(Lm.shape[0] - 1):
        Z[k + 1:] -= np.multiply.outer(Lm[k + 1:, k], Z[k]) if Z.ndim == 2 else Lm[k + 1:, k] * Z[k]
    return Z


def backward(Lm, Z):
    """L'^-1 Z."""
    Xs = np.array(Z, dtype=Lm.dtype, copy=True)
    for k in range(Lm.shape[0] - 1, 0, -1):
        Xs[:k] -= np.multiply.outer(Lm[k, :k], Xs[k]) if Xs.ndim == 2 else Lm[k, :k] * Xs[k]
    return Xs


def split_row(row, d, T):
    row = np.asarray(row, dtype=np.float64).ravel()
    if row.shape[0] != 2 * d + 2:
        raise ValueError("a CGP parameter row has 2 d + 2 = %d entries" % (2 * d + 2))
    r = row.astype(T)
    return r[0], r[1:1 + d], r[1 + d:1 + 2 * d], r[1 + 2 * d]


def state(X, y, row, skip=-1, dtype=np.float64):
    """The CGP state at one parameter row -> dict(status, val, beta, tau2, loo, s, res2, temp, sf, s11, u = Q^-1 1, L, d,
    Q: the fifth matrix, n: points used).  loo is NaN without a held-out row."""
    T = np.dtype(dtype).type
    X = np.asarray(X, dtype=np.float64).astype(T)
    y = np.asarray(y, dtype=np.float64).ravel().astype(T)
    lam, theta, alpha, bw = split_row(row, X.shape[1], T)
    x0 = None
    if skip is not None and skip >= 0:
        keep = np.arange(X.shape[0]) != skip
        x0, X, y = X[skip], X[keep], y[keep]
    n = X.shape[0]
    one = np.ones(n, dtype=T)
    G, Lc, Gbw = corr(X, X, theta), corr(X, X, alpha), corr(X, X, theta * bw)
    nan = T(np.nan)
    out = dict(status=0, val=nan, beta=nan, tau2=nan, loo=nan, n=n, s=None, res2=None, temp=None, sf=nan)
    s = one.copy()
    res2 = sf = None
    with np.errstate(all="ignore"):
        for rep in range(5):
            rs = np.sqrt(s)
            Q = G + lam * (rs[:, None] * Lc * rs[None, :])
            Lm, dv, bad = ldl(Q, T(n * EPS))
            if bad:
                out["status"] = bad
                return out
            W = backward(Lm, forward(Lm, np.stack([y, one], axis=1)) / dv[:, None])
            s11 = one @ W[:, 1]
            beta = (one @ W[:, 0]) / s11
            temp = W[:, 0] - beta * W[:, 1]
            if rep == 4:
                break
            e = y - beta - G @ temp
            res2 = e * e
            sn = (Gbw @ res2) / (Gbw @ one)
            sf = sn.sum() / T(n)
            s = sn / sf
        tau2 = ((y - beta) @ temp) / T(n)
        val = np.log(dv).sum() + T(n) * np.log(tau2)
        out.update(val=val, beta=beta, tau2=tau2, s=s, res2=res2, temp=temp, sf=sf, s11=s11, u=W[:, 1], L=Lm, d=dv, Q=Q)
        if x0 is not None:
            g, l, gbw = corr(x0[None], X, theta)[0], corr(x0[None], X, alpha)[0], corr(x0[None], X, theta * bw)[0]
            v = ((gbw @ res2) / (gbw @ one)) / sf
            q = g + lam * np.sqrt(v) * np.sqrt(s) * l
            out["loo"] = beta + q @ temp
    return out


def predict(X, y, row, Xtest, dtype=np.float64, st=None):
    """predict.CGP(..., PI = TRUE) (GV:287-307) -> ([m, 6]: Yp gp lp v Y_low Y_up, the state).  q'Q^-1 q by forward
    substitution on the kept factor."""
    T = np.dtype(dtype).type
    st = state(X, y, row, -1, dtype) if st is None else st
    Xt = np.asarray(Xtest, dtype=np.float64).astype(T)
    m = Xt.shape[0]
    if st["status"]:
        return np.full((m, 6), np.nan), st
    X = np.asarray(X, dtype=np.float64).astype(T)
    lam, theta, alpha, bw = split_row(row, X.shape[1], T)
    with np.errstate(all="ignore"):
        g, l, gbw = corr(Xt, X, theta), corr(Xt, X, alpha), corr(Xt, X, theta * bw)
        v = ((gbw @ st["res2"]) / gbw.sum(1)) / st["sf"]
        rs = np.sqrt(st["s"])
        q = g + lam * np.sqrt(v)[:, None] * (l * rs[None, :])
        Yp = st["beta"] + q @ st["temp"]
        gp = st["beta"] + g @ st["temp"]
        lp = lam * np.sqrt(v) * ((l * rs[None, :]) @ st["temp"])
        Z = forward(st["L"], q.T)
        qQq = (Z * Z / st["d"][:, None]).sum(0)
        q1 = q @ st["u"]
        ppp = 1 + lam * v - qQq + (1 - q1) ** 2 / st["s11"]
        ppp = np.where(ppp < 0, T(0), ppp)
        half = T(1.96) * np.sqrt(st["tau2"] * ppp)
    return np.stack([Yp, gp, lp, v, Yp - half, Yp + half], axis=1), st


class NumpyHandle:
    """cgp_state_batch / cgp_predict of api.Handle on the host in fp64.  Counts its calls and the rows they carried."""

    def __init__(self):
        self.calls = 0
        self.points = 0

    def cgp_state_batch(self, X, y, params, skip=None):
        params = np.atleast_2d(np.asarray(params, dtype=np.float64))
        B = params.shape[0]
        self.calls += 1
        self.points += B
        val, beta, tau2, loo = (np.full(B, np.nan) for _ in range(4))
        status = np.zeros(B, dtype=np.int32)
        for b in range(B):
            r = state(X, y, params[b], -1 if skip is None else int(skip[b]))
            status[b] = r["status"]
            val[b], beta[b], tau2[b], loo[b] = r["val"], r["beta"], r["tau2"], r["loo"]
        return val, beta, tau2, (None if skip is None else loo), status

    def cgp_predict(self, X, y, row, Xtest):
        self.calls += 1
        out, st = predict(X, y, row, Xtest)
        if st["status"]:
            return out, None, int(st["status"])
        keep = dict(s=np.asarray(st["s"], dtype=np.float64), res2=np.asarray(st["res2"], dtype=np.float64),
                    temp=np.asarray(st["temp"], dtype=np.float64), sf=float(st["sf"]), beta=float(st["beta"]),
                    tau2=float(st["tau2"]))
        return np.asarray(out, dtype=np.float64), keep, 0


# ---- the yardstick of the device tests (and of fp64 against long double on the host) ------------------------------------
BAND_C = 8.0


def cond1(st):
    """cond_1 of the fifth Q of a state."""
    return float(np.linalg.cond(np.asarray(st["Q"], dtype=np.float64), 1))


def scales(st, y, out=None):
    """The cancellation-free magnitude of each output of a long-double state (and of its predict columns `out`):
      val                 n            (n log tau2: n times the relative error of tau2)
      beta, loo, Yp, gp, lp, Y_low, Y_up   max |y|   (predictions: sums of terms of the size of the data)
      tau2                sum |y - beta| |temp| / n   (the quadratic form without its cancellation)
      v                   v + 2 max |e| max |y| / sf: e = y - beta - G temp is a difference of terms of size |y|, so it carries
                          their absolute error, e^2 carries 2 |e| times that, and v is a ratio of weighted means of e^2 to sf."""
    ymax = float(np.abs(np.asarray(y, dtype=np.float64)).max())
    n = st["n"]
    ys = np.asarray(y, dtype=np.float64)
    if ys.shape[0] != n:    # the state was formed with a row held out: tau2's sum runs over its own points
        ys = None
    temp = np.asarray(st["temp"], dtype=np.float64)
    s = dict(val=float(n), beta=ymax, loo=ymax, Yp=ymax, gp=ymax, lp=ymax, Y_low=ymax, Y_up=ymax)
    s["tau2"] = float(np.abs(temp).sum()) * 2.0 * ymax / n if ys is None else float(
        (np.abs(ys - float(st["beta"])) * np.abs(temp)).sum() / n)
    emax = float(np.sqrt(np.asarray(st["res2"], dtype=np.float64).max()))
    vmax = 0.0 if out is None else float(np.abs(np.asarray(out[:, 3], dtype=np.float64)).max())
    s["v"] = vmax + 2.0 * emax * ymax / float(st["sf"])
    return s


def band(n, cond, scale, C=BAND_C):
    return C * n * EPS * cond * scale


COLS = ("Yp", "gp", "lp", "v", "Y_low", "Y_up")
