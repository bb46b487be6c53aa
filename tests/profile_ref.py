"""References for the likelihood with sigma2 concentrated out (ccgp_profile_batch), shared by tests/test_profile_ref.py
(host) and tests/test_gpu_profile.py (device).

For a draw (w, theta) with M = sum_c w_c^2 R_c(theta_c):
    beta = 1'M^-1 y / 1'M^-1 1,  Q = (y - beta 1)'M^-1 (y - beta 1),  sigma2_hat = Q / n,
    l_p  = -(n log 2 pi + n log sigma2_hat + log det M + n) / 2,
and d l_p / d row = d l / d row of the mode-0 likelihood l(row; beta, sigma2) taken at (beta_hat, sigma2_hat): l_p(row) =
max over (beta, sigma2) of l, the maximiser is interior and unique (Q > 0), so the partial derivatives with respect to beta
and sigma2 vanish there and the total derivative of l_p is the partial derivative of l (envelope theorem).

profile_exact builds all of it from oracle.ccgp_oracle.loglik_grad_parts / grad_from_parts: the parts at sigma2 = 1 give
sigma2_hat = r' Sinv r / n; the parts and the closed-form gradient are then taken again at that sigma2_hat.

NumpyHandle is a host stand-in for api.Handle.profile_batch (fp64, LAPACK) so that fit.ordinary_kriging_fit -- the
lockstep optimiser and its chain rule -- runs without a device.
"""
import numpy as np

from oracle import ccgp_oracle as orc


def sigma2_exact(X, y, row, K, d, dtype=np.longdouble, Rc=None):
    """(sigma2_hat in dtype, the parts at sigma2 = 1 it was formed from)."""
    dtype = np.dtype(dtype).type
    p1 = orc.loglik_grad_parts(X, y, row, K, d, 1.0, dtype, Rc=Rc)
    yv = np.asarray(y, dtype=dtype).reshape(-1)
    r = yv - p1["beta"]
    return (r @ (p1["Sinv"] @ r)) / dtype(yv.shape[0]), p1


def profile_exact(X, y, row, K, d, dtype=np.longdouble, Rc=None):
    """dict(sigma2, loglik, beta, grad, scale, parts) in dtype; parts = loglik_grad_parts at sigma2_hat (for cond1 and the
    cancellation-free sizes of oracle.loglik_beta_scales).  Rc: the component matrices of a family other than the Gaussian
    (the gradient then means nothing: grad_from_parts differentiates the Gaussian kernel)."""
    dtype = np.dtype(dtype).type
    p1 = orc.loglik_grad_parts(X, y, row, K, d, 1.0, dtype, Rc=Rc)
    yv = np.asarray(y, dtype=dtype).reshape(-1)
    r = yv - p1["beta"]
    s2 = (r @ (p1["Sinv"] @ r)) / dtype(yv.shape[0])
    parts = orc.loglik_grad_parts(X, y, row, K, d, s2, dtype, Rc=p1["Rc"])
    grad, scale = orc.grad_from_parts(parts, X, row, K, d, s2)
    return dict(sigma2=s2, loglik=parts["loglik"], beta=parts["beta"], grad=grad, scale=scale, parts=parts)


def profile_loglik(X, y, row, K, d, dtype=np.longdouble):
    """l_p alone (for central differences)."""
    return profile_exact(X, y, row, K, d, dtype)["loglik"]


class NumpyHandle:
    """profile_batch of api.Handle on the host: fp64 closed form, one Gaussian component per call of the fit (any K works).
    A matrix that LAPACK cannot factorise gives status 1 and NaN, as a failed draw does on the device.  Counts its calls
    and the points they carried."""

    def __init__(self):
        self.calls = 0
        self.points = 0

    def profile_batch(self, X, y, K, params, grad=False):
        X = np.asarray(X, dtype=np.float64)
        params = np.atleast_2d(np.asarray(params, dtype=np.float64))
        B, P = params.shape
        d = X.shape[1]
        self.calls += 1
        self.points += B
        ll, s2, beta = np.full(B, np.nan), np.full(B, np.nan), np.full(B, np.nan)
        g = np.full((B, P), np.nan) if grad else None
        st = np.zeros(B, dtype=np.int32)
        for b in range(B):
            try:
                with np.errstate(all="ignore"):
                    r = profile_exact(X, y, params[b], K, d, np.float64)
            except (np.linalg.LinAlgError, ValueError):
                st[b] = 1
                continue
            if not np.isfinite(r["loglik"]):
                st[b] = 1
                continue
            ll[b], s2[b], beta[b] = r["loglik"], r["sigma2"], r["beta"]
            if grad:
                g[b] = r["grad"]
        return ll, s2, beta, g, st
