"""numpy/scipy restatement of the reference's per-draw GP evaluation.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.  What pins it: the reference holds no tests and no
golden vectors, but it holds ONE recorded output, `Ground Vibrations Emulator/Results/Size 50 Results 1.txt`; its
single-GP columns are reproduced by corr_matrix / corr_vec / solve / beta_mle / the predictive formulas to 1e-8 on all
450 numbers (tests/test_reference_pins.py), the hyperprior pair hard-coded at HX:774-775 is the argmax of
choose_hyperpars, and the Combined-GP columns agree up to Monte-Carlo noise.  PARITY UNPINNED for what no reference-held
number covers: the log-likelihood scalar itself (arbitrated by oracle/mp_check.py at 50 digits and by LAPACK), the Halton
start index, every Matern / spline / ADV result, and base R's solve() tolerance rule (restated from its documentation).

Every function names the reference lines it follows.  Abbreviations:
  HX  = Heat Exchanger Emulator/Combined GP Heat Exchanger.R
  GV  = Ground Vibrations Emulator/Combined GP Ground Vibrations.R
  ISO = 2D Codes and Designs/2D Combined GP Isotropic Public.R
  ADV = 2D Codes and Designs/2D Combined GP Isotropic Advanced.R
  ANI = 2D Codes and Designs/2D Combined GP Anisotropic Public.R
  D1  = 1D Codes and Designs/1D Combined GP Public.R
  D1F = 1D Codes and Designs/1D Combined GP Two Families Public.R
  BSQ = Batch Sequential ME Designs/Batch Sequential ME Design.R

The operation ORDER of the R code is kept (expanded-distance form, LU inverse for
R.Inv, Cholesky + chol2inv inside dmnorm) because that order is what a drop-in has
to agree with; third-party pieces that are not under /root/reference
(mnormt::dmnorm, fOptions::runif.halton, pscl::qigamma, base besselK) are
restated from their published definitions.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg as sla
import scipy.special as sps
import scipy.stats as sst

LOG_2PI = math.log(2.0 * math.pi)


# --------------------------------------------------------------------------- a1/a2
def corr_matrix(X, theta):
    """Gaussian Gram matrix, one scale per input dimension.

    HX:328-337 (general d), ANI:351-360 (d = 2, theta = c(theta1, theta2)).
    R = exp(-(U + t(U) + V)), U[i, .] = sum_k theta_k x_ik^2, V = -2 X Theta X'.
    """
    X = np.asarray(X, dtype=np.float64)
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    n = X.shape[0]
    Theta = np.diag(theta)
    u = ((X ** 2) @ Theta).sum(axis=1)          # apply(X^2 %*% Theta, 1, sum)
    U = np.repeat(u[:, None], n, axis=1)        # matrix(u, n, n, byrow = F)
    V = -2.0 * ((X @ Theta) @ X.T)
    dist = (U + U.T) + V
    return np.exp(-dist)


def corr_matrix_iso(X, theta):
    """HX:347-356 (= GV:346, ISO:350, ADV:353-362, BSQ:347): Theta = theta * I_d."""
    X = np.asarray(X, dtype=np.float64)
    return corr_matrix(X, np.full(X.shape[1], float(theta)))


# --------------------------------------------------------------------------- a3
def corr_vec(x, X, theta):
    """Correlations between one new site and the design. ANI:369-377 / HX:367-375.

    r_i = exp(-((theta' x^2) - 2 (X Theta x)_i + sum_k theta_k x_ik^2)).
    """
    X = np.asarray(X, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    Theta = np.diag(theta)
    a = float(theta @ (x ** 2))
    b = 2.0 * ((X @ Theta) @ x)
    c = ((X ** 2) @ Theta).sum(axis=1)
    return np.exp(-((a - b) + c))


def corr_vec_iso(x, X, theta):
    """HX:367-375."""
    X = np.asarray(X, dtype=np.float64)
    return corr_vec(x, X, np.full(X.shape[1], float(theta)))


# --------------------------------------------------------------------------- a4/a5
def _mix(p, A1, A2):
    return (p ** 2 * A1 + (1.0 - p) ** 2 * A2) / (p ** 2 + (1.0 - p) ** 2)


def mixed_corr_matrix_iso(D, p, theta1, theta2):
    """HX:408-415 (GV, ISO, BSQ identical; ADV:414-421 passes lambda as theta2)."""
    return _mix(p, corr_matrix_iso(D, theta1), corr_matrix_iso(D, theta2))


def mixed_corr_vec_iso(x, D, p, theta1, theta2):
    """HX:425-431."""
    return _mix(p, corr_vec_iso(x, D, theta1), corr_vec_iso(x, D, theta2))


def mixed_corr_matrix_aniso(D, p, theta1, theta2, lam):
    """ANI:399-406: R2 uses (1+lambda)*(theta1, theta2)."""
    t = np.array([theta1, theta2], dtype=np.float64)
    return _mix(p, corr_matrix(D, t), corr_matrix(D, (1.0 + lam) * t))


def mixed_corr_vec_aniso(x, D, p, theta1, theta2, lam):
    """ANI:416-422."""
    t = np.array([theta1, theta2], dtype=np.float64)
    return _mix(p, corr_vec(x, D, t), corr_vec(x, D, (1.0 + lam) * t))


# --------------------------------------------------------------------------- a6/a7
def beta_mle(R_inv, y):
    """HX:384-388: 1' R.Inv y / sum(R.Inv)."""
    R_inv = np.asarray(R_inv, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    one = np.ones(y.shape[0])
    return float(((one @ R_inv) @ y) / R_inv.sum())


def sigma2_mle(R_inv, y, beta):
    """HX:394-399 / D1:411-415: (y - beta 1)' R.Inv (y - beta 1) / n."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    u = y - beta * np.ones(y.shape[0])
    return float(((u @ np.asarray(R_inv, dtype=np.float64)) @ u) / y.shape[0])


# --------------------------------------------------------------------------- a12/a13
def solve_inverse(R, tol=None):
    """base R solve(R) (HX:454) = solve.default(a, tol = .Machine$double.eps) -> La_solve: LAPACK dgesv(R, I), an error
    for an exactly singular U ("system is exactly singular"), THEN rcond = dgecon("1", LU, ||R||_1) and an error when
    rcond < tol ("system is computationally singular: reciprocal condition number = ...").  The reference wraps the
    call in try() and maps either error to R.Inv <- NA (HX:454-455).  Base R is not in the reference tree; restated
    from its documented behaviour (?solve: "tol: the tolerance for detecting linear dependencies in the columns of a").
    tol: the 1-D scripts pass tol = 1e-16 (D1:440)."""
    A = np.asarray(R, dtype=np.float64)
    x = np.linalg.inv(A)                      # dgesv(A, I); raises LinAlgError on an exactly singular U
    lu, _, info = sla.lapack.dgetrf(A)        # the same factorisation again, for the condition estimate
    anorm = np.abs(A).sum(axis=0).max()
    rcond, info = sla.lapack.dgecon(lu, anorm, norm="1")
    if not rcond >= (np.finfo(np.float64).eps if tol is None else tol):
        raise np.linalg.LinAlgError("system is computationally singular: reciprocal condition number = %g" % rcond)
    return x


def dmnorm_log(x, mean, varcov):
    """mnormt::dmnorm(x, mean, varcov, log = TRUE) -- package source not in the
    reference tree; restated from its definition: pd.solve symmetrises, takes the
    upper Cholesky factor, chol2inv, log.det = 2 sum log diag(U);
    logPDF = -(Q + d log 2pi + log.det)/2 with Q = (x-mean)' Sigma^-1 (x-mean).
    Call sites: HX:460, HX:570, GV:448, ISO:451, ADV:465, ADV:573, ANI:455, BSQ:448.
    Raises numpy.linalg.LinAlgError when varcov is not positive definite (R: error).
    """
    S = np.asarray(varcov, dtype=np.float64)
    S = (S + S.T) / 2.0
    d = S.shape[0]
    xc = np.asarray(x, dtype=np.float64).reshape(-1) - mean
    U = sla.cholesky(S, lower=False)
    inv, info = sla.lapack.dpotri(U, lower=0)
    if info != 0:
        raise np.linalg.LinAlgError("dpotri failed")
    inv = np.triu(inv) + np.triu(inv, 1).T
    log_det = 2.0 * np.log(np.diag(U)).sum()
    Q = float((inv @ xc) @ xc)
    return -(Q + d * LOG_2PI + log_det) / 2.0


# --------------------------------------------------------------------------- a8
PRIOR_VARIANTS = ("HX", "ADV", "GV", "ISO", "BSQ", "D1", "ANI")


def log_jacobian(theta_t):
    """-phi - 2 log(1+e^-phi) + psi1 + psi2 [+ zeta]  (HX:461, ANI:459)."""
    t = np.asarray(theta_t, dtype=np.float64)
    val = -t[2] - 2.0 * math.log(1.0 + math.exp(-t[2])) + t[0] + t[1]
    if t.shape[0] == 4:
        val += t[3]
    return float(val)


def log_prior(theta_t, variant, prior_pars=None):
    """The script-specific log-prior on the transformed scale.

    HX:462 / ADV:467 inverse-gamma with passed (a1,b1,a2,b2); GV:450; ISO:453 =
    BSQ:450 = D1:636; ANI:462.
    """
    t = np.asarray(theta_t, dtype=np.float64)
    psi1, psi2 = t[0], t[1]
    th1, th2 = math.exp(psi1), math.exp(psi2)
    if variant in ("HX", "ADV"):
        a1, b1, a2, b2 = prior_pars
        return float(-(a1 + 1.0) * psi1 - b1 / th1 - (a2 + 1.0) * psi2 - b2 / th2)
    if variant == "GV":
        return float(-4.0 * psi1 - 1.0 / th1 - 6.0 * psi2 - 75.0 / th2)
    if variant in ("ISO", "BSQ", "D1"):
        return float(-4.0 * psi1 - 2.0 / th1 - 6.0 * psi2 - 16.0 / th2)
    if variant == "ANI":
        zeta = t[3]
        lam = math.exp(zeta)
        return float(-psi1 - psi1 ** 2 / 2.0 - psi2 - psi2 ** 2 / 2.0 - 4.0 * zeta - 4.0 / lam)
    raise ValueError(variant)


def logpost(D, theta_t, y, sigma2, variant="HX", prior_pars=None):
    """Joint log-posterior of one transformed draw -> dict(val, beta, R_inv).

    HX:441-466, GV:429-454, ISO:433-457, ADV:447-471, ANI:433-467, BSQ:430-454.
    Steps kept in the reference's order: unpack, Mixed.corr.matrix, solve(R) (NA on
    failure), beta.MLE, dmnorm(y, sum(beta), (p^2+(1-p)^2) sigma2 R), + log-Jacobian
    + log-prior.  ADV also returns like = exp(log.like) (ADV:470).
    """
    t = np.asarray(theta_t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    theta1, theta2 = math.exp(t[0]), math.exp(t[1])
    p = 1.0 / (1.0 + math.exp(-t[2]))
    if variant == "ANI":
        R = mixed_corr_matrix_aniso(D, p, theta1, theta2, math.exp(t[3]))
    else:
        R = mixed_corr_matrix_iso(D, p, theta1, theta2)
    try:
        R_inv = solve_inverse(R)
    except np.linalg.LinAlgError:
        return dict(val=float("nan"), beta=float("nan"), R_inv=None, like=float("nan"))
    beta = beta_mle(R_inv, y)
    log_like = dmnorm_log(y, beta, (p ** 2 + (1.0 - p) ** 2) * sigma2 * R)
    val = log_like + log_jacobian(t) + log_prior(t, variant, prior_pars)
    return dict(val=float(val), beta=beta, R_inv=R_inv, like=math.exp(log_like),
                log_like=float(log_like))


# --------------------------------------------------------------------------- a9
def runif_halton(N):
    """fOptions::runif.halton(N, 1): base-2 radical inverse of 1..N (1/2, 1/4, 3/4, ...).
    Package source not in the reference tree; restated from the van der Corput
    definition (HX:554).  If the package used another start index the grid means
    move at O(1/N); flagged in DESIGN.md."""
    out = np.empty(N, dtype=np.float64)
    for i in range(1, N + 1):
        f, r, k = 0.5, 0.0, i
        while k:
            if k & 1:
                r += f
            k >>= 1
            f *= 0.5
        out[i - 1] = r
    return out


def qigamma(p, alpha, beta):
    """pscl::qigamma(p, alpha, beta) = 1 / qgamma(1 - p, shape alpha, rate beta)
    (HX:555-556).  Equals scipy.stats.invgamma.ppf(p, alpha, scale=beta)."""
    p = np.asarray(p, dtype=np.float64)
    return 1.0 / (sst.gamma.ppf(1.0 - p, alpha) / beta)


def cond_like_log(D, y, p, theta1, theta2, sigma2, tau):
    """log of cond.like, HX:561-572: dmnorm(y, 0, sigma2 (p^2+(1-p)^2) R + tau^2 11')."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    sigma2_t = sigma2 * (p ** 2 + (1.0 - p) ** 2)
    R = mixed_corr_matrix_iso(D, p, theta1, theta2)
    return dmnorm_log(y, 0.0, sigma2_t * R + tau ** 2 * np.ones((n, n)))


def likeli_hyperpars(D, y, theta1_pars, theta2_pars, sigma2, N=1000, tau=50.0,
                     return_logs=False):
    """HX:549-575 (N=1000, tau=50) / ADV:552-578 (N=1728, tau=100): mean over N Halton
    points of exp(cond.like); p, theta1 and theta2 all come from the SAME quantile."""
    u = runif_halton(N)
    th1 = qigamma(u, theta1_pars[0], theta1_pars[1])
    th2 = qigamma(u, theta2_pars[0], theta2_pars[1])
    logs = np.array([cond_like_log(D, y, u[j], th1[j], th2[j], sigma2, tau)
                     for j in range(N)])
    if return_logs:
        return logs
    return float(np.mean(np.exp(logs)))


def choose_hyperpars(D, y, hyper, sigma2, N=1000, tau=50.0, take_log=True):
    """HX:584-595 (log of the mean, HX:591) / ADV:588-599 (no log, ADV:595).
    Returns (argmax row index 0-based, per-row values)."""
    hyper = np.asarray(hyper, dtype=np.float64)
    vals = np.empty(hyper.shape[0])
    for i in range(hyper.shape[0]):
        m = likeli_hyperpars(D, y, hyper[i, 0:2], hyper[i, 2:4], sigma2, N, tau)
        vals[i] = math.log(m) if take_log else m
    return int(np.argmax(vals)), vals


# --------------------------------------------------------------------------- a10/a11
def factors(R_inv, beta, y):
    """HX:604-613: mean.factor = R.Inv (y - beta), var.factor1 = colSums(R.Inv),
    var.factor2 = sum(var.factor1)."""
    R_inv = np.asarray(R_inv, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    mean_factor = R_inv @ (y - beta)
    v1 = R_inv.sum(axis=0)
    return mean_factor, v1, float(v1.sum())


def predict_post_from_factors(r, beta, mean_factor, v1, v2, R_inv, sigma2):
    """The arithmetic of predict.post once r is known (HX:667-670)."""
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    var = sigma2 * (1.0 - (r @ R_inv) @ r + (1.0 - v1 @ r) ** 2 / v2)
    mean = beta + mean_factor @ r
    return float(mean), float(var)


def predict_post_iso(x, D, y, p, theta1, theta2, sigma2):
    """HX:655-673 for one (draw, test point), recomputing the cached per-draw terms
    exactly as Metro/factors.frame would have stored them (HX:454-458, HX:604-613)."""
    R = mixed_corr_matrix_iso(D, p, theta1, theta2)
    R_inv = solve_inverse(R)
    beta = beta_mle(R_inv, y)
    mf, v1, v2 = factors(R_inv, beta, y)
    r = mixed_corr_vec_iso(x, D, p, theta1, theta2)
    return predict_post_from_factors(r, beta, mf, v1, v2, R_inv, sigma2)


def predict_post_aniso(x, D, y, p, theta1, theta2, lam, sigma2):
    """ANI:604-623."""
    R = mixed_corr_matrix_aniso(D, p, theta1, theta2, lam)
    R_inv = solve_inverse(R)
    beta = beta_mle(R_inv, y)
    mf, v1, v2 = factors(R_inv, beta, y)
    r = mixed_corr_vec_aniso(x, D, p, theta1, theta2, lam)
    return predict_post_from_factors(r, beta, mf, v1, v2, R_inv, sigma2)


def predict_table(D, y, draws, Xtest, sigma2, aniso=False):
    """(S x m) mean and variance tables: what prediction() consumes before its
    rnorm/quantile step (HX:686-693).  draws rows: (p, theta1, theta2[, lambda])."""
    draws = np.asarray(draws, dtype=np.float64)
    Xtest = np.asarray(Xtest, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    S, m = draws.shape[0], Xtest.shape[0]
    mean = np.empty((S, m))
    var = np.empty((S, m))
    betas = np.empty(S)
    for s in range(S):
        if aniso:
            p, t1, t2, lam = draws[s]
            R = mixed_corr_matrix_aniso(D, p, t1, t2, lam)
        else:
            p, t1, t2 = draws[s]
            R = mixed_corr_matrix_iso(D, p, t1, t2)
        R_inv = solve_inverse(R)
        beta = beta_mle(R_inv, y)
        betas[s] = beta
        mf, v1, v2 = factors(R_inv, beta, y)
        for j in range(m):
            if aniso:
                r = mixed_corr_vec_aniso(Xtest[j], D, p, t1, t2, lam)
            else:
                r = mixed_corr_vec_iso(Xtest[j], D, p, t1, t2)
            mean[s, j], var[s, j] = predict_post_from_factors(r, beta, mf, v1, v2, R_inv, sigma2)
    return mean, var, betas


# --------------------------------------------------------------------------- general K
def params_from_iso(p, theta1, theta2, d):
    """Pack an isotropic 2-component draw as the C-ABI row (w_1..w_K, theta_c,k)."""
    return np.concatenate([[p, 1.0 - p], np.full(d, theta1), np.full(d, theta2)])


def params_from_aniso(p, theta1, theta2, lam):
    return np.array([p, 1.0 - p, theta1, theta2, (1.0 + lam) * theta1, (1.0 + lam) * theta2])


def unpack_params(row, K, d):
    row = np.asarray(row, dtype=np.float64)
    return row[:K], row[K:].reshape(K, d)


def mixed_corr_matrix_general(X, w, Theta):
    """K-component generalisation of HX:408-415: sum_c w_c^2 R_c / sum_c w_c^2."""
    w = np.asarray(w, dtype=np.float64)
    acc = None
    for c in range(w.shape[0]):
        Rc = w[c] ** 2 * corr_matrix(X, Theta[c])
        acc = Rc if acc is None else acc + Rc
    return acc / np.sum(w ** 2)


def mixed_corr_vec_general(x, X, w, Theta):
    w = np.asarray(w, dtype=np.float64)
    acc = None
    for c in range(w.shape[0]):
        rc = w[c] ** 2 * corr_vec(x, X, Theta[c])
        acc = rc if acc is None else acc + rc
    return acc / np.sum(w ** 2)


MEAN_PROFILE_BETA = 0
MEAN_ZERO_PLUS_TAU2 = 1


def loglik_general(X, y, w, Theta, sigma2, mean_mode=MEAN_PROFILE_BETA, tau2=0.0):
    """The likelihood term of logpost (mode 0: HX:454-460) or of cond.like (mode 1:
    HX:567-570) for K components.  Returns (loglik, beta).  Raises LinAlgError on a
    non-PD matrix (the C-ABI reports that through status[])."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = y.shape[0]
    w = np.asarray(w, dtype=np.float64)
    R = mixed_corr_matrix_general(X, w, Theta)
    c = sigma2 * np.sum(w ** 2)
    if mean_mode == MEAN_PROFILE_BETA:
        R_inv = solve_inverse(R)
        beta = beta_mle(R_inv, y)
        return dmnorm_log(y, beta, c * R), beta
    return dmnorm_log(y, 0.0, c * R + tau2 * np.ones((n, n))), 0.0


def loglik_grad_fd(X, y, row, K, d, sigma2, h=1e-6):
    """Central finite differences of the profiled log-likelihood with respect to the
    raw C-ABI parameter row -- the check for the build-defined gradient extension
    (the reference has no analytic gradient: LearnBayes::laplace differences
    numerically, HX:493)."""
    row = np.asarray(row, dtype=np.float64)
    g = np.empty_like(row)
    for j in range(row.shape[0]):
        e = np.zeros_like(row)
        e[j] = h * max(1.0, abs(row[j]))
        wp, Tp = unpack_params(row + e, K, d)
        wm, Tm = unpack_params(row - e, K, d)
        g[j] = (loglik_general(X, y, wp, Tp, sigma2)[0]
                - loglik_general(X, y, wm, Tm, sigma2)[0]) / (2.0 * e[j])
    return g


# --------------------------------------------------------------------------- entropy criteria (8(f)-4)
def cross_corr_matrix(D_old, D_new, theta):
    """BSQ:835-848: exp(-(U + V + W)), n.new x n.old, isotropic."""
    D_old, D_new = np.asarray(D_old, dtype=np.float64), np.asarray(D_new, dtype=np.float64)
    d = D_new.shape[1]
    Theta = np.diag(np.full(d, float(theta)))
    U = ((D_new ** 2) @ Theta).sum(axis=1)[:, None]
    V = -2.0 * ((D_new @ Theta) @ D_old.T)
    W = ((D_old ** 2) @ Theta).sum(axis=1)[None, :]
    return np.exp(-((U + V) + W))


def entropy(D, p, theta1, theta2):
    """BSQ:856-861: -det(R.mixed)."""
    return -float(np.linalg.det(mixed_corr_matrix_iso(D, p, theta1, theta2)))


def augmented_mixed_entropy(D_old, D_new, p, theta1, theta2):
    """BSQ:869-877 with R.old.Inv = solve(R.old) as in Batch.Entropy.optim (BSQ:924-925)."""
    R_old_inv = solve_inverse(mixed_corr_matrix_iso(D_old, p, theta1, theta2))
    R_cross = _mix(p, cross_corr_matrix(D_old, D_new, theta1), cross_corr_matrix(D_old, D_new, theta2))
    R_new = mixed_corr_matrix_iso(D_new, p, theta1, theta2)
    return -float(np.linalg.det(R_new - (R_cross @ R_old_inv) @ R_cross.T))


# --------------------------------------------------------------------------- config 1 (CPU plumbing)
def matern_corr(nu, h, theta):
    """D1:348-351: (2 sqrt(nu)|h|/theta)^nu K_nu(2 sqrt(nu)|h|/theta) / (Gamma(nu) 2^(nu-1)),
    1 at h = 0.  base besselK -> scipy.special.kv."""
    h = np.abs(np.asarray(h, dtype=np.float64))
    z = 2.0 * math.sqrt(nu) * h / theta
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        val = z ** nu * sps.kv(nu, z) / (sps.gamma(nu) * 2.0 ** (nu - 1.0))
    return np.where(h == 0.0, 1.0, val)


def corr_matrix_matern(nu, X, theta):
    """D1:368-374 (X is n x 1)."""
    x = np.asarray(X, dtype=np.float64).reshape(-1)
    return matern_corr(nu, x[:, None] - x[None, :], theta)


def corr_vec_matern(x, X, theta, nu):
    """D1:383-389."""
    return matern_corr(nu, float(x) - np.asarray(X, dtype=np.float64).reshape(-1), theta)


def log_likeli_1d(nu, theta, D, y):
    """D1:437-444 log.likeli(nu, theta, D.train, y.train) = log(det(R)) + n log(sigma2.MLE): the ordinary-kriging
    profile objective that MLEs() minimises with nlminb (D1:455-471); = D1F:527-537 with corr.matrix.Matern."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    R = corr_matrix_matern(nu, D, theta)
    R_inv = solve_inverse(R, tol=1e-16)
    beta = beta_mle(R_inv, y)
    s2 = sigma2_mle(R_inv, y, beta)
    return math.log(np.linalg.det(R)) + y.shape[0] * math.log(s2)


def logpost_1d(D, theta_t, y, sigma2, nu):
    """D1:609-641 (Matern nu, prior D1:636)."""
    t = np.asarray(theta_t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    theta1, theta2 = math.exp(t[0]), math.exp(t[1])
    p = 1.0 / (1.0 + math.exp(-t[2]))
    R = _mix(p, corr_matrix_matern(nu, D, theta1), corr_matrix_matern(nu, D, theta2))
    R_inv = solve_inverse(R)
    beta = beta_mle(R_inv, y)
    log_like = dmnorm_log(y, beta, (p ** 2 + (1.0 - p) ** 2) * sigma2 * R)
    val = log_like + log_jacobian(t) + log_prior(t, "D1")
    return dict(val=float(val), beta=beta, R_inv=R_inv)


def predict_post_1d(x, D, y, p, theta1, theta2, sigma2, nu):
    """D1:794-812 for one (draw, test point), recomputing the cached per-draw terms as
    factors.frame would have stored them (D1:760-781)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    R = _mix(p, corr_matrix_matern(nu, D, theta1), corr_matrix_matern(nu, D, theta2))
    R_inv = solve_inverse(R)
    beta = beta_mle(R_inv, y)
    mf, v1, v2 = factors(R_inv, beta, y)
    r = _mix(p, corr_vec_matern(x, D, theta1, nu), corr_vec_matern(x, D, theta2, nu))
    return predict_post_from_factors(r, beta, mf, v1, v2, R_inv, sigma2)


# --------------------------------------------------------------------------- two-family 1-D script (D1F)
def spline_corr(theta, h):
    """D1F:346-357 spline.corr.func(theta, h): the non-negative cubic spline correlation."""
    u = np.abs(np.asarray(h, dtype=np.float64)) / theta
    return np.where(u <= 0.5, 1.0 - 6.0 * u ** 2 + 6.0 * u ** 3, np.where(u <= 1.0, 2.0 * (1.0 - u) ** 3, 0.0))


def corr_matrix_spline(X, theta):
    """D1F:398-404."""
    x = np.asarray(X, dtype=np.float64).reshape(-1)
    return spline_corr(theta, x[:, None] - x[None, :])


def corr_vec_spline(x, X, theta):
    """D1F:412-418."""
    return spline_corr(theta, float(x) - np.asarray(X, dtype=np.float64).reshape(-1))


def corr_matrix_combined(X, p, theta1, theta2, nu):
    """D1F:453-462: (p^2 Matern(nu, theta1) + (1-p)^2 spline(theta2)) / (p^2 + (1-p)^2)."""
    return _mix(p, corr_matrix_matern(nu, X, theta1), corr_matrix_spline(X, theta2))


def corr_vec_combined(x, X, p, theta1, theta2, nu):
    """D1F:470-480 AS WRITTEN: `return(p^2*r1 + (1-p)^2*r2)/(p^2 + (1-p)^2)` returns before the
    division, so the vector is NOT normalised ("the D1F:479 quirk")."""
    return p ** 2 * corr_vec_matern(x, X, theta1, nu) + (1.0 - p) ** 2 * corr_vec_spline(x, X, theta2)


def logpost_2f(D, theta_t, y, sigma2, nu):
    """D1F:576-601 (prior D1F:596 = D1:636)."""
    t = np.asarray(theta_t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    theta1, theta2 = math.exp(t[0]), math.exp(t[1])
    p = 1.0 / (1.0 + math.exp(-t[2]))
    R = corr_matrix_combined(D, p, theta1, theta2, nu)
    R_inv = solve_inverse(R)
    beta = beta_mle(R_inv, y)
    log_like = dmnorm_log(y, beta, (p ** 2 + (1.0 - p) ** 2) * sigma2 * R)
    val = log_like + log_jacobian(t) + log_prior(t, "D1")
    return dict(val=float(val), beta=beta, R_inv=R_inv)


def predict_post_2f(x, D, y, p, theta1, theta2, sigma2, nu):
    """D1F:737-754 for one (draw, test point) -- with the un-normalised corr.vec.combined."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    R_inv = solve_inverse(corr_matrix_combined(D, p, theta1, theta2, nu))
    beta = beta_mle(R_inv, y)
    mf, v1, v2 = factors(R_inv, beta, y)
    r = corr_vec_combined(x, D, p, theta1, theta2, nu)
    return predict_post_from_factors(r, beta, mf, v1, v2, R_inv, sigma2)


def test_function_2d(x, y, code):
    """ANI:330-341: the five bivariate test simulators (needed to make y.train)."""
    if code == 1:
        return math.exp(-1.4 * x) * math.cos(7 * math.pi * x * y / 2) + math.log(x + y + 0.1)
    if code == 2:
        return (((x - 0.2) ** 2 - (y - 0.7) ** 2) * math.exp(-5 * ((x - 0.8) ** 2 + (y - 0.1) ** 2))
                * math.cos(10 * (x - 0.5) * y))
    if code == 3:
        return ((x - 0.5) ** 2 + 4 * (y - 0.8) ** 2) * (math.cos(math.pi * (x - 0.1)) + math.cos(math.pi * (y - 0.5)))
    if code == 4:
        return (math.sin(2 * x) + math.cos(4 * x)) * (math.sin(8 * y) + math.cos(4 * y))
    if code == 5:
        return math.sin(9 * x - 4.5) / (9 * x - 4.5) * math.sin(12 * y - 6) / (12 * y - 6)
    raise ValueError(code)


# --------------------------------------------------------------------------- analytic gradient, extended precision
# The reference has no gradient (HX:493 differences numerically), so the library's ccgp_loglik_grad_batch is held against
# the closed form it implements.  With Sigma = sigma2 sum_c w_c^2 R_c (the mixed matrix of mixed_corr_matrix_general times
# sigma2 sum_c w_c^2), alpha = Sigma^-1 (y - beta 1) and M = (alpha alpha' - Sigma^-1) / 2, the profiled log-likelihood has
#   d/dw_q     = sum_ab M_ab  2 sigma2 w_q R_q,ab
#   d/dtheta_qk = sum_ab M_ab (-sigma2 w_q^2 (x_ak - x_bk)^2 R_q,ab)
# (beta is stationary, so its own derivative drops out).  Evaluated in np.longdouble through the hand-written Cholesky
# below, or in fp64 through LAPACK; nothing here calls the device library.
LONGDOUBLE_EPS_MAX = 1e-18
# The per-component acceptance band of a device gradient (tests/test_gpu_gradient_exact.py states why this C):
#   |g_dev[j] - g_ref[j]| <= GRAD_TOL_C * eps * cond1(R) * (1 + rho) * scale[j],   rho = expanded_form_magnitude(...)
GRAD_TOL_C = 128.0


def expanded_form_magnitude(X, row, K, d):
    """rho = max_c,a 2 sum_k theta_ck x_ak^2: the size of the terms of the expanded exponent u_a + u_b - 2 sum_k theta_k x_ak x_bk
    (HX:352-355) that the device, like the reference scripts, evaluates.  Its absolute rounding, ~eps rho, is a relative
    perturbation of every kernel value that no algorithm downstream can undo."""
    X = np.asarray(X, dtype=np.float64)
    _, Th = unpack_params(row, K, d)
    return float(2.0 * ((X ** 2) @ np.asarray(Th, dtype=np.float64).T).max())


def grad_tolerance(scale, kappa, rho=0.0, c=GRAD_TOL_C):
    return c * np.finfo(np.float64).eps * kappa * (1.0 + rho) * np.asarray(scale, dtype=np.float64)


def require_extended_precision():
    """The long-double reference is only worth its name where long double is wider than fp64 (x87 80-bit: eps 1.1e-19)."""
    eps = float(np.finfo(np.longdouble).eps)
    if eps > LONGDOUBLE_EPS_MAX:
        raise RuntimeError("np.longdouble has eps %.3g > %.0e on this host: the extended-precision gradient reference "
                           "is unavailable (no fall-back to fp64)" % (eps, LONGDOUBLE_EPS_MAX))


def _log_2pi(dtype):
    """log(2 pi) in dtype: the fp64 constant is 1.4e-16 off, which n / 2 times over is a visible share of a rounding unit of
    the log-likelihood at n in the hundreds."""
    if dtype == np.float64:
        return LOG_2PI
    return np.log(dtype(8) * np.arctan(dtype(1)))


def _chol_inverse(A, dtype):
    """(Sigma^-1, log det Sigma) of a symmetric positive definite A.  fp64: LAPACK (dpotrf / dpotri).  long double: a
    column Cholesky, then L^-1 by forward substitution on the identity and Sigma^-1 = L^-T L^-1, vectorised over rows."""
    if dtype == np.float64:
        c, low = sla.cho_factor(np.asarray(A, dtype=np.float64), lower=True)
        inv, info = sla.lapack.dpotri(c, lower=1)
        if info != 0:
            raise np.linalg.LinAlgError("dpotri failed")
        inv = np.tril(inv) + np.tril(inv, -1).T
        return inv, 2.0 * float(np.log(np.diag(c)).sum())
    L = _chol_lower(A, dtype)
    Z = _lower_inverse(L, dtype)
    return Z.T @ Z, dtype(2) * np.log(np.diag(L)).sum()


def _chol_lower(A, dtype):
    """The lower Cholesky factor of a symmetric positive definite A in long double: a column Cholesky."""
    require_extended_precision()
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % j)
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def _lower_inverse(L, dtype):
    """Z = L^-1 (lower triangular) by forward substitution on the identity, vectorised over rows."""
    n = L.shape[0]
    Z = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        Z[i, :i] = -(L[i, :i] @ Z[:i, :i]) / L[i, i]
        Z[i, i] = dtype(1) / L[i, i]
    return Z


def _sq_dist(X, k, dtype):
    x = np.asarray(X[:, k], dtype=dtype)
    return (x[:, None] - x[None, :]) ** 2


def component_corr(X, theta_c, dtype=np.float64):
    """R_c in the direct squared-difference form (exp(-sum_k theta_ck (x_ak - x_bk)^2)), in dtype."""
    X = np.asarray(X, dtype=np.float64)
    acc = np.zeros((X.shape[0], X.shape[0]), dtype=dtype)
    for k in range(X.shape[1]):
        acc += dtype(theta_c[k]) * _sq_dist(X, k, dtype)
    return np.exp(-acc)


def loglik_grad_parts(X, y, row, K, d, sigma2, dtype=np.float64, Rc=None):
    """The pieces of the closed form in dtype: dict(Sigma, Sinv, Rc (list), M, alpha, u, loglik, beta).  u = Sigma^-1 1 /
    1' Sigma^-1 1 are the weights with beta = u' y.  Raises LinAlgError on a matrix that is not positive definite.
    Rc: the K component matrices in dtype, for a family other than the Gaussian (the 1-D scripts' Matern and spline: the row
    then supplies the weights only); default: component_corr of the row's theta."""
    X = np.asarray(X, dtype=np.float64)
    yv = np.asarray(y, dtype=dtype).reshape(-1)
    n = yv.shape[0]
    w, Th = unpack_params(row, K, d)
    s2 = dtype(sigma2)
    if Rc is None:
        Rc = [component_corr(X, Th[c], dtype) for c in range(K)]
    Sigma = np.zeros((n, n), dtype=dtype)
    for c in range(K):
        Sigma += (s2 * dtype(w[c]) ** 2) * Rc[c]
    Sinv, logdet = _chol_inverse(Sigma, dtype)
    s1 = Sinv.sum(axis=0)
    u = s1 / s1.sum()
    beta = u @ yv
    alpha = Sinv @ (yv - beta)
    q = (yv - beta) @ alpha
    ll = -(dtype(n) * _log_2pi(dtype) + logdet + q) / dtype(2)
    M = (np.outer(alpha, alpha) - Sinv) / dtype(2)
    return dict(Sigma=Sigma, Sinv=Sinv, Rc=Rc, M=M, alpha=alpha, u=u, loglik=ll, beta=beta)


def grad_from_parts(parts, X, row, K, d, sigma2, weights=None):
    """(grad, scale) from the closed form: grad[j] = sum_ab W_ab M_ab dSigma_j,ab, scale[j] = sum_ab W_ab |M_ab| |dSigma_j,ab|.
    weights: an n x n array W (default all ones); the test of the tolerance passes altered weights to model kernel bugs."""
    X = np.asarray(X, dtype=np.float64)
    M, Rc = parts["M"], parts["Rc"]
    dtype = M.dtype.type
    WM = M if weights is None else M * weights
    aWM = np.abs(WM)
    w, _ = unpack_params(row, K, d)
    s2 = dtype(sigma2)
    P = K + K * d
    grad = np.zeros(P, dtype=dtype)
    scale = np.zeros(P, dtype=dtype)
    for q in range(K):
        dw = dtype(2) * s2 * dtype(w[q]) * Rc[q]
        grad[q] = (WM * dw).sum()
        scale[q] = (aWM * np.abs(dw)).sum()
        cq = -s2 * dtype(w[q]) ** 2
        for k in range(d):
            dt = cq * (_sq_dist(X, k, dtype) * Rc[q])
            grad[K + q * d + k] = (WM * dt).sum()
            scale[K + q * d + k] = (aWM * np.abs(dt)).sum()
    return grad, scale


def loglik_grad_exact(X, y, row, K, d, sigma2, dtype=np.float64):
    """Closed-form gradient of the profiled log-likelihood with respect to the raw C-ABI row (w_1..w_K, theta_c,k).
    Returns (loglik, beta, grad, scale), all float64 arrays / scalars rounded from dtype (np.float64: LAPACK; np.longdouble:
    the hand-written Cholesky, about 1e-19 relative).  scale[j] = sum_ab |M_ab| |dSigma_ab / d row_j| is the cancellation-free
    size of component j: a perturbation of every term of the sum by a relative eps moves grad[j] by at most eps * scale[j]."""
    dtype = np.dtype(dtype).type
    parts = loglik_grad_parts(X, y, row, K, d, sigma2, dtype)
    grad, scale = grad_from_parts(parts, X, row, K, d, sigma2)
    return float(parts["loglik"]), float(parts["beta"]), grad.astype(np.float64), scale.astype(np.float64)


def loglik_beta_scales(parts, y):
    """Cancellation-free sizes of the log-likelihood and beta, in the sense of loglik_grad_exact's scale:
    loglik: n/2 + (|alpha|' |Sigma| |alpha|) / 2 (the log-determinant and the quadratic form); beta: sum_i |u_i| |y_i|."""
    n = parts["alpha"].shape[0]
    a = np.abs(parts["alpha"])
    s_ll = 0.5 * n + 0.5 * float(a @ np.abs(parts["Sigma"]) @ a)
    s_beta = float(np.abs(parts["u"]) @ np.abs(np.asarray(y, dtype=np.float64).reshape(-1)))
    return s_ll, s_beta


def cond1(A, A_inv):
    """1-norm condition number ||A||_1 ||A^-1||_1 from an accurate inverse."""
    return float(np.abs(np.asarray(A, np.float64)).sum(axis=0).max() * np.abs(np.asarray(A_inv, np.float64)).sum(axis=0).max())


def solve_inverse_exact(R, dtype=np.longdouble):
    """R^-1 of a symmetric positive definite R (solve(R), HX:454, for the matrices the device inverts) in dtype through
    _chol_inverse.  Returns the dtype array."""
    dtype = np.dtype(dtype).type
    inv, _ = _chol_inverse(np.asarray(R, dtype=dtype), dtype)
    return inv


def conditioned_row(X, K, d, rng, kappa_max=1e8, w=None):
    """A random anisotropic draw (w_1..w_K, theta_c,k) for the gradient tests whose mixed matrix has cond1 <= kappa_max:
    length scales spread over a factor 20 around the design spacing (n^(-1/d)), the last component rough, then every theta
    scaled up by 1.5 until the fp64 1-norm condition number is within bound.  w: the weights to use instead of random ones
    (the random ones are still drawn, so the length scales do not depend on it).  Returns (row, cond1)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    rough = 2.0 * n ** (2.0 / d) / d
    w_drawn = 0.2 + 0.6 * rng.random(K)
    w = w_drawn if w is None else np.asarray(w, dtype=np.float64)
    Th = rough * np.exp(rng.uniform(np.log(0.05), 0.0, size=(K, d)))
    Th[-1] = rng.uniform(rough, 2.0 * rough, d)
    for _ in range(200):
        kappa = float(np.linalg.cond(mixed_corr_matrix_general(X, w, Th), 1))
        if kappa <= kappa_max:
            return np.concatenate([w, Th.ravel()]), kappa
        Th = Th * 1.5
    raise RuntimeError("no draw with cond1 <= %g" % kappa_max)


# --------------------------------------------------------------------------- marginal likelihood (mean mode 1), extended precision
# cond.like (HX:561-572) factorises Sigma = Sigma0 + tau2 11', Sigma0 = sigma2 sum_c w_c^2 R_c, with mean 0.  With alpha =
# Sigma^-1 y and M = (alpha alpha' - Sigma^-1) / 2, d loglik = tr(M dSigma): a relative perturbation delta of every entry of
# Sigma moves the value by at most delta sum_ab |M_ab| |Sigma_ab|, and errors of the kernel values touch Sigma0 only.  The
# acceptance band of tests/test_gpu_marginal_exact.py is therefore, with rho = expanded_form_magnitude(...),
#   |ll_dev - ll_ref| <= MARGINAL_TOL_C * eps * (sum |M| |Sigma| + rho sum |M| |Sigma0|)        (marginal_unit)
# -- no condition number in it (the gradient tests' eps cond1 scale is vacuous here: cond1 and |alpha|'|Sigma||alpha| both
# grow with tau2 n).  First order only holds while eps cond1(Sigma) is small: every checked draw has cond1(Sigma) <=
# MARGINAL_COND_MAX.  The constant: the fp64 LAPACK evaluation with the exponent in the scripts' expanded form (marginal_parts(
# ..., np.float64, expanded=True)), a correct fp64 implementation, reaches at most MARGINAL_LAPACK_MAX units over the whole
# case list of the device module (tests/test_oracle.py measures it on every run); C is 32 times that -- the device's own
# summation orders, a 2-ulp exp, a Cholesky backward error growing like sqrt(n) up to n = 520 -- rounded up to a power of two
# and capped at GRAD_TOL_C.  Nothing here was taken from a device run; measured afterwards on an MI355X, the device's largest
# ratio over all routes is 0.085 units, 2 % of C (DESIGN.md has the per-route table).
MARGINAL_COND_MAX = 4e9
MARGINAL_LAPACK_MAX = 0.108        # measured: 0.1077 at n = 5, d = 4, K = 2, (sigma2, tau2) = (1, 25); 100 draws, n = 2 ... 520
MARGINAL_TOL_C = 4.0               # 32 x 0.108 = 3.46, rounded up to a power of two
# relative accuracy tests/test_special.py requires of the host inverse-gamma quantile; the device instance of the same source
# gets the same allowance in the grid's node term
GRID_NODE_Q = 2e-13


# The max-entropy design criteria (ccgp_mixed_logdet_designs, ccgp_mixed_logdet_grad_designs) are held the same way, by
# tests/design_exact.py: |ld_dev - ld_ref| <= C_LD unit_ld, |g_dev - g_ref| <= C_G unit_g entry by entry, units first order in
# a relative error eps (1 + rho_ab) of every entry of R (no condition number).  The fp64 LAPACK evaluation with the exponent in
# the expanded form (design_exact.fp64_restatement) reaches at most these many units over that module's case list
# (tests/test_design_exact_host.py measures both on every run); C is 32 times the figure, rounded up to a power of two and
# capped at GRAD_TOL_C (design_exact.design_constants): C_LD = 8, C_G = 16.  Nothing here was taken from a device run.
DESIGN_LD_LAPACK_MAX = 0.245       # measured: 0.2443 at the one-point design n = 1, d = 1, K = 1 (`instances`, design 1)
DESIGN_GRAD_LAPACK_MAX = 0.296     # measured: 0.2951 at n = 64, d = 1, K = 1 (`instances`, design 0)


def marginal_parts(X, y, row, K, d, sigma2, tau2, dtype=np.longdouble, expanded=False, Rc=None):
    """The mode-1 counterpart of loglik_grad_parts in dtype (long double: the hand-written Cholesky of Sigma0 and the rank-one
    term in closed form; fp64: LAPACK on Sigma):
    dict(Sigma, Sigma0, Sinv, Rc (list), M, alpha, loglik, beta = 0).  Kernel values in the direct squared-difference form, or,
    with expanded (fp64 only), in the scripts' expanded form u_a + u_b - 2 sum_k theta_k x_ak x_bk (corr_matrix).
    grad_from_parts() works on the result as it stands (it reads M and Rc).  Raises LinAlgError when not positive definite.
    Rc: the K component matrices in dtype, as in loglik_grad_parts."""
    dtype = np.dtype(dtype).type
    X = np.asarray(X, dtype=np.float64)
    yv = np.asarray(y, dtype=dtype).reshape(-1)
    n = yv.shape[0]
    w, Th = unpack_params(row, K, d)
    s2 = dtype(sigma2)
    if Rc is not None:
        assert not expanded
    elif expanded:
        assert dtype == np.float64
        Rc = [corr_matrix(X, Th[c]) for c in range(K)]
    else:
        Rc = [component_corr(X, Th[c], dtype) for c in range(K)]
    Sigma0 = np.zeros((n, n), dtype=dtype)
    for c in range(K):
        Sigma0 += (s2 * dtype(w[c]) ** 2) * Rc[c]
    Sigma = Sigma0 + dtype(tau2)
    if dtype == np.float64:
        Sinv, logdet = _chol_inverse(Sigma, dtype)          # what the scripts and the device do: factorise Sigma itself
        alpha = Sinv @ yv
    else:
        # the rank-one term in closed form (Sherman-Morrison, matrix determinant lemma): only Sigma0 is factorised, so that
        # the reference does not lose cond1(Sigma) / cond1(Sigma0) ~ tau2 n / sigma2 of its own precision
        S0inv, logdet0 = _chol_inverse(Sigma0, dtype)
        t2 = dtype(tau2)
        u = S0inv.sum(axis=0)
        den = dtype(1) + t2 * u.sum()
        Sinv = S0inv - (t2 / den) * np.outer(u, u)
        logdet = logdet0 + np.log1p(t2 * u.sum())
        alpha = S0inv @ yv - (t2 * (u @ yv) / den) * u
    ll = -(dtype(n) * _log_2pi(dtype) + logdet + yv @ alpha) / dtype(2)
    M = (np.outer(alpha, alpha) - Sinv) / dtype(2)
    return dict(Sigma=Sigma, Sigma0=Sigma0, Sinv=Sinv, Rc=Rc, M=M, alpha=alpha, loglik=ll, beta=dtype(0))


def marginal_unit(parts, X, row, K, d, rho=None):
    """eps (sum_ab |M_ab| |Sigma_ab| + rho sum_ab |M_ab| |Sigma0_ab|): what one relative fp64 rounding of every entry of Sigma,
    and rho roundings of every kernel value's exponent, move the mode-1 log-likelihood by (first order).  rho: the relative
    error of a kernel value in units of eps where it is not the expanded exponent's (another family); default: that."""
    aM = np.abs(parts["M"])
    if rho is None:
        rho = expanded_form_magnitude(X, row, K, d)
    return float(np.finfo(np.float64).eps * ((aM * np.abs(parts["Sigma"])).sum() + rho * (aM * np.abs(parts["Sigma0"])).sum()))


def logmeanexp_exact(logs, take_log=True):
    """log(mean(exp(logs))) (likeli.hyperpars / choose.hyperpars, HX:574, HX:591) or, without take_log, the mean itself
    (ADV:595), in long double (its exponent range holds exp(-11000))."""
    require_extended_precision()
    v = np.asarray(logs, dtype=np.longdouble).reshape(-1)
    mx = v.max()
    lme = mx + np.log(np.exp(v - mx).sum() / np.longdouble(v.shape[0]))
    return lme if take_log else np.exp(lme)


# --------------------------------------------------------------------------- predict.post tables, extended precision
# The tables of predict.post (HX:655-673) in the factor's metric, as every device route computes them:
#   ww = r'R^-1 r,  z1w = 1'R^-1 r,  zyw = y'R^-1 r,  s11 = 1'R^-1 1,  beta = 1'R^-1 y / s11,
#   mean = beta + (zyw - beta z1w),  var = sigma2 (1 - ww + (1 - z1w)^2 / s11),
# from the pieces of the gradient reference above (direct squared differences, the hand-written Cholesky in long double).
# The acceptance bands of tests/test_gpu_predict_exact.py are predict_bands(); why this C is in that module's docstring.
PREDICT_TOL_C = 128.0


def cross_corr(Xtest, X, theta_c, dtype=np.float64):
    """m x n correlations exp(-sum_k theta_ck (x_tk - x_ak)^2) between test sites and the design, direct form, in dtype."""
    X = np.asarray(X, dtype=np.float64)
    Xtest = np.asarray(Xtest, dtype=np.float64)
    acc = np.zeros((Xtest.shape[0], X.shape[0]), dtype=dtype)
    for k in range(X.shape[1]):
        acc += dtype(theta_c[k]) * (np.asarray(Xtest[:, k], dtype=dtype)[:, None] - np.asarray(X[:, k], dtype=dtype)[None, :]) ** 2
    return np.exp(-acc)


def predict_factor(X, y, row, K, d, dtype=np.longdouble, Rc=None):
    """What a draw's tables share between test sites, in dtype: dict(R, L, Rinv, o = R^-1 1, s11 = 1'o, beta, g = R^-1 (y -
    beta 1), Rinv_y) of the normalised mixed matrix R = sum_c w_c^2 R_c / sum_c w_c^2 (HX:408-415).  Rc: the K component
    matrices in dtype, as in loglik_grad_parts."""
    dtype = np.dtype(dtype).type
    X = np.asarray(X, dtype=np.float64)
    yv = np.asarray(y, dtype=dtype).reshape(-1)
    n = yv.shape[0]
    w, Th = unpack_params(row, K, d)
    w2 = np.asarray(w, dtype=dtype) ** 2
    R = np.zeros((n, n), dtype=dtype)
    for c in range(K):
        R += w2[c] * (component_corr(X, Th[c], dtype) if Rc is None else Rc[c])
    R = R / w2.sum()
    L = _chol_lower(R, dtype)
    Z = _lower_inverse(L, dtype)
    Rinv = Z.T @ Z
    o = Rinv.sum(axis=0)
    s11 = o.sum()
    Rinv_y = Rinv @ yv
    beta = (o @ yv) / s11
    g = Rinv @ (yv - beta)
    return dict(R=R, L=L, Rinv=Rinv, o=o, s11=s11, beta=beta, g=g, Rinv_y=Rinv_y, y=yv, w2=w2, Th=Th)


def predict_parts(X, y, row, K, d, sigma2, Xtest, dtype=np.longdouble, factor=None, rc=None, raw_r=False, rho=None, rho_t=None):
    """The tables of one draw at the rows of Xtest in dtype (default long double: no LAPACK, about 1e-19 relative):
    dict(mean[m], var[m], beta, s11, r[m, n], a[m, n] = (R^-1 r)', g, o, ww[m], z1w[m], zyw[m], W = |L| |L|', rho, rho_t[m]).
    factor: a predict_factor() of the same draw, to share it between site sets.
    Another family than the Gaussian passes rc, the K component cross blocks [m, n] in dtype (with its factor built on Rc),
    raw_r = True where its scripts leave r un-normalised (D1F:470-480), and rho, rho_t[m]: the relative error of an entry of R
    (against W = |L| |L|') and of r in units of eps, which predict_bands reads in place of the expanded exponent's size."""
    dtype = np.dtype(dtype).type
    f = factor if factor is not None else predict_factor(X, y, row, K, d, dtype)
    Xtest = np.atleast_2d(np.asarray(Xtest, dtype=np.float64))
    r = np.zeros((Xtest.shape[0], f["R"].shape[0]), dtype=dtype)
    for c in range(K):
        r += f["w2"][c] * (cross_corr(Xtest, X, f["Th"][c], dtype) if rc is None else rc[c])
    if not raw_r:
        r = r / f["w2"].sum()
    a = r @ f["Rinv"]
    ww = (a * r).sum(axis=1)
    z1w = r @ f["o"]
    zyw = r @ f["Rinv_y"]
    u = dtype(1) - z1w
    mean = f["beta"] + r @ f["g"]
    var = dtype(sigma2) * (dtype(1) - ww + u * u / f["s11"])
    aL = np.abs(np.asarray(f["L"], dtype=np.float64))
    Th = np.asarray(f["Th"], dtype=np.float64)
    return dict(mean=mean, var=var, beta=f["beta"], s11=f["s11"], r=r, a=a, g=f["g"], o=f["o"], ww=ww, z1w=z1w, zyw=zyw,
                W=aL @ aL.T, y=f["y"], rho=expanded_form_magnitude(X, row, K, d) if rho is None else rho,
                rho_t=2.0 * ((Xtest ** 2) @ Th.T).max(axis=1) if rho_t is None else rho_t)


def predict_bands(parts, sigma2, c=PREDICT_TOL_C):
    """First-order bands dict(mean[m], var[m], beta, s11) of a device table around predict_parts().  The device errs in the
    entries of R and r -- a relative eps (1 + rho) each, rho the size of the expanded exponent's terms (for an entry of r the
    larger of the design's and the site's own) -- and in the factorisation and the solves, a backward error |dR| <= eta W with
    W = |L| |L|' >= |R|.  For a bilinear form p'R^-1 q both give
        Q(p, q) = eta (|R^-1 p|' W |R^-1 q| + |R^-1 p|' |q| + |p|' |R^-1 q|),   eta = c eps (1 + rho),
    and from there
        var  : sigma2 (Q(r, r) + 2 |u| Q(1, r) / s11 + u^2 Q(1, 1) / s11^2 + eps (1 + ww + u^2 / s11)),  u = 1 - z1w
        beta : (Q(1, y - beta 1) + 2 |beta| Q(1, 1)) / s11 + eps sum_i |o_i y_i| / s11
        mean : Q(r, y - beta 1) + (1 + |z1w|) band_beta + eps (|beta| + |r|' |g|).
    beta: the device divides 1'R^-1 y by 1'R^-1 1, two solves with their own roundings, so the error of the second does not
    cancel against the first's: hence the |beta| Q(1, 1) beside the form in y - beta 1; the last term is the size of the sum
    before cancellation (loglik_beta_scales).  No condition number and no floor anywhere: on a training point R^-1 r is a unit
    vector and the variance band is a few eta sigma2."""
    eps = float(np.finfo(np.float64).eps)
    W, r, a, g, o, y, ww, z1w = (np.asarray(parts[k], dtype=np.float64) for k in ("W", "r", "a", "g", "o", "y", "ww", "z1w"))
    beta, s11 = float(parts["beta"]), float(parts["s11"])
    A, G, O, Rr = np.abs(a), np.abs(g), np.abs(o), np.abs(r)
    eta0 = c * eps * (1.0 + parts["rho"])
    eta = c * eps * (1.0 + np.maximum(parts["rho"], parts["rho_t"]))
    yc = np.abs(y - beta)
    one = np.ones_like(O)
    AW = A @ W
    q_ww = eta * ((AW * A).sum(axis=1) + 2.0 * (A * Rr).sum(axis=1))
    q_z1w = eta * (AW @ O + A @ one + Rr @ O)
    q_s11 = eta0 * (O @ W @ O + 2.0 * O.sum())
    q_ry = eta * (AW @ G + A @ yc + Rr @ G)
    q_1y = eta0 * (O @ W @ G + O @ yc + G.sum())
    u = 1.0 - z1w
    band_var = sigma2 * (q_ww + 2.0 * np.abs(u) * q_z1w / s11 + u * u * q_s11 / s11 ** 2 + eps * (1.0 + ww + u * u / s11))
    band_beta = (q_1y + 2.0 * abs(beta) * q_s11) / s11 + eps * float(O @ np.abs(y)) / s11
    band_mean = q_ry + (1.0 + np.abs(z1w)) * band_beta + eps * (abs(beta) + Rr @ G)
    return dict(mean=band_mean, var=band_var, beta=band_beta, s11=q_s11)


def _ldl_lower(A):
    """fp64 L' D L'^T of a symmetric positive definite A: (unit lower L', D), column by column as the device eliminates."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    Lp = np.eye(n)
    D = np.empty(n)
    for j in range(n):
        v = A[j:, j] - Lp[j:, :j] @ (D[:j] * Lp[j, :j])
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % j)
        D[j] = v[0]
        Lp[j + 1:, j] = v[1:] * (1.0 / D[j])
    return Lp, D


def predict_device_restatement(X, y, row, K, d, Xtest):
    """A plain fp64 restatement of the device's own formula, the yardstick PREDICT_TOL_C is measured against (and the subject
    of the planted mistakes of tests/test_oracle.py): expanded-form exponents (corr_matrix / corr_vec), the L' D L'^T
    factorisation, unit-lower forward substitutions of y, 1 and every r, then the D^-1-weighted dot products.  Returns
    dict(w[m, n] = L'^-1 r, rd = 1 / D, zy, z1, s11, beta); predict_device_finish() makes the tables of them."""
    X = np.asarray(X, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    Xtest = np.atleast_2d(np.asarray(Xtest, dtype=np.float64))
    wts, Th = unpack_params(row, K, d)
    Lp, D = _ldl_lower(mixed_corr_matrix_general(X, wts, Th))
    n, m = yv.shape[0], Xtest.shape[0]
    B = np.empty((n, 2 + m))
    B[:, 0], B[:, 1] = yv, 1.0
    for t in range(m):
        B[:, 2 + t] = mixed_corr_vec_general(Xtest[t], X, wts, Th)
    for i in range(1, n):
        B[i] -= Lp[i, :i] @ B[:i]
    rd = 1.0 / D
    zy, z1 = B[:, 0].copy(), B[:, 1].copy()
    s11 = float(np.sum(z1 * (z1 * rd)))
    beta = float(np.sum(zy * (z1 * rd))) / s11
    return dict(w=B[:, 2:].T.copy(), rd=rd, zy=zy, z1=z1, s11=s11, beta=beta)


def predict_device_finish(dev, sigma2):
    """(mean[m], var[m], ww, z1w, zyw) from predict_device_restatement(): the three dot products in the device's order (ww, z1w,
    zyw over w D^-1), then mean = beta + (zyw - beta z1w), var = sigma2 (1 - ww + u u / s11)."""
    wr = dev["w"] * dev["rd"][None, :]
    ww = (dev["w"] * wr).sum(axis=1)
    z1w = wr @ dev["z1"]
    zyw = wr @ dev["zy"]
    u = 1.0 - z1w
    mean = dev["beta"] + (zyw - dev["beta"] * z1w)
    var = sigma2 * (1.0 - ww + u * u / dev["s11"])
    return mean, var, ww, z1w, zyw
