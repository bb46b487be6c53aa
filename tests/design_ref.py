"""numpy fp64 reference of the max-entropy design criterion and its design gradient (Batch Sequential ME Design.R:856-948),
shared by the optimiser's CPU tests and its GPU tests.  Test infrastructure only: the package itself has no CPU path."""
import itertools
import os

import numpy as np

from conftest import DATA
from ccgp_amd.tables import read_table

BSQ_PRIOR = (0.5, 1.0, 4.0)   # p.prior, theta1.prior, theta2.prior (BSQ:981-983)


def initial_me_design():
    """`Initial ME Design.txt`, the stored first batch (BSQ:988), 14 x 2."""
    _, D = read_table(os.path.join(DATA, "bsq", "initial_me_design.txt"))
    return D


def params_row(p, theta1, theta2, d):
    return np.concatenate([[p, 1.0 - p], np.full(d, float(theta1)), np.full(d, float(theta2))])


def mixed_R_general(D, K, row):
    """R = sum_q w_q^2 R_q / sum_q w_q^2, R_q,ij = exp(-sum_k theta_qk (x_ik - x_jk)^2); row = (w_1..w_K, theta_11..)."""
    D = np.asarray(D, dtype=np.float64)
    n, d = D.shape
    w2 = np.asarray(row[:K], dtype=np.float64) ** 2
    th = np.asarray(row[K:], dtype=np.float64).reshape(K, d)
    diff2 = (D[:, None, :] - D[None, :, :]) ** 2
    Rq = np.exp(-np.einsum("ijk,qk->qij", diff2, th))
    return np.einsum("q,qij->ij", w2, Rq) / w2.sum(), Rq, w2 / w2.sum(), th


def logdet_grad_general(D, K, row, n_fixed=0, Rinv=None):
    """(log det R, d log det R / d x_ik for the rows i >= n_fixed) with np.linalg.inv (or a given R^-1)."""
    D = np.asarray(D, dtype=np.float64)
    R, Rq, wh, th = mixed_R_general(D, K, row)
    sign, ld = np.linalg.slogdet(R)
    A = np.linalg.inv(R) if Rinv is None else Rinv
    diff = D[:, None, :] - D[None, :, :]                       # x_ik - x_jk
    S = np.einsum("q,qk,qij->ijk", wh, th, Rq)                 # sum_q w^_q theta_qk R_q,ij
    G = -4.0 * np.einsum("ij,ijk,ijk->ik", A, diff, S)
    return (ld if sign > 0 else np.nan), G[n_fixed:]


def mixed_R(D, p, theta1, theta2):
    return mixed_R_general(D, 2, params_row(p, theta1, theta2, np.asarray(D).shape[1]))[0]


def numpy_evaluator(p, theta1, theta2, D_old=None, calls=None):
    """evaluate(X[k, n, d]) -> (-log det, -grad, status) for design.minimize_starts, one design at a time: the first
    batch criterion, or with D_old the Schur criterion log det R(D_old U X) - log det R(D_old)."""
    d_old = None if D_old is None else np.asarray(D_old, dtype=np.float64)
    ld_old = 0.0
    if d_old is not None:
        ld_old = np.linalg.slogdet(mixed_R(d_old, p, theta1, theta2))[1]

    def evaluate(X):
        if calls is not None:
            calls.append(np.array(X, copy=True))
        k = X.shape[0]
        f, g, st = np.empty(k), np.empty(X.shape), np.zeros(k, dtype=np.int32)
        for b in range(k):
            D = X[b] if d_old is None else np.vstack([d_old, X[b]])
            nf = 0 if d_old is None else d_old.shape[0]
            row = params_row(p, theta1, theta2, D.shape[1])
            try:
                np.linalg.cholesky(mixed_R_general(D, 2, row)[0])
                ld, gr = logdet_grad_general(D, 2, row, nf)
            except np.linalg.LinAlgError:   # a pivot <= 0: two coincident rows
                f[b], g[b], st[b] = np.nan, np.nan, 1
                continue
            f[b], g[b] = -(ld - ld_old), -gr
        return f, g, st
    return evaluate


def projected_gradient(x, g, lo=-1.0, hi=1.0):
    """L-BFGS-B's measure: max |P(x - g) - x|, P the projection on the box."""
    return float(np.max(np.abs(np.clip(x - g, lo, hi) - x)))


def square_symmetries():
    """The 8 symmetries of [-1, 1]^2 as functions of an n x 2 design."""
    out = []
    for swap, sx, sy in itertools.product((False, True), (1.0, -1.0), (1.0, -1.0)):
        out.append(lambda D, swap=swap, sx=sx, sy=sy: (D[:, ::-1] if swap else D) * np.array([sx, sy]))
    return out


def design_distance(A, B):
    """Smallest, over the 8 symmetries of the square and the row orders (Hungarian matching), of the largest
    per-point coordinate difference between designs A and B."""
    from scipy.optimize import linear_sum_assignment
    best = np.inf
    for T in square_symmetries():
        TA = T(np.asarray(A, dtype=np.float64))
        C = np.max(np.abs(TA[:, None, :] - np.asarray(B)[None, :, :]), axis=2)
        r, c = linear_sum_assignment(C)
        best = min(best, float(C[r, c].max()))
    return best
