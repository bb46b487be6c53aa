"""numpy / device-pointer wrappers of the libccgp C ABI (include/ccgp.h).

Every function here is a 1:1 call into the shared library; nothing is computed in
Python.  Matrices cross the boundary column-major (R's layout): inputs are copied with
`np.asfortranarray`, outputs are allocated Fortran-ordered.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_double, c_int, c_size_t, c_void_p

import numpy as np

from ._lib import load_library

MEAN_PROFILE_BETA = 0
MEAN_ZERO_PLUS_TAU2 = 1
PRIOR_INVGAMMA, PRIOR_GV, PRIOR_ISO, PRIOR_ANI = 0, 1, 2, 3
T_COV, T_UPDATE, T_DIAG, T_TRSM, T_SOLVE, T_FUSED = range(6)
KERNEL_GAUSS, KERNEL_MATERN, KERNEL_MATERN_SPLINE = 0, 1, 2
OPT_FUSE_DIAG, OPT_TAIL_STRIPS, OPT_WIDE_OFFSETS, OPT_SMALL_GRID16 = 2, 3, 4, 5
OPT_SCHED, OPT_SCHED_POLICY, OPT_PREDICT_FACTOR, OPT_FUSED_SOLVE = 7, 8, 9, 10
OPT_FAMILY_FUSED = 11   # the 1-D families on the register-resident evaluator at n <= 32 (default 0: the blocked sweep)
OPT_FAMILY_FUSED_PREDICT = 12   # their prediction and leave-one-out on that evaluator (default 0; independent of option 11)
OPT_FAMILY_FUSED_GRAD = 13   # their analytic gradient and profiled mode on that evaluator (default 0; independent of 11 and 12)
VAR_ORDINARY, VAR_PLUGIN, VAR_UNBIASED = 0, 1, 2   # ccgp_krige_predict_batch's var_form
TIMING_NAMES = ("cov", "update", "diag", "trsm", "solve", "fused", "sweep")

_dp = POINTER(c_double)
_ip = POINTER(c_int)

# name -> (restype, argtypes); also the list tests check against include/ccgp.h
SIGNATURES = {
    "ccgp_create": (c_int, [c_int, POINTER(c_void_p)]),
    "ccgp_destroy": (c_int, [c_void_p]),
    "ccgp_last_error": (c_char_p, [c_void_p]),
    "ccgp_version": (c_char_p, []),
    "ccgp_set_stream": (c_int, [c_void_p, c_void_p]),
    "ccgp_set_kernel": (c_int, [c_void_p, c_int, c_double]),
    "ccgp_set_workspace_limit": (c_int, [c_void_p, c_size_t]),
    "ccgp_set_option": (c_int, [c_void_p, c_int, c_int]),
    "ccgp_reserve": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "ccgp_synchronize": (c_int, [c_void_p]),
    "ccgp_corr_matrix": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp]),
    "ccgp_corr_cross": (c_int, [c_void_p, _dp, c_int, _dp, c_int, c_int, _dp, _dp]),
    "ccgp_mixed_corr_matrix": (c_int, [c_void_p, _dp, c_int, c_int, c_int, _dp, _dp]),
    "ccgp_mixed_corr_cross": (c_int, [c_void_p, _dp, c_int, _dp, c_int, c_int, c_int, _dp, _dp]),
    "ccgp_family_corr_dtheta": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp]),
    "ccgp_beta_mle": (c_int, [c_void_p, _dp, _dp, c_int, _dp]),
    "ccgp_sigma2_mle": (c_int, [c_void_p, _dp, _dp, c_int, c_double, _dp]),
    "ccgp_loglik_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, c_double,
                                  c_int, c_double, _dp, _dp, _ip]),
    "ccgp_loglik_batch_dev": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
                                      c_int, c_double, c_int, c_double, c_void_p, c_void_p, c_void_p]),
    "ccgp_loglik_grad_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, c_double,
                                       _dp, _dp, _dp, _ip]),
    "ccgp_profile_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, _dp, _dp, _dp, _dp, _ip]),
    "ccgp_cgp_state_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, _ip, _dp, _dp, _dp, _dp, _ip]),
    "ccgp_cgp_predict": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, _dp, c_int, _dp, _dp, _ip]),
    "ccgp_logpost": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_double, c_int, _dp, _dp, _dp, _dp,
                             _dp, _dp, _ip]),
    "ccgp_logpost_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_double, c_int, _dp, c_int, _dp, _dp, _dp, _dp, _ip]),
    "ccgp_loglik_batch_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, _ip, c_int, c_int, c_double,
                                       _dp, _dp, _ip]),
    "ccgp_logpost_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, _ip, c_int, _dp, _dp, _dp, _dp,
                                  _ip]),
    "ccgp_profile_batch_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, c_int, _dp, _ip, c_int, _dp, _dp, _dp, _dp,
                                        _ip]),
    "ccgp_chain_terms": (c_int, [c_int, c_int, _dp, c_int, _dp, _dp, _dp, _dp]),
    "ccgp_chain_logpost_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, _ip, c_int, _dp, _dp, _dp,
                                        _dp, _ip]),
    "ccgp_metro_segments_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, c_int, _ip, _dp, _dp, _dp,
                                         c_int, _dp, _dp, _ip, _ip, c_int, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                         _ip, _ip]),
    "ccgp_fit_state_doubles": (c_int, [c_int]),
    "ccgp_fit_begin": (c_int, [_dp, c_int, _dp, _dp, _dp, c_int, c_double, c_double, c_int]),
    "ccgp_fit_feed": (c_int, [_dp, c_int, c_double, _dp, c_int]),
    "ccgp_profile_fit_eval_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, _ip, c_int, _dp, _dp, _dp, _dp, _dp,
                                           _ip]),
    "ccgp_profile_fit_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, c_int, _ip, _dp, _ip, _ip, _dp, _ip, c_int]),
    "ccgp_nm_state_doubles": (c_int, [c_int]),
    "ccgp_nm_begin": (c_int, [_dp, c_int, _dp, c_double, c_double, c_int]),
    "ccgp_nm_feed": (c_int, [_dp, c_int, c_double]),
    "ccgp_laplace_search_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, c_int, _ip, _dp, _ip, _ip,
                                         _dp, _ip, c_int]),
    "ccgp_cgp_state_batch_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, _ip, c_int, _ip, _dp, _dp, _dp, _dp,
                                          _ip]),
    "ccgp_predict_batch_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, _ip, c_int, _dp, c_int, _dp, _dp,
                                        _dp, _ip]),
    "ccgp_krige_predict_batch_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, c_int, _dp, _ip, c_int, _dp, c_int, _dp,
                                              c_int, _dp, _dp, _dp, _dp, _ip]),
    "ccgp_predict_summary_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, _dp, c_int, c_int, _dp, _ip, c_int, _dp, c_int, _dp,
                                          c_int, _dp, _dp, _dp, _ip]),
    "ccgp_cgp_predict_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, _ip, c_int, _dp, c_int, _dp, _dp, _ip]),
    "ccgp_cgp_fit_rows": (c_int, [c_int]),
    "ccgp_cgp_fit_eval_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, _dp, _dp, c_double, _ip, c_int, _dp, _dp,
                                       _ip]),
    "ccgp_cgp_fit_sets": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, c_int, _ip, _dp, c_double, _ip, c_int, _ip, _dp, _ip,
                                  c_int]),
    "ccgp_grid_marginal": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_double, _dp, c_int, c_int,
                                   c_double, c_int, c_double, _dp, _ip, _dp]),
    "ccgp_mixed_logdet_designs": (c_int, [c_void_p, _dp, c_int, c_int, c_int, c_int, _dp, _dp, _ip]),
    "ccgp_mixed_logdet_grad_designs": (c_int, [c_void_p, _dp, c_int, c_int, c_int, c_int, _dp, c_int, _dp, _dp, _ip]),
    "ccgp_design_fit_eval": (c_int, [c_void_p, _dp, c_int, c_int, c_int, c_int, _dp, c_double, _dp, c_int, _dp, _dp, _ip]),
    "ccgp_design_fit": (c_int, [c_void_p, _dp, c_int, c_int, c_int, c_int, _dp, c_double, c_int, _dp, _ip, _ip, _dp, _ip, c_int]),
    "ccgp_halton_base2": (c_int, [c_int, _dp]),
    "ccgp_qigamma": (c_int, [_dp, c_int, c_double, c_double, _dp]),
    "ccgp_predict_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, _dp, c_int,
                                   c_double, _dp, _dp, _dp, _ip]),
    "ccgp_krige_predict_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, _dp, c_int, _dp, c_int,
                                         _dp, _dp, _dp, _dp, _ip]),
    "ccgp_loo_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, _dp, c_int, _dp, _dp, _dp, _dp, _ip]),
    "ccgp_loo_summary": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, c_double, _dp, c_int, _dp, _dp,
                                 _ip]),
    "ccgp_predict_batch_dev": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
                                       c_int, c_void_p, c_int, c_double, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "ccgp_predict_summary": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, _dp, c_int, c_double,
                                     _dp, c_int, _dp, _dp, _dp, _ip]),
    "ccgp_predict_summary_dev": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                         c_int, c_double, _dp, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ccgp_summary_from_factorset": (c_int, [c_void_p, c_void_p, _dp, c_int, _dp, c_int, _dp, _dp]),
    "ccgp_factor_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, c_double, POINTER(c_void_p),
                                  _dp, _dp, _ip]),
    "ccgp_predict_from_factorset": (c_int, [c_void_p, c_void_p, _dp, c_int, _dp, _dp]),
    "ccgp_factorset_bytes": (c_size_t, [c_void_p]),
    "ccgp_factorset_free": (c_int, [c_void_p, c_void_p]),
    "ccgp_factors": (c_int, [c_void_p, _dp, c_double, _dp, c_int, _dp]),
    "ccgp_predict_from_factors": (c_int, [c_void_p, _dp, c_int, c_int, c_double, _dp, _dp, c_double,
                                          _dp, c_double, _dp, _dp]),
    "ccgp_predict_post": (c_int, [c_void_p, _dp, c_int, _dp, c_int, c_int, c_int, _dp, c_double, _dp, _dp, c_double,
                                  _dp, c_double, _dp, _dp]),
    "ccgp_multi_create": (c_int, [c_int, _ip, POINTER(c_void_p)]),
    "ccgp_multi_destroy": (c_int, [c_void_p]),
    "ccgp_multi_count": (c_int, [c_void_p]),
    "ccgp_multi_handle": (c_void_p, [c_void_p, c_int]),
    "ccgp_multi_last_error": (c_char_p, [c_void_p]),
    "ccgp_multi_set_kernel": (c_int, [c_void_p, c_int, c_double]),
    "ccgp_multi_loglik_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, c_double,
                                        c_int, c_double, _dp, _dp, _ip]),
    "ccgp_multi_grid_marginal": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_double, _dp, c_int, c_int,
                                         c_double, c_int, c_double, _dp, _ip, _dp]),
    "ccgp_multi_predict_batch": (c_int, [c_void_p, _dp, c_int, c_int, _dp, c_int, _dp, c_int, _dp, c_int,
                                         c_double, _dp, _dp, _dp, _ip]),
    "ccgp_enable_timing": (c_int, [c_void_p, c_int]),
    "ccgp_get_timing": (c_int, [c_void_p, c_int, _dp, _ip]),
    "ccgp_last_sched_profile": (c_int, [c_void_p, c_void_p, c_int, _ip]),
    "ccgp_workspace_bytes": (c_int, [c_void_p, POINTER(c_size_t), POINTER(c_size_t)]),
    "ccgp_debug_fill_scratch": (c_int, [c_void_p, c_int]),
}

_bound = None


def lib():
    global _bound
    if _bound is None:
        L = load_library()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return _bound


class CcgpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libccgp error %d: %s" % (code, msg))
        self.code = code


def _f(a, shape=None):
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
    return a


def _p(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _ipt(a):
    return a.ctypes.data_as(_ip) if a is not None else None


# what the single-set batch wrappers and their sets forms share
def _check_columns(P, want, formula):
    if P != want:
        raise ValueError("params must have %s = %d columns" % (formula, want))


def _skip_rows(skip, B):
    """skip as int32[B], or None."""
    if skip is None:
        return None
    sk = np.ascontiguousarray(np.ravel(skip), dtype=np.int32)
    if sk.shape[0] != B:
        raise ValueError("skip must have one entry per row of params")
    return sk


def _outputs(B, count):
    """`count` double arrays of B entries and, last, the B status words."""
    return [np.empty(B) for _ in range(count)] + [np.zeros(B, dtype=np.int32)]


def halton_base2(N):
    out = np.empty(int(N), dtype=np.float64)
    rc = lib().ccgp_halton_base2(int(N), _p(out))
    if rc:
        raise CcgpError(rc, "ccgp_halton_base2")
    return out


def qigamma(p, alpha, beta):
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(p, dtype=np.float64)))
    out = np.empty_like(p)
    rc = lib().ccgp_qigamma(_p(p), p.size, float(alpha), float(beta), _p(out))
    if rc:
        raise CcgpError(rc, "ccgp_qigamma")
    return out


def chain_terms(prior_id, d, theta_t, prior_pars=None):
    """ccgp_chain_terms: the parameter rows [B, 2 + 2 d], log-Jacobians and log-priors of the transformed vectors theta_t
    [B, q] by the portable arithmetic the chain kernel runs (csrc/chain_terms.h) -> (rows, ljac, lprior).  No device."""
    theta_t = _f(np.atleast_2d(theta_t))
    B = theta_t.shape[0]
    pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
    rows = np.empty((B, 2 + 2 * int(d)), order="F")
    lj, lp = np.empty(B), np.empty(B)
    rc = lib().ccgp_chain_terms(int(prior_id), int(d), _p(theta_t), B, _p(pp), _p(rows), _p(lj), _p(lp))
    if rc:
        raise CcgpError(rc, "ccgp_chain_terms")
    return rows, lj, lp


# the codes of a start's state (csrc/fit_logic.h) and where its words lie
FIT_RUNNING, FIT_CONV_REDUCTION, FIT_CONV_PROJ_GRAD, FIT_MAXIT, FIT_LINE_SEARCH, FIT_NOT_EVALUABLE = range(6)
FIT_CODE, FIT_F, FIT_ITERATIONS, FIT_EVALS, FIT_HEADER = 1, 2, 5, 12, 16
FIT_MAX_EVALS = 4096


def fit_state_doubles(d):
    """ccgp_fit_state_doubles: the doubles of one start's state, 16 + 16 d."""
    W = lib().ccgp_fit_state_doubles(int(d))
    if W < 0:
        raise CcgpError(W, "ccgp_fit_state_doubles")
    return W


def fit_begin(x0, lower, upper, maxit=100, factr=1e7, pgtol=0.0, max_backtracks=30):
    """ccgp_fit_begin: the state of a start at x0 [d] under the box [lower, upper] (scalars or [d]) with design.minimize_starts'
    defaults -> float64[W].  state[FIT_HEADER + 3 d:][:d] is the point to evaluate first.  No device."""
    x0 = np.ascontiguousarray(np.ravel(np.asarray(x0, dtype=np.float64)))
    d = x0.shape[0]
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), (d,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (d,)))
    state = np.empty(fit_state_doubles(d))
    rc = lib().ccgp_fit_begin(_p(state), d, _p(x0), _p(lo), _p(hi), int(maxit), float(factr), float(pgtol), int(max_backtracks))
    if rc:
        raise CcgpError(rc, "ccgp_fit_begin")
    return state


def fit_feed(state, f, g, ok=True):
    """ccgp_fit_feed: hand the state (float64[W], C-contiguous, changed in place) the value and gradient at its trial point
    -> the new code.  No device."""
    if not (isinstance(state, np.ndarray) and state.dtype == np.float64 and state.flags.c_contiguous and state.ndim == 1):
        raise ValueError("state must be a contiguous float64 vector")
    d = (state.shape[0] - FIT_HEADER) // 16
    g = np.ascontiguousarray(np.ravel(np.asarray(g, dtype=np.float64)))
    if g.shape[0] != d or fit_state_doubles(d) != state.shape[0]:
        raise ValueError("state and gradient disagree about d")
    rc = lib().ccgp_fit_feed(_p(state), d, float(f), _p(g), int(bool(ok)))
    if rc < 0:
        raise CcgpError(rc, "ccgp_fit_feed")
    return rc


def cgp_fit_rows(d):
    """ccgp_cgp_fit_rows: the parameter rows of one evaluation of the CGP refinement, 1 + 2 (d + 3)."""
    R = lib().ccgp_cgp_fit_rows(int(d))
    if R < 0:
        raise CcgpError(R, "ccgp_cgp_fit_rows")
    return R


def fit_trial(state):
    """The point a running start wants evaluated next: a copy of the `trial` words of its state (or of each row of [A, W])."""
    state = np.asarray(state)
    d = (state.shape[-1] - FIT_HEADER) // 16
    return np.array(state[..., FIT_HEADER + 3 * d:FIT_HEADER + 4 * d])


def fit_x(state):
    """The last accepted iterate of a start: a copy of the `x` words of its state (or of each row of [A, W])."""
    state = np.asarray(state)
    d = (state.shape[-1] - FIT_HEADER) // 16
    return np.array(state[..., FIT_HEADER:FIT_HEADER + d])


# the codes of a Nelder-Mead search's state (csrc/nm_logic.h) and where its words lie
NM_RUNNING, NM_CONVERGED, NM_MAXITER = range(3)
NM_Q, NM_CODE, NM_PHASE, NM_ITERATIONS, NM_CHARGED, NM_FED, NM_HEADER = 0, 1, 2, 4, 5, 6, 16
NM_COUNTERS = dict(expansion_taken=10, expansion_refused=11, reflection=12, outside_contraction=13, inside_contraction=14,
                   shrink=15)
NM_MAX_EVALS = 4096


def nm_state_doubles(q):
    """ccgp_nm_state_doubles: the doubles of one search's state, q^2 + 5 q + 18."""
    W = lib().ccgp_nm_state_doubles(int(q))
    if W < 0:
        raise CcgpError(W, "ccgp_nm_state_doubles")
    return W


def _nm_q(state):
    q = int(np.asarray(state)[..., NM_Q].flat[0])
    if q < 1 or q > 8 or np.asarray(state).shape[-1] != q * q + 5 * q + 18:
        raise ValueError("not the state of a search: %d words for q = %d" % (np.asarray(state).shape[-1], q))
    return q


def nm_begin(x0, xatol=1e-6, fatol=1e-9, maxiter=2000):
    """ccgp_nm_begin: the state of fit.laplace_sets' Nelder-Mead search from x0 [q] -> float64[W]; nm_trial(state) is the
    point to evaluate first.  No device."""
    x0 = np.ascontiguousarray(np.ravel(np.asarray(x0, dtype=np.float64)))
    q = x0.shape[0]
    state = np.empty(nm_state_doubles(q))
    rc = lib().ccgp_nm_begin(_p(state), q, _p(x0), float(xatol), float(fatol), int(maxiter))
    if rc:
        raise CcgpError(rc, "ccgp_nm_begin")
    return state


def nm_feed(state, val):
    """ccgp_nm_feed: hand the state (float64[W], C-contiguous, changed in place) the log-posterior at its trial point -> the
    new code.  No device."""
    if not (isinstance(state, np.ndarray) and state.dtype == np.float64 and state.flags.c_contiguous and state.ndim == 1):
        raise ValueError("state must be a contiguous float64 vector")
    rc = lib().ccgp_nm_feed(_p(state), _nm_q(state), float(val))
    if rc < 0:
        raise CcgpError(rc, "ccgp_nm_feed")
    return rc


def nm_trial(state):
    """The point a running search wants evaluated next: a copy of the `trial` words of its state (or of each row of [A, W])."""
    state = np.asarray(state)
    return np.array(state[..., state.shape[-1] - _nm_q(state):])


def nm_simplex(state):
    """(simplex [q + 1, q], values [q + 1]) of a search's state, best vertex first once sorted; the values are the
    log-posterior's (the state keeps them negated), -1e300 where it was not finite."""
    state = np.asarray(state)
    q = _nm_q(state)
    sim = np.array(state[NM_HEADER:NM_HEADER + (q + 1) * q]).reshape(q + 1, q)
    return sim, -np.array(state[NM_HEADER + (q + 1) * q:NM_HEADER + (q + 1) * q + q + 1])


SUMMARY_MAX_PROBS = 8


def _probs(probs):
    return np.ascontiguousarray(np.ravel(np.asarray(probs, dtype=np.float64)))


def _summary_dict(out, n_failed, beta=None, status=None):
    """The m x (4 + n_probs) block of ccgp_predict_summary as named arrays."""
    return dict(y_hat=out[:, 0], pred_var=out[:, 1], quant=out[:, 2], cdf_at=out[:, 3], quantiles=out[:, 4:],
                beta=beta, status=status, n_failed=n_failed)


class FactorSet:
    """S Cholesky factors kept in HBM (ccgp_factor_batch); predict(Xtest) -> (mean[S, m], var[S, m])."""

    def __init__(self, handle, ptr, S, loglik, beta, status):
        self._handle, self._fs, self.S = handle, ptr, S
        self.loglik, self.beta, self.status = loglik, beta, status

    @property
    def nbytes(self):
        return int(lib().ccgp_factorset_bytes(self._fs))

    def predict(self, Xtest):
        Xtest = _f(np.atleast_2d(Xtest))
        m = Xtest.shape[0]
        mean = np.empty((self.S, m), dtype=np.float64, order="F")
        var = np.empty((self.S, m), dtype=np.float64, order="F")
        self._handle._chk(lib().ccgp_predict_from_factorset(self._handle._h, self._fs, _p(Xtest), m, _p(mean), _p(var)))
        return mean, var

    def summary(self, Xtest, probs, y_at=None):
        """prediction()'s per-site summaries (HX:686-703) from the kept factors: the dict of Handle.predict_summary
        (beta / status are the set's own)."""
        Xtest = _f(np.atleast_2d(Xtest))
        m = Xtest.shape[0]
        probs = _probs(probs)
        y_at = _f(np.ravel(y_at), (m,)) if y_at is not None else None
        out = np.empty((m, 4 + probs.size), dtype=np.float64, order="F")
        bad = self._handle._chk(lib().ccgp_summary_from_factorset(self._handle._h, self._fs, _p(Xtest), m, _p(probs),
                                                                  probs.size, _p(y_at), _p(out)))
        return _summary_dict(out, bad, self.beta, self.status)

    def free(self):
        if self._fs:
            lib().ccgp_factorset_free(self._handle._h, self._fs)
            self._fs = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultiHandle:
    """Several devices behind one host process (ccgp_multi_*): the batched calls are cut into contiguous shards,
    one per listed device, and gathered in host memory.  devices: a count (0 .. k-1) or an explicit list; a device
    may be listed more than once (the shards then share it)."""

    def __init__(self, devices):
        devs = list(range(devices)) if isinstance(devices, int) else [int(v) for v in devices]
        arr = (c_int * len(devs))(*devs)
        self._m = c_void_p()
        rc = lib().ccgp_multi_create(len(devs), arr, ctypes.byref(self._m))
        if rc:
            self._m = None
            raise CcgpError(rc, "ccgp_multi_create(%s) failed -- is every device visible?" % devs)
        self.devices = devs

    def close(self):
        if getattr(self, "_m", None):
            lib().ccgp_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise CcgpError(rc, lib().ccgp_multi_last_error(self._m).decode())
        return rc

    def count(self):
        return lib().ccgp_multi_count(self._m)

    def set_kernel(self, family=0, nu=0.0):
        self._chk(lib().ccgp_multi_set_kernel(self._m, int(family), float(nu)))

    def set_workspace_limit(self, nbytes):
        for i in range(self.count()):
            rc = lib().ccgp_set_workspace_limit(c_void_p(lib().ccgp_multi_handle(self._m, i)), int(nbytes))
            if rc:
                raise CcgpError(rc, "ccgp_set_workspace_limit")

    def debug_fill_scratch(self, byte):
        """ccgp_debug_fill_scratch on every shard's handle; returns the shards' return values."""
        return [lib().ccgp_debug_fill_scratch(c_void_p(lib().ccgp_multi_handle(self._m, i)), int(byte))
                for i in range(self.count())]

    def loglik_batch(self, X, y, K, params, sigma2, mean_mode=MEAN_PROFILE_BETA, tau2=0.0):
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        _check_columns(P, K + K * d, "K + K*d")
        ll, beta, st = _outputs(B, 2)
        self._chk(lib().ccgp_multi_loglik_batch(self._m, _p(X), n, d, _p(y), K, _p(params), B, float(sigma2),
                                                int(mean_mode), float(tau2), _p(ll), _p(beta), _ipt(st)))
        return ll, beta, st

    def grid_marginal(self, X, y, sigma2, hyper, N, tau, take_log, aniso_lambda=-1.0, want_logs=False):
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        hyper = _f(hyper)
        G = hyper.shape[0]
        out = np.empty(G)
        arg = c_int()
        logs = np.empty((G, N), dtype=np.float64) if want_logs else None
        self._chk(lib().ccgp_multi_grid_marginal(self._m, _p(X), n, d, _p(y), float(sigma2), _p(hyper), G, int(N),
                                                 float(tau), 1 if take_log else 0, float(aniso_lambda), _p(out),
                                                 ctypes.byref(arg), _p(logs)))
        return (out, arg.value, logs) if want_logs else (out, arg.value)

    def predict_batch(self, X, y, K, params, Xtest, sigma2):
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        S = params.shape[0]
        Xtest = _f(np.atleast_2d(Xtest))
        m = Xtest.shape[0]
        mean = np.empty((S, m), dtype=np.float64, order="F")
        var = np.empty((S, m), dtype=np.float64, order="F")
        beta = np.empty(S)
        st = np.zeros(S, dtype=np.int32)
        self._chk(lib().ccgp_multi_predict_batch(self._m, _p(X), n, d, _p(y), K, _p(params), S, _p(Xtest), m,
                                                 float(sigma2), _p(mean), _p(var), _p(beta), _ipt(st)))
        return mean, var, beta, st


class Handle:
    """One libccgp handle bound to one HIP device (one per process / per GPU)."""

    def __init__(self, device=0):
        self._h = c_void_p()
        rc = lib().ccgp_create(int(device), ctypes.byref(self._h))
        if rc:
            self._h = None
            raise CcgpError(rc, "ccgp_create(device=%d) failed -- is a HIP device visible?" % device)
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            lib().ccgp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise CcgpError(rc, lib().ccgp_last_error(self._h).decode())
        return rc

    # -- plumbing ----------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr):
        """Run the calls that follow on the caller's stream: pass `torch.cuda.Stream().cuda_stream`.  0 / None selects the
        handle's OWN non-blocking stream, not the default stream -- and torch's default stream may report
        `cuda_stream == 0`, so `torch.cuda.current_stream().cuda_stream` can silently mean the handle's own stream, which
        does not order with the work torch enqueued.  The switch itself orders nothing: with work in flight on the previous
        stream, order the two streams (an event, or synchronize()) first."""
        self._chk(lib().ccgp_set_stream(self._h, c_void_p(hip_stream_ptr or 0)))

    def set_kernel(self, family=0, nu=0.0):
        """Correlation family for the calls that follow: KERNEL_GAUSS (default) or KERNEL_MATERN with
        smoothness nu (the 1-D scripts, D1:348-351; d must then be 1)."""
        self._chk(lib().ccgp_set_kernel(self._h, int(family), float(nu)))

    def set_workspace_limit(self, nbytes):
        self._chk(lib().ccgp_set_workspace_limit(self._h, int(nbytes)))

    def set_option(self, option, value):
        """Measurement switches of include/ccgp.h (OPT_*)."""
        self._chk(lib().ccgp_set_option(self._h, int(option), int(value)))

    def reserve(self, n, d, K, B, m=0):
        """Size every buffer the *_dev calls of this shape need (with m > 0 the prediction's too, kept-factor scratch and
        second stream included): afterwards they only enqueue."""
        self._chk(lib().ccgp_reserve(self._h, n, d, K, B, m))

    def workspace_bytes(self):
        """(workspace, staging) bytes of device scratch the handle holds now; does not synchronise."""
        ws, st = c_size_t(), c_size_t()
        self._chk(lib().ccgp_workspace_bytes(self._h, ctypes.byref(ws), ctypes.byref(st)))
        return ws.value, st.value

    def debug_fill_scratch(self, byte):
        """ccgp_debug_fill_scratch: fill workspace, staging and pinned buffer with `byte` (0 .. 255) now and every buffer
        the handle allocates from now on; -1 turns the fill on allocation off.  Returns the C return value (0 = done)."""
        return self._chk(lib().ccgp_debug_fill_scratch(self._h, int(byte)))

    def synchronize(self):
        self._chk(lib().ccgp_synchronize(self._h))

    def enable_timing(self, on=True, only=None):
        """Bracket launch groups with HIP events on their stream.  only = names from TIMING_NAMES to
        restrict the events to (each timed launch costs two event records)."""
        mask = 1 if on else 0
        if on and only is not None:
            mask = 0
            for name in only:
                mask |= 1 << (1 + TIMING_NAMES.index(name))
        self._chk(lib().ccgp_enable_timing(self._h, mask))

    def get_timing(self):
        out = {}
        for i, name in enumerate(TIMING_NAMES):
            ms, cnt = c_double(), c_int()
            self._chk(lib().ccgp_get_timing(self._h, i, ctypes.byref(ms), ctypes.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def last_sched_profile(self):
        """Per-workgroup time account of the last scheduled sweep (OPT_SCHED_POLICY bit 2): array (workgroups, 8) --
        microseconds waiting for a task, in D / U / T tiles, applying arrivals; tasks run; XCD served; second-on-its-CU."""
        buf = np.zeros((1024, 8), dtype=np.uint64)
        nw = c_int()
        self._chk(lib().ccgp_last_sched_profile(self._h, buf.ctypes.data_as(c_void_p), 1024, ctypes.byref(nw)))
        out = buf[:nw.value].astype(np.float64)
        out[:, :5] *= 0.01
        return out

    def corr_matrix(self, X, theta):
        X = _f(X)
        n, d = X.shape
        theta = _f(np.broadcast_to(np.asarray(theta, dtype=np.float64), (d,)))
        out = np.empty((n, n), dtype=np.float64, order="F")
        self._chk(lib().ccgp_corr_matrix(self._h, _p(X), n, d, _p(theta), _p(out)))
        return out

    def corr_cross(self, Xnew, X, theta):
        X = _f(X)
        n, d = X.shape
        Xnew = _f(np.atleast_2d(Xnew))
        m = Xnew.shape[0]
        theta = _f(np.broadcast_to(np.asarray(theta, dtype=np.float64), (d,)))
        out = np.empty((m, n), dtype=np.float64, order="F")
        self._chk(lib().ccgp_corr_cross(self._h, _p(Xnew), m, _p(X), n, d, _p(theta), _p(out)))
        return out

    def mixed_corr_matrix(self, X, K, params_row):
        X = _f(X)
        n, d = X.shape
        row = _f(params_row, (K + K * d,))
        out = np.empty((n, n), dtype=np.float64, order="F")
        self._chk(lib().ccgp_mixed_corr_matrix(self._h, _p(X), n, d, K, _p(row), _p(out)))
        return out

    def mixed_corr_cross(self, Xnew, X, K, params_row):
        X = _f(X)
        n, d = X.shape
        Xnew = _f(np.atleast_2d(Xnew))
        m = Xnew.shape[0]
        row = _f(params_row, (K + K * d,))
        out = np.empty((m, n), dtype=np.float64, order="F")
        self._chk(lib().ccgp_mixed_corr_cross(self._h, _p(Xnew), m, _p(X), n, d, K, _p(row), _p(out)))
        return out

    def family_corr_dtheta(self, X, K, params_row, q):
        """ccgp_family_corr_dtheta: d R_q / d theta_q of component q (0-based) under the 1-D family in force, entry by
        entry -- the derivative the gradient under OPT_FAMILY_FUSED_GRAD sums.  X: n coordinates; params_row: the 2 K
        doubles (weights, thetas).  Returns the n x n table."""
        x = _f(np.ravel(X))
        n = x.size
        row = _f(params_row, (2 * K,))
        out = np.empty((n, n), dtype=np.float64, order="F")
        self._chk(lib().ccgp_family_corr_dtheta(self._h, _p(x), n, K, _p(row), int(q), _p(out)))
        return out

    # -- a6, a7, a10, a11 (explicit R.Inv forms) ---------------------------------------
    def beta_mle(self, R_inv, y):
        R_inv, y = _f(R_inv), _f(np.ravel(y))
        out = c_double()
        self._chk(lib().ccgp_beta_mle(self._h, _p(R_inv), _p(y), y.size, ctypes.byref(out)))
        return out.value

    def sigma2_mle(self, R_inv, y, beta):
        R_inv, y = _f(R_inv), _f(np.ravel(y))
        out = c_double()
        self._chk(lib().ccgp_sigma2_mle(self._h, _p(R_inv), _p(y), y.size, float(beta), ctypes.byref(out)))
        return out.value

    def factors(self, R_inv, beta, y):
        R_inv, y = _f(R_inv), _f(np.ravel(y))
        n = y.size
        out = np.empty(2 * n + 1, dtype=np.float64)
        self._chk(lib().ccgp_factors(self._h, _p(R_inv), float(beta), _p(y), n, _p(out)))
        return out

    def predict_from_factors(self, r, beta, mean_factor, var_factor1, var_factor2, R_inv, sigma2):
        r = _f(np.atleast_2d(r))
        m, n = r.shape
        mf, v1, R_inv = _f(mean_factor, (n,)), _f(var_factor1, (n,)), _f(R_inv, (n, n))
        mean, var = np.empty(m), np.empty(m)
        self._chk(lib().ccgp_predict_from_factors(self._h, _p(r), m, n, float(beta), _p(mf), _p(v1),
                                                  float(var_factor2), _p(R_inv), float(sigma2),
                                                  _p(mean), _p(var)))
        return mean, var

    def predict_post(self, Xnew, X, K, params_row, beta, mean_factor, var_factor1, var_factor2, R_inv, sigma2):
        """Literal predict.post (HX:655-673) in one device round trip: Mixed.corr.vec for the rows of Xnew, then the
        quadratic forms with the caller's cached terms.  Returns (mean[m], var[m])."""
        X = _f(X)
        n, d = X.shape
        Xnew = _f(np.atleast_2d(Xnew))
        m = Xnew.shape[0]
        row = _f(params_row, (K + K * d,))
        mf, v1, R_inv = _f(mean_factor, (n,)), _f(var_factor1, (n,)), _f(R_inv, (n, n))
        mean, var = np.empty(m), np.empty(m)
        self._chk(lib().ccgp_predict_post(self._h, _p(Xnew), m, _p(X), n, d, K, _p(row), float(beta), _p(mf), _p(v1),
                                          float(var_factor2), _p(R_inv), float(sigma2), _p(mean), _p(var)))
        return mean, var

    # -- a8, a9, a12 --------------------------------------------------------------------
    def loglik_batch(self, X, y, K, params, sigma2, mean_mode=MEAN_PROFILE_BETA, tau2=0.0):
        """params: [B, K + K*d].  Returns (loglik[B], beta[B], status[B])."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        _check_columns(P, K + K * d, "K + K*d")
        ll, beta, st = _outputs(B, 2)
        self._chk(lib().ccgp_loglik_batch(self._h, _p(X), n, d, _p(y), K, _p(params), B, float(sigma2),
                                          int(mean_mode), float(tau2), _p(ll), _p(beta), _ipt(st)))
        return ll, beta, st

    def loglik_grad_batch(self, X, y, K, params, sigma2):
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        ll, beta = np.empty(B), np.empty(B)
        grad = np.empty((B, P), dtype=np.float64, order="F")
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_loglik_grad_batch(self._h, _p(X), n, d, _p(y), K, _p(params), B,
                                               float(sigma2), _p(ll), _p(beta), _p(grad), _ipt(st)))
        return ll, beta, grad, st

    def profile_batch(self, X, y, K, params, grad=False):
        """ccgp_profile_batch: the likelihood with sigma2 concentrated out (ordinary kriging), one factorisation per
        draw.  params: [B, K + K*d].  Returns (loglik[B], sigma2[B], beta[B], grad[B, P] or None, status[B]); grad is
        d loglik / d params at each draw's own (beta, sigma2) and needs the Gaussian family, or a 1-D family at n <= 32
        with OPT_FAMILY_FUSED_GRAD on."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        _check_columns(P, K + K * d, "K + K*d")
        ll, s2, beta, st = _outputs(B, 3)
        g = np.empty((B, P), dtype=np.float64, order="F") if grad else None
        self._chk(lib().ccgp_profile_batch(self._h, _p(X), n, d, _p(y), K, _p(params), B, _p(ll), _p(s2), _p(beta),
                                           _p(g), _ipt(st)))
        return ll, s2, beta, g, st

    def cgp_state_batch(self, X, y, params, skip=None):
        """ccgp_cgp_state_batch: the CGP state (var.MLE.DK, GV:102-133) at the B rows (lambda, theta[d], alpha[d], bw) of
        params in one call; skip[B] (-1: none) holds a row out and predicts it (the jackknife, GV:168-197).  Returns
        (val[B], beta[B], tau2[B], loo[B] or None without skip, status[B]); NaN where status != 0."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        _check_columns(P, 2 * d + 2, "2 d + 2")
        sk = _skip_rows(skip, B)
        val, beta, tau2, st = _outputs(B, 3)
        loo = np.empty(B) if sk is not None else None
        self._chk(lib().ccgp_cgp_state_batch(self._h, _p(X), n, d, _p(y), _p(params), B, _ipt(sk), _p(val), _p(beta),
                                             _p(tau2), _p(loo), _ipt(st)))
        return val, beta, tau2, loo, st

    def cgp_predict(self, X, y, row, Xtest):
        """ccgp_cgp_predict: the final CGP state (GV:200-221) at ONE parameter row and predict.CGP(PI = TRUE) (GV:287-307)
        at the m rows of Xtest (m may be 0).  Returns (out[m, 6]: Yp gp lp v Y_low Y_up, dict(s, res2, temp, sf, beta, tau2)
        or None when the state failed, status)."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        row = _f(np.ravel(row), (2 * d + 2,))
        Xt = _f(np.asarray(Xtest, dtype=np.float64).reshape(-1, d))
        m = Xt.shape[0]
        out = np.empty((m, 6), dtype=np.float64, order="F")
        state = np.empty(3 * n + 3)
        st = c_int()
        self._chk(lib().ccgp_cgp_predict(self._h, _p(X), n, d, _p(y), _p(row), _p(Xt) if m else None, m,
                                         _p(out) if m else None, _p(state), ctypes.byref(st)))
        if st.value:
            return out, None, st.value
        keep = dict(s=state[:n].copy(), res2=state[n:2 * n].copy(), temp=state[2 * n:3 * n].copy(), sf=float(state[3 * n]),
                    beta=float(state[3 * n + 1]), tau2=float(state[3 * n + 2]))
        return out, keep, 0

    def logpost(self, X, y, sigma2, prior_id, theta_t, prior_pars=None, want_Rinv=True):
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        theta_t = _f(np.ravel(theta_t))
        pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
        val, beta, ll = c_double(), c_double(), c_double()
        st = c_int()
        Rinv = np.empty((n, n), dtype=np.float64, order="F") if want_Rinv else None
        self._chk(lib().ccgp_logpost(self._h, _p(X), n, d, _p(y), float(sigma2), int(prior_id),
                                     _p(theta_t), _p(pp), ctypes.byref(val), ctypes.byref(beta),
                                     ctypes.byref(ll), _p(Rinv), ctypes.byref(st)))
        return dict(val=val.value, beta=beta.value, loglik=ll.value, R_inv=Rinv, status=st.value)

    def logpost_batch(self, X, y, sigma2, prior_id, theta_t, prior_pars=None):
        """ccgp_logpost_batch: logpost of B transformed parameter vectors (rows of theta_t) in one call ->
        (val, beta, loglik, status), each value as Handle.logpost returns it, bit for bit."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        theta_t = _f(np.atleast_2d(theta_t))
        B = theta_t.shape[0]
        pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
        val, beta, ll, st = _outputs(B, 3)
        self._chk(lib().ccgp_logpost_batch(self._h, _p(X), n, d, _p(y), float(sigma2), int(prior_id), _p(theta_t), B,
                                           _p(pp), _p(val), _p(beta), _p(ll), _ipt(st)))
        return val, beta, ll, st

    @staticmethod
    def _sets(Xs, ys, sigma2s, set_of, B):
        """The C training sets of one shape as the sets calls take them: designs [C, n, d] -> C column-major blocks,
        responses [C, n], variances [C] (None where the call takes none), and the rows' set indices as int32[B]."""
        Xs = np.asarray(Xs, dtype=np.float64)
        if Xs.ndim != 3:
            raise ValueError("Xs must be [C, n, d]: the sets of one call have one shape")
        C, n, d = Xs.shape
        blocks = np.ascontiguousarray(np.transpose(Xs, (0, 2, 1)))
        ys = np.ascontiguousarray(np.asarray(ys, dtype=np.float64).reshape(C, n))
        s2 = None if sigma2s is None else np.ascontiguousarray(np.asarray(sigma2s, dtype=np.float64).reshape(C))
        idx = np.ascontiguousarray(np.asarray(set_of).reshape(B).astype(np.int32))
        return blocks, ys, s2, idx, C, n, d

    def loglik_batch_sets(self, Xs, ys, sigma2s, K, params, set_of, mean_mode=MEAN_PROFILE_BETA, tau2=0.0):
        """ccgp_loglik_batch_sets: row b of params [B, K + K*d] on training set set_of[b] of the C sets Xs [C, n, d],
        ys [C, n], sigma2s [C] in one call.  Returns (loglik[B], beta[B], status[B]), each row with the bits loglik_batch
        gives it on its set alone."""
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        Xb, yb, s2, idx, C, n, d = self._sets(Xs, ys, sigma2s, set_of, B)
        _check_columns(P, K + K * d, "K + K*d")
        ll, beta, st = _outputs(B, 2)
        self._chk(lib().ccgp_loglik_batch_sets(self._h, _p(Xb), n, d, _p(yb), _p(s2), C, K, _p(params), _ipt(idx), B,
                                               int(mean_mode), float(tau2), _p(ll), _p(beta), _ipt(st)))
        return ll, beta, st

    def logpost_sets(self, Xs, ys, sigma2s, prior_id, theta_t, set_of, prior_pars=None):
        """ccgp_logpost_sets: logpost of row b of theta_t on training set set_of[b] -> (val, beta, loglik, status), each
        value as logpost_batch returns it on that set alone, bit for bit."""
        theta_t = _f(np.atleast_2d(theta_t))
        B = theta_t.shape[0]
        Xb, yb, s2, idx, C, n, d = self._sets(Xs, ys, sigma2s, set_of, B)
        pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
        val, beta, ll, st = _outputs(B, 3)
        self._chk(lib().ccgp_logpost_sets(self._h, _p(Xb), n, d, _p(yb), _p(s2), C, int(prior_id), _p(theta_t), _ipt(idx), B,
                                          _p(pp), _p(val), _p(beta), _p(ll), _ipt(st)))
        return val, beta, ll, st

    def chain_logpost_sets(self, Xs, ys, sigma2s, prior_id, theta_t, set_of, prior_pars=None):
        """ccgp_chain_logpost_sets: logpost_sets with the portable Jacobian / prior arithmetic of the device chains -- the
        host twin of metro_segments_sets' evaluation -> (val, beta, loglik, status)."""
        theta_t = _f(np.atleast_2d(theta_t))
        B = theta_t.shape[0]
        Xb, yb, s2, idx, C, n, d = self._sets(Xs, ys, sigma2s, set_of, B)
        pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
        val, beta, ll, st = _outputs(B, 3)
        self._chk(lib().ccgp_chain_logpost_sets(self._h, _p(Xb), n, d, _p(yb), _p(s2), C, int(prior_id), _p(theta_t),
                                                _ipt(idx), B, _p(pp), _p(val), _p(beta), _p(ll), _ipt(st)))
        return val, beta, ll, st

    def metro_segments_sets(self, Xs, ys, sigma2s, prior_id, set_of, theta0, l0, steps, logu, n_prop, stop_acc,
                            prior_pars=None, beta0=None, trace=False):
        """ccgp_metro_segments_sets: A chains, chain a on training set set_of[a], walked on the device through the proposals
        theta + steps[a, t] with log-uniforms logu[a, t] (steps [A, T, q], logu [A, T]) from the state (theta0 [A, q], l0 [A],
        beta0 [A] or None) until chain a has accepted stop_acc[a] draws or used n_prop[a] proposals.  Returns dict(used[A],
        accepted[A], draws [A, M, q], draw_val [A, M], draw_beta [A, M] with M = max(stop_acc, 1) -- NaN beyond a chain's
        accepted count --, theta [A, q], l [A], beta [A], failed: proposals whose factorisation failed, and with trace=True
        trace_val, trace_beta, trace_status, trace_accept [A, T])."""
        theta0 = _f(np.atleast_2d(theta0))
        A, q = theta0.shape
        Xb, yb, s2, idx, C, n, d = self._sets(Xs, ys, sigma2s, set_of, A)
        steps = np.ascontiguousarray(np.asarray(steps, dtype=np.float64))
        if steps.ndim != 3 or steps.shape[0] != A or steps.shape[2] != q:
            raise ValueError("steps must be [A, T, q]")
        T = steps.shape[1]
        logu = np.ascontiguousarray(np.asarray(logu, dtype=np.float64).reshape(A, T))
        l0 = np.ascontiguousarray(np.asarray(l0, dtype=np.float64).reshape(A))
        b0 = None if beta0 is None else np.ascontiguousarray(np.asarray(beta0, dtype=np.float64).reshape(A))
        n_prop = np.ascontiguousarray(np.asarray(n_prop).reshape(A).astype(np.int32))
        stop_acc = np.ascontiguousarray(np.asarray(stop_acc).reshape(A).astype(np.int32))
        M = max(int(stop_acc.max()) if A else 1, 1)
        pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
        used, acc = np.zeros(A, dtype=np.int32), np.zeros(A, dtype=np.int32)
        draws, dval, dbeta = np.empty((A, M, q)), np.empty((A, M)), np.empty((A, M))
        theta, l, beta = np.empty((A, q), order="F"), np.empty(A), np.empty(A)
        tr = (np.empty((A, T)), np.empty((A, T)), np.zeros((A, T), dtype=np.int32), np.zeros((A, T), dtype=np.int32)) \
            if trace else (None, None, None, None)
        failed = self._chk(lib().ccgp_metro_segments_sets(
            self._h, _p(Xb), n, d, _p(yb), _p(s2), C, int(prior_id), _p(pp), A, _ipt(idx), _p(theta0), _p(l0), _p(b0), T,
            _p(steps), _p(logu), _ipt(n_prop), _ipt(stop_acc), M, _ipt(used), _ipt(acc), _p(draws), _p(dval), _p(dbeta),
            _p(theta), _p(l), _p(beta), _p(tr[0]), _p(tr[1]), _ipt(tr[2]), _ipt(tr[3])))
        out = dict(used=used, accepted=acc, draws=draws, draw_val=dval, draw_beta=dbeta, theta=np.ascontiguousarray(theta),
                   l=l, beta=beta, failed=failed)
        if trace:
            out.update(trace_val=tr[0], trace_beta=tr[1], trace_status=tr[2], trace_accept=tr[3])
        return out

    def profile_batch_sets(self, Xs, ys, K, params, set_of, grad=True):
        """ccgp_profile_batch_sets: row b of params [B, K + K*d] on training set set_of[b] of the C sets Xs [C, n, d],
        ys [C, n] in one call.  Returns what profile_batch returns -- (loglik[B], sigma2[B], beta[B], grad[B, P] or None,
        status[B]) -- each row with the bits profile_batch gives it on its set alone."""
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, B)
        _check_columns(P, K + K * d, "K + K*d")
        ll, s2, beta, st = _outputs(B, 3)
        g = np.empty((B, P), dtype=np.float64, order="F") if grad else None
        self._chk(lib().ccgp_profile_batch_sets(self._h, _p(Xb), n, d, _p(yb), C, K, _p(params), _ipt(idx), B, _p(ll), _p(s2),
                                                _p(beta), _p(g), _ipt(st)))
        return ll, s2, beta, g, st

    def profile_fit_eval_sets(self, Xs, ys, logtheta, set_of, grad=True):
        """ccgp_profile_fit_eval_sets: the ordinary-kriging objective at the rows of logtheta [B, d], row b on training set
        set_of[b] -- theta = exp(logtheta) by the portable exp, f = -loglik, g = -(d loglik / d theta) theta -- the host twin
        of profile_fit_sets' evaluation.  Returns (f[B], g[B, d] or None, theta[B, d], sigma2[B], beta[B], status[B])."""
        logtheta = _f(np.atleast_2d(logtheta))
        B, dd = logtheta.shape
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, B)
        _check_columns(dd, d, "d")
        f, s2, beta, st = _outputs(B, 3)
        g = np.empty((B, d), order="F") if grad else None
        theta = np.empty((B, d), order="F")
        self._chk(lib().ccgp_profile_fit_eval_sets(self._h, _p(Xb), n, d, _p(yb), C, _p(logtheta), _ipt(idx), B, _p(f), _p(g),
                                                   _p(theta), _p(s2), _p(beta), _ipt(st)))
        return f, g, theta, s2, beta, st

    def profile_fit_sets(self, Xs, ys, set_of, state, max_evals, trace=False, T=None):
        """ccgp_profile_fit_sets: A starts, start a on training set set_of[a], stepped on the device from state [A, W]
        (api.fit_begin) through up to max_evals[a] evaluations each.  Returns dict(state [A, W], evals[A], failed: evaluations
        whose factorisation failed, and with trace=True trace_f, trace_status [A, T], T = max(max_evals) unless given)."""
        state = np.ascontiguousarray(np.atleast_2d(np.asarray(state, dtype=np.float64))).copy()
        A = state.shape[0]
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, A)
        max_evals = np.ascontiguousarray(np.broadcast_to(np.asarray(max_evals), (A,)).astype(np.int32))
        if T is None:
            T = int(max_evals.max()) if A else 0
        if state.shape[1] != fit_state_doubles(d):
            raise ValueError("state must be [A, %d] for d = %d" % (fit_state_doubles(d), d))
        evals = np.zeros(A, dtype=np.int32)
        tr_f, tr_st = (np.full((A, T), np.nan), np.full((A, T), -1, dtype=np.int32)) if trace else (None, None)
        failed = self._chk(lib().ccgp_profile_fit_sets(self._h, _p(Xb), n, d, _p(yb), C, A, _ipt(idx), _p(state),
                                                       _ipt(max_evals), _ipt(evals), _p(tr_f), _ipt(tr_st), int(T)))
        out = dict(state=state, evals=evals, failed=failed)
        if trace:
            out.update(trace_f=tr_f, trace_status=tr_st)
        return out

    def laplace_search_sets(self, Xs, ys, sigma2s, prior_id, set_of, state, max_evals, prior_pars=None, trace=False, T=None):
        """ccgp_laplace_search_sets: A Nelder-Mead searches, search a on training set set_of[a], stepped on the device from
        state [A, W] (api.nm_begin) through up to max_evals[a] evaluations each.  Returns dict(state [A, W], evals[A], failed:
        evaluations whose factorisation failed, and with trace=True trace_val, trace_status [A, T], T = max(max_evals) unless
        given)."""
        state = np.ascontiguousarray(np.atleast_2d(np.asarray(state, dtype=np.float64))).copy()
        A = state.shape[0]
        Xb, yb, s2, idx, C, n, d = self._sets(Xs, ys, sigma2s, set_of, A)
        max_evals = np.ascontiguousarray(np.broadcast_to(np.asarray(max_evals), (A,)).astype(np.int32))
        if T is None:
            T = int(max_evals.max()) if A else 0
        pp = _f(np.ravel(prior_pars)) if prior_pars is not None else None
        q = 4 if int(prior_id) == PRIOR_ANI else 3
        if state.shape[1] != nm_state_doubles(q):
            raise ValueError("state must be [A, %d] for this prior (q = %d)" % (nm_state_doubles(q), q))
        evals = np.zeros(A, dtype=np.int32)
        tr_v, tr_st = (np.full((A, T), np.nan), np.full((A, T), -1, dtype=np.int32)) if trace else (None, None)
        failed = self._chk(lib().ccgp_laplace_search_sets(self._h, _p(Xb), n, d, _p(yb), _p(s2), C, int(prior_id), _p(pp), A,
                                                          _ipt(idx), _p(state), _ipt(max_evals), _ipt(evals), _p(tr_v),
                                                          _ipt(tr_st), int(T)))
        out = dict(state=state, evals=evals, failed=failed)
        if trace:
            out.update(trace_val=tr_v, trace_status=tr_st)
        return out

    def cgp_state_batch_sets(self, Xs, ys, params, set_of, skip=None):
        """ccgp_cgp_state_batch_sets: the CGP state at row b of params [B, 2 d + 2] on training set set_of[b] of the C sets
        Xs [C, n, d], ys [C, n] in one call, skip[B] as in cgp_state_batch.  Returns what cgp_state_batch returns -- (val[B],
        beta[B], tau2[B], loo[B] or None without skip, status[B]) -- each row with the bits it has on its set alone."""
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, B)
        _check_columns(P, 2 * d + 2, "2 d + 2")
        sk = _skip_rows(skip, B)
        val, beta, tau2, st = _outputs(B, 3)
        loo = np.empty(B) if sk is not None else None
        self._chk(lib().ccgp_cgp_state_batch_sets(self._h, _p(Xb), n, d, _p(yb), C, _p(params), _ipt(idx), B, _ipt(sk), _p(val),
                                                  _p(beta), _p(tau2), _p(loo), _ipt(st)))
        return val, beta, tau2, loo, st

    def _sets_sites(self, Xs, ys, sigma2s, K, params, set_of, Xtests):
        """What the three Gaussian sets predictions share: _sets, the B x (K + K d) rows and the sets' test sites [C, m, d] as
        C column-major blocks."""
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        Xb, yb, s2, idx, C, n, d = self._sets(Xs, ys, sigma2s, set_of, B)
        _check_columns(P, K + K * d, "K + K*d")
        Xt = np.asarray(Xtests, dtype=np.float64)
        if Xt.ndim != 3 or Xt.shape[0] != C or Xt.shape[2] != d:
            raise ValueError("Xtests must be [C, m, d]: the sets of one call have as many test sites each")
        return Xb, yb, s2, idx, C, n, d, params, B, np.ascontiguousarray(np.transpose(Xt, (0, 2, 1))), Xt.shape[1]

    def predict_batch_sets(self, Xs, ys, sigma2s, K, params, set_of, Xtests):
        """ccgp_predict_batch_sets: row b of params on training set set_of[b] of the C sets Xs [C, n, d], ys [C, n], sigma2s [C],
        predicted at that set's own test sites Xtests [C, m, d].  Returns what predict_batch returns -- (mean[B, m], var[B, m],
        beta[B], status[B]) -- each row with the bits predict_batch gives it on its set alone."""
        Xb, yb, s2, idx, C, n, d, params, B, Xtb, m = self._sets_sites(Xs, ys, sigma2s, K, params, set_of, Xtests)
        mean, var = np.empty((B, m), order="F"), np.empty((B, m), order="F")
        beta, st = _outputs(B, 1)
        self._chk(lib().ccgp_predict_batch_sets(self._h, _p(Xb), n, d, _p(yb), _p(s2), C, K, _p(params), _ipt(idx), B, _p(Xtb), m,
                                                _p(mean), _p(var), _p(beta), _ipt(st)))
        return mean, var, beta, st

    def krige_predict_batch_sets(self, Xs, ys, K, params, set_of, sigma2, Xtests, form):
        """ccgp_krige_predict_batch_sets: row b of params is one fitted single-GP model of training set set_of[b] with its own
        sigma2[b] (None for VAR_UNBIASED), predicted at that set's test sites Xtests [C, m, d].  Returns what
        krige_predict_batch returns -- (mean[B, m], var[B, m], beta[B], q[B], status[B]) -- each row with its bits there."""
        Xb, yb, _, idx, C, n, d, params, B, Xtb, m = self._sets_sites(Xs, ys, None, K, params, set_of, Xtests)
        s2 = None if sigma2 is None else _f(np.broadcast_to(np.asarray(sigma2, dtype=np.float64), (B,)).copy())
        mean, var = np.empty((B, m), order="F"), np.empty((B, m), order="F")
        beta, q, st = _outputs(B, 2)
        self._chk(lib().ccgp_krige_predict_batch_sets(self._h, _p(Xb), n, d, _p(yb), C, K, _p(params), _ipt(idx), B, _p(s2),
                                                      int(form), _p(Xtb), m, _p(mean), _p(var), _p(beta), _p(q), _ipt(st)))
        return mean, var, beta, q, st

    def predict_summary_sets(self, Xs, ys, sigma2s, K, params, set_of, Xtests, probs, ys_at=None):
        """ccgp_predict_summary_sets: prediction()'s per-site summaries per training set -- set c's from the rows with
        set_of[b] == c -- at that set's own test sites Xtests [C, m, d]; ys_at [C, m] adds cdf_at.  Returns a list of C dicts
        as predict_summary returns them (beta, status: the set's rows in their order; n_failed: the set's), each with the bits
        predict_summary gives on that set's rows alone; a set without rows is NaN throughout."""
        Xb, yb, s2, idx, C, n, d, params, B, Xtb, m = self._sets_sites(Xs, ys, sigma2s, K, params, set_of, Xtests)
        probs = _probs(probs)
        yat = None if ys_at is None else np.ascontiguousarray(np.asarray(ys_at, dtype=np.float64).reshape(C, m))
        out = np.empty((C, 4 + probs.size, m))
        beta, st = _outputs(B, 1)
        self._chk(lib().ccgp_predict_summary_sets(self._h, _p(Xb), n, d, _p(yb), _p(s2), C, K, _p(params), _ipt(idx), B, _p(Xtb),
                                                  m, _p(probs), probs.size, _p(yat), _p(out), _p(beta), _ipt(st)))
        res = []
        for c in range(C):
            rows = np.flatnonzero(idx == c)
            res.append(_summary_dict(np.asfortranarray(out[c].T), int(np.count_nonzero(st[rows])), beta[rows], st[rows]))
        return res

    def cgp_predict_sets(self, Xs, ys, params, set_of, Xtests):
        """ccgp_cgp_predict_sets: the final CGP state at row b of params [B, 2 d + 2] on training set set_of[b] of the C sets
        Xs [C, n, d], ys [C, n], and predict.CGP(PI = TRUE) at that set's own test sites Xtests [C, m, d] (m may be 0), all
        rows in one call.  Returns (out[B, m, 6], keeps: per row what cgp_predict returns -- dict(s, res2, temp, sf, beta, tau2)
        or None where the row's state failed --, status[B]), each row with the bits cgp_predict gives it on its set alone."""
        params = _f(np.atleast_2d(params))
        B, P = params.shape
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, B)
        _check_columns(P, 2 * d + 2, "2 d + 2")
        Xt = np.asarray(Xtests, dtype=np.float64)
        if Xt.ndim != 3 or Xt.shape[0] != C or Xt.shape[2] != d:
            raise ValueError("Xtests must be [C, m, d]: the sets of one call have as many test sites each")
        m = Xt.shape[1]
        Xtb = np.ascontiguousarray(np.transpose(Xt, (0, 2, 1)))
        blocks = np.empty((B, 6, m))
        state = np.empty((B, 3 * n + 3))
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_cgp_predict_sets(self._h, _p(Xb), n, d, _p(yb), C, _p(params), _ipt(idx), B, _p(Xtb) if m else None,
                                              m, _p(blocks) if m else None, _p(state), _ipt(st)))
        keeps = [None if st[b] else dict(s=state[b, :n].copy(), res2=state[b, n:2 * n].copy(), temp=state[b, 2 * n:3 * n].copy(),
                                         sf=float(state[b, 3 * n]), beta=float(state[b, 3 * n + 1]),
                                         tau2=float(state[b, 3 * n + 2])) for b in range(B)]
        return np.transpose(blocks, (0, 2, 1)), keeps, st

    def cgp_fit_eval_sets(self, Xs, ys, w, lower, upper, step, set_of):
        """ccgp_cgp_fit_eval_sets: the CGP refinement's objective at the points w [B, d + 3] = (lambda, theta, kappa, bw), point b
        on training set set_of[b] under its box lower[b], upper[b] ([B, d + 3]) -- f = the value at w (1e6 where it is not
        finite), g by central differences of `step` clipped at the box -- the host twin of cgp_fit_sets' evaluation.  Returns
        (f[B], g[B, d + 3], status[B]: the centre row's)."""
        w = _f(np.atleast_2d(w))
        B, P = w.shape
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, B)
        _check_columns(P, d + 3, "d + 3")
        lo = _f(np.broadcast_to(np.asarray(lower, dtype=np.float64), (B, P)))
        hi = _f(np.broadcast_to(np.asarray(upper, dtype=np.float64), (B, P)))
        f, st = _outputs(B, 1)
        g = np.empty((B, P), order="F")
        self._chk(lib().ccgp_cgp_fit_eval_sets(self._h, _p(Xb), n, d, _p(yb), C, _p(w), _p(lo), _p(hi), float(step), _ipt(idx), B,
                                               _p(f), _p(g), _ipt(st)))
        return f, g, st

    def cgp_fit_sets(self, Xs, ys, set_of, state, step, max_evals, look=16, trace=False, T=None):
        """ccgp_cgp_fit_sets: A starts of the CGP refinement, start a on training set set_of[a], stepped on the device from state
        [A, W] (api.fit_begin at (lambda, theta, kappa, bw) under the start's box) through up to max_evals[a] evaluations each:
        rounds of two launches (evaluate, step), `look` of them between the host's looks at the gates.  Returns dict(state
        [A, W], evals[A], failed: evaluations whose centre row failed, and with trace=True trace_f, trace_status [A, T],
        T = max(max_evals) unless given)."""
        state = np.ascontiguousarray(np.atleast_2d(np.asarray(state, dtype=np.float64))).copy()
        A = state.shape[0]
        Xb, yb, _, idx, C, n, d = self._sets(Xs, ys, None, set_of, A)
        max_evals = np.ascontiguousarray(np.broadcast_to(np.asarray(max_evals), (A,)).astype(np.int32))
        if T is None:
            T = int(max_evals.max()) if A else 0
        if state.shape[1] != FIT_HEADER + 16 * (d + 3):
            raise ValueError("state must be [A, %d] for d = %d (d + 3 variables)" % (FIT_HEADER + 16 * (d + 3), d))
        evals = np.zeros(A, dtype=np.int32)
        tr_f, tr_st = (np.full((A, T), np.nan), np.full((A, T), -1, dtype=np.int32)) if trace else (None, None)
        failed = self._chk(lib().ccgp_cgp_fit_sets(self._h, _p(Xb), n, d, _p(yb), C, A, _ipt(idx), _p(state), float(step),
                                                   _ipt(max_evals), int(look), _ipt(evals), _p(tr_f), _ipt(tr_st), int(T)))
        out = dict(state=state, evals=evals, failed=failed)
        if trace:
            out.update(trace_f=tr_f, trace_status=tr_st)
        return out

    def grid_marginal(self, X, y, sigma2, hyper, N, tau, take_log, aniso_lambda=-1.0, want_logs=False):
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        hyper = _f(hyper)
        G = hyper.shape[0]
        if hyper.shape[1] != 4:
            raise ValueError("hyper must be G x 4")
        out = np.empty(G)
        arg = c_int()
        logs = np.empty((G, N), dtype=np.float64) if want_logs else None
        self._chk(lib().ccgp_grid_marginal(self._h, _p(X), n, d, _p(y), float(sigma2), _p(hyper), G,
                                           int(N), float(tau), 1 if take_log else 0,
                                           float(aniso_lambda), _p(out), ctypes.byref(arg), _p(logs)))
        return (out, arg.value, logs) if want_logs else (out, arg.value)

    # -- 8(f)-4: entropy criteria ------------------------------------------------------------
    def mixed_logdet_designs(self, designs, K, params_row):
        """designs: [B, n, d] candidate designs sharing one parameter row -> (logdet[B], status[B])."""
        designs = np.asarray(designs, dtype=np.float64)
        B, n, d = designs.shape
        Xs = np.ascontiguousarray(np.stack([np.asfortranarray(D).ravel(order="F") for D in designs]))
        row = _f(params_row, (K + K * d,))
        out = np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_mixed_logdet_designs(self._h, _p(Xs), n, d, B, K, _p(row), _p(out), _ipt(st)))
        return out, st

    def mixed_logdet_grad_designs(self, designs, K, params_row, n_fixed=0):
        """designs: [B, n, d] sharing one parameter row -> (logdet[B], grad[B, n - n_fixed, d], status[B]):
        d log det R_mixed / d x of the rows >= n_fixed (NaN and status != 0 where the elimination failed)."""
        designs = np.asarray(designs, dtype=np.float64)
        B, n, d = designs.shape
        nf = int(n_fixed)
        Xs = np.ascontiguousarray(np.stack([np.asfortranarray(D).ravel(order="F") for D in designs]))
        row = _f(params_row, (K + K * d,))
        out = np.empty(B)
        g = np.empty(B * max(n - nf, 0) * d)
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_mixed_logdet_grad_designs(self._h, _p(Xs), n, d, B, K, _p(row), nf, _p(out), _p(g), _ipt(st)))
        return out, g.reshape(B, d, n - nf).transpose(0, 2, 1), st

    @staticmethod
    def _design_fit_shared(D_old, d, K, params_row):
        """The inputs every start of a design search shares: D_old [n_fixed, d] or None -> (column-major copy or None, n_fixed,
        the parameter row)."""
        old = None if D_old is None else np.asarray(D_old, dtype=np.float64).reshape(-1, d)
        nf = 0 if old is None else old.shape[0]
        if nf == 0:
            old = None
        else:
            old = np.ascontiguousarray(np.asfortranarray(old).ravel(order="F"))
        return old, nf, _f(params_row, (K + K * d,))

    def design_fit_eval(self, x, K, params_row, D_old=None, ld_offset=0.0):
        """ccgp_design_fit_eval: the design search's objective at the points x [B, n_free, d] (the free rows of B designs;
        D_old [n_fixed, d] or None is the fixed batch on top of each) -- f = -(log det R - ld_offset), g = -(d log det R / d x)
        -- the host twin of design_fit's evaluation.  Returns (f[B], g[B, n_free, d], status[B])."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        B, nfree, d = x.shape
        old, nf, row = self._design_fit_shared(D_old, d, K, params_row)
        f = np.empty(B)
        g = np.empty((B, nfree, d))
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_design_fit_eval(self._h, _p(old), nf, nf + nfree, d, K, _p(row), float(ld_offset), _p(x), B, _p(f),
                                             _p(g), _ipt(st)))
        return f, g, st

    def design_fit(self, n_free, d, K, params_row, state, max_evals, D_old=None, ld_offset=0.0, trace=False, T=None):
        """ccgp_design_fit: A starts of the design search (n_free free rows of d dimensions each under D_old [n_fixed, d] or
        None), stepped on the device from state [A, W] (api.fit_begin at the raveled start) through up to max_evals[a]
        evaluations each.  Returns dict(state [A, W], evals[A], failed: evaluations whose elimination failed, and with
        trace=True trace_f, trace_status [A, T], T = max(max_evals) unless given)."""
        state = np.ascontiguousarray(np.atleast_2d(np.asarray(state, dtype=np.float64))).copy()
        A = state.shape[0]
        nfree, d = int(n_free), int(d)
        old, nf, row = self._design_fit_shared(D_old, d, K, params_row)
        max_evals = np.ascontiguousarray(np.broadcast_to(np.asarray(max_evals), (A,)).astype(np.int32))
        if T is None:
            T = int(max_evals.max()) if A else 0
        if state.shape[1] != FIT_HEADER + 16 * nfree * d:
            raise ValueError("state must be [A, %d] for %d free rows of %d dimensions" % (FIT_HEADER + 16 * nfree * d, nfree, d))
        evals = np.zeros(A, dtype=np.int32)
        tr_f, tr_st = (np.full((A, T), np.nan), np.full((A, T), -1, dtype=np.int32)) if trace else (None, None)
        failed = self._chk(lib().ccgp_design_fit(self._h, _p(old), nf, nf + nfree, d, K, _p(row), float(ld_offset), A, _p(state),
                                                 _ipt(max_evals), _ipt(evals), _p(tr_f), _ipt(tr_st), int(T)))
        out = dict(state=state, evals=evals, failed=failed)
        if trace:
            out.update(trace_f=tr_f, trace_status=tr_st)
        return out

    # -- a10 + a11 -------------------------------------------------------------------------
    def predict_batch(self, X, y, K, params, Xtest, sigma2):
        """Returns (mean[S, m], var[S, m], beta[S], status[S])."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        S = params.shape[0]
        Xtest = _f(np.atleast_2d(Xtest))
        m = Xtest.shape[0]
        mean = np.empty((S, m), dtype=np.float64, order="F")
        var = np.empty((S, m), dtype=np.float64, order="F")
        beta = np.empty(S)
        st = np.zeros(S, dtype=np.int32)
        self._chk(lib().ccgp_predict_batch(self._h, _p(X), n, d, _p(y), K, _p(params), S, _p(Xtest), m,
                                           float(sigma2), _p(mean), _p(var), _p(beta), _ipt(st)))
        return mean, var, beta, st

    def krige_predict_batch(self, X, y, K, params, sigma2, Xtest, form):
        """ccgp_krige_predict_batch: the single-GP comparator's prediction.  Row b of params is one fitted model with its own
        sigma2[b] (ignored, may be None, for VAR_UNBIASED); form: VAR_ORDINARY (predict.post), VAR_PLUGIN (mlegp's
        se.fit^2 = sigma2 (1 - r'R^-1 r)) or VAR_UNBIASED (Q / (n - 1) in place of sigma2, D1:504-516).
        Returns (mean[B, m], var[B, m], beta[B], q[B], status[B]); q[b] = (y - beta 1)'R^-1 (y - beta 1)."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B = params.shape[0]
        if params.shape[1] != K + K * d:
            raise ValueError("params must have K + K*d = %d columns" % (K + K * d))
        s2 = None
        if sigma2 is not None:
            s2 = _f(np.broadcast_to(np.asarray(sigma2, dtype=np.float64), (B,)).copy())
        Xtest = _f(np.atleast_2d(Xtest))
        m = Xtest.shape[0]
        mean = np.empty((B, m), dtype=np.float64, order="F")
        var = np.empty((B, m), dtype=np.float64, order="F")
        beta, q = np.empty(B), np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_krige_predict_batch(self._h, _p(X), n, d, _p(y), K, _p(params), B, _p(s2), int(form),
                                                 _p(Xtest), m, _p(mean), _p(var), _p(beta), _p(q), _ipt(st)))
        return mean, var, beta, q, st

    def predict_summary(self, X, y, K, params, Xtest, sigma2, probs, y_at=None):
        """prediction()'s per-site summaries (HX:686-703) of the S draws, computed on the device from the exact
        posterior predictive (the equal-weight mixture of the draws' normals); only m x (4 + n_probs) doubles come
        back.  Returns a dict: y_hat[m], pred_var[m], quant[m], cdf_at[m] (NaN without y_at), quantiles[m, n_probs],
        beta[S], status[S], n_failed."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        S = params.shape[0]
        Xtest = _f(np.atleast_2d(Xtest))
        m = Xtest.shape[0]
        probs = _probs(probs)
        y_at = _f(np.ravel(y_at), (m,)) if y_at is not None else None
        out = np.empty((m, 4 + probs.size), dtype=np.float64, order="F")
        beta = np.empty(S)
        st = np.zeros(S, dtype=np.int32)
        bad = self._chk(lib().ccgp_predict_summary(self._h, _p(X), n, d, _p(y), K, _p(params), S, _p(Xtest), m,
                                                   float(sigma2), _p(probs), probs.size, _p(y_at), _p(out), _p(beta),
                                                   _ipt(st)))
        return _summary_dict(out, bad, beta, st)

    # -- leave-one-out cross-validation ------------------------------------------------------
    def loo_batch(self, X, y, K, params, sigma2, form=VAR_ORDINARY):
        """ccgp_loo_batch: the leave-one-out mean and variance of every training point for each of the B rows of params,
        from one factorisation per row (Dubrule 1983) -- what B x n calls of predict_batch on the n - 1 other points
        return.  sigma2: a scalar, an array of B values, or None (VAR_UNBIASED reads none); form as for
        krige_predict_batch, the UNBIASED form with n - 2 degrees of freedom (a fold has n - 1 points).
        Returns (mean[B, n], var[B, n], beta[B], q[B], status[B]); beta and q are the full-data values."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        B = params.shape[0]
        if params.shape[1] != K + K * d:
            raise ValueError("params must have K + K*d = %d columns" % (K + K * d))
        s2 = None
        if sigma2 is not None:
            s2 = _f(np.broadcast_to(np.asarray(sigma2, dtype=np.float64), (B,)).copy())
        mean = np.empty((B, n), dtype=np.float64, order="F")
        var = np.empty((B, n), dtype=np.float64, order="F")
        beta, q = np.empty(B), np.empty(B)
        st = np.zeros(B, dtype=np.int32)
        self._chk(lib().ccgp_loo_batch(self._h, _p(X), n, d, _p(y), K, _p(params), B, _p(s2), int(form), _p(mean),
                                       _p(var), _p(beta), _p(q), _ipt(st)))
        return mean, var, beta, q, st

    def loo_summary(self, X, y, K, params, sigma2, probs):
        """ccgp_loo_summary: predict_summary's per-site summaries of the leave-one-out posterior predictive, the sites
        being the n training points and y_at = y: the dict of predict_summary, cdf_at[i] = the PIT value F(y_i)."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        S = params.shape[0]
        probs = _probs(probs)
        out = np.empty((n, 4 + probs.size), dtype=np.float64, order="F")
        beta = np.empty(S)
        st = np.zeros(S, dtype=np.int32)
        bad = self._chk(lib().ccgp_loo_summary(self._h, _p(X), n, d, _p(y), K, _p(params), S, float(sigma2), _p(probs),
                                               probs.size, _p(out), _p(beta), _ipt(st)))
        return _summary_dict(out, bad, beta, st)

    # -- 8(f)-2: device-resident factor set -------------------------------------------------
    def factor_batch(self, X, y, K, params, sigma2):
        """Factorise the S draws once and keep the factors on the device -> FactorSet (use as a context manager or
        call .free()).  .loglik / .beta / .status hold what ccgp_loglik_batch would have returned."""
        X, y = _f(X), _f(np.ravel(y))
        n, d = X.shape
        params = _f(np.atleast_2d(params))
        S = params.shape[0]
        ll, beta = np.empty(S), np.empty(S)
        st = np.zeros(S, dtype=np.int32)
        fs = c_void_p()
        self._chk(lib().ccgp_factor_batch(self._h, _p(X), n, d, _p(y), K, _p(params), S, float(sigma2),
                                          ctypes.byref(fs), _p(ll), _p(beta), _ipt(st)))
        return FactorSet(self, fs, S, ll, beta, st)

    # -- device-resident forms (torch tensors or raw pointers) ----------------------------
    @staticmethod
    def _dptr(t):
        if t is None:
            return c_void_p(0)
        if isinstance(t, int):
            return c_void_p(t)
        return c_void_p(t.data_ptr())

    def loglik_batch_dev(self, dX, n, d, dy, K, dparams, B, sigma2, mean_mode, tau2, d_loglik, d_beta,
                         d_status):
        """All d* are device buffers (torch CUDA tensors or integer addresses): dX n*d
        column-major, dparams B x P column-major, d_status int32[B].  Asynchronous."""
        self._chk(lib().ccgp_loglik_batch_dev(self._h, self._dptr(dX), n, d, self._dptr(dy), K,
                                              self._dptr(dparams), B, float(sigma2), int(mean_mode),
                                              float(tau2), self._dptr(d_loglik), self._dptr(d_beta),
                                              self._dptr(d_status)))

    def predict_batch_dev(self, dX, n, d, dy, K, dparams, S, dXtest, m, sigma2, d_mean, d_var, d_beta,
                          d_status):
        self._chk(lib().ccgp_predict_batch_dev(self._h, self._dptr(dX), n, d, self._dptr(dy), K,
                                               self._dptr(dparams), S, self._dptr(dXtest), m,
                                               float(sigma2), self._dptr(d_mean), self._dptr(d_var),
                                               self._dptr(d_beta), self._dptr(d_status)))

    def predict_summary_dev(self, dX, n, d, dy, K, dparams, S, dXtest, m, sigma2, probs, d_y_at, d_out, d_beta=None,
                            d_status=None):
        """ccgp_predict_summary on device buffers, asynchronous: d_out is m x (4 + n_probs) column-major (float64),
        d_y_at / d_beta / d_status may be None; probs is a host sequence."""
        probs = _probs(probs)
        self._chk(lib().ccgp_predict_summary_dev(self._h, self._dptr(dX), n, d, self._dptr(dy), K, self._dptr(dparams),
                                                 S, self._dptr(dXtest), m, float(sigma2), _p(probs), probs.size,
                                                 self._dptr(d_y_at), self._dptr(d_out), self._dptr(d_beta),
                                                 self._dptr(d_status)))
