"""The analytic gradient (ccgp_loglik_grad_batch) and the explicit inverse (solve(R), HX:454) against an exact reference,
on every device route that computes them.

The reference has no gradient (LearnBayes::laplace differences numerically, HX:493); the library's closed form is
  M = (alpha alpha' - Sigma^-1) / 2,  dll/dw_q = sum_ab M_ab 2 sigma2 w_q R_q,ab,
  dll/dtheta_qk = -sum_ab M_ab sigma2 w_q^2 (x_ak - x_bk)^2 R_q,ab,
evaluated by oracle/ccgp_oracle.loglik_grad_exact in long double (hand-written Cholesky, eps 1.1e-19) up to n = 520, and
in fp64 (LAPACK) at n >= 2048, where the long-double evaluation would take minutes.  Every gradient component j of every
checked draw must satisfy

    |g_dev[j] - g_ref[j]| <= C * eps * cond1(R) * (1 + rho) * scale[j],      C = oracle.ccgp_oracle.GRAD_TOL_C = 128,

with scale[j] = sum_ab |M_ab| |dSigma_ab / d row_j|, the size of the sum before cancellation, and rho = max_c,a 2 sum_k
theta_ck x_ak^2 (oracle.expanded_form_magnitude).  rho is there because the device, like the reference scripts, forms each
exponent in the expanded form u_a + u_b - 2 sum_k theta_k x_ak x_bk (HX:352-355): its absolute rounding, ~eps rho, is a
relative error of every kernel value that the reference (direct squared differences) does not share.  Without it the
register instance at n = 128, d = 1, theta = 6.5e4 (rho = 1.3e5, cond1 = 152) sat at 203 x eps cond1 scale while every
other case stayed below 0.04.  Why this C: the device
forms Sigma^-1 by a Cholesky sweep, whose backward error perturbs M by about n eps |Sigma^-1| |Sigma| |Sigma^-1| <= cond1 eps
times |M|-sized terms (the n of that bound is a worst case that random rounding does not reach), the kernel values by a few
ulps (the polynomial exp, tests/test_gpu_parity.py), and the contraction adds one rounding per pair; 128 covers those with
headroom of about two orders of magnitude over the fp64 LAPACK evaluation (tests/test_oracle.py holds the fp64 oracle to
the same band against 50 digits) while staying 1e4 or more below what a wrong pair weight, a dropped or doubled 64 x 64
tile, a padded dimension leaking into a real one or a skipped component group moves (tests/test_oracle.py: the band
rejects each of them).  The draws have cond1 <= 1e8 (asserted), so no band is vacuous, and no atol is taken from the
largest component: a component 1e6 times smaller than its neighbours is held to its own scale.  The log-likelihood and
beta are held to the same C with their own cancellation-free sizes (oracle.loglik_beta_scales); at n >= 2048 the band is
doubled for the fp64 reference's own error.

Route of each case: the timing counters separate the n <= 128 evaluators (CCGP_T_FUSED) from the blocked sweep (the
gradient contraction is timed as CCGP_T_SOLVE, the persistent scheduler as CCGP_T_SWEEP); which of the two n <= 128
evaluators runs is decided by the predicates mirrored in route() below.
"""
import math

import numpy as np
import pytest

from conftest import synthetic_design
from oracle import ccgp_oracle as orc

EPS = float(np.finfo(np.float64).eps)
KAPPA_MAX = 1e8
LDS_LIMIT = 160 * 1024 - 64           # kLdsBytes - 64 (csrc/ccgp_internal.h)
MAX_RATIO = {}                        # route -> largest |g_dev - g_ref| / (eps cond1 (1 + rho) scale) seen


# ----------------------------------------------------------------------------- mirrors of the C++ route predicates
def small_lds_bytes(n, d, mtile):
    """csrc/small.hip small_lds_bytes (kMaxK = 8, kExpTableDoubles = 256)."""
    return 8 * ((n + 2 + mtile) * n + d * n + 8 * n + d * mtile + 8 * mtile + 8 * d + 8 + 16 + 256)


def small_reg_inverse_supported(n, d, K):
    """csrc/small_reg.hip small_reg_inverse_supported: kPerMat(16 NB, 16, NB + 1, K, d, inv = true) doubles per matrix plus
    the design (CCGP_SMALL_EXP_TABLE = 0: no table)."""
    if n > 128:
        return False
    NP = 16 * ((n + 15) // 16)
    per_mat = K * NP + K * d + K + 2 * (NP + 16 * (NP // 16 + 1)) + NP + 2 * NP + 8 + NP * (NP + 2) + 1 + 4 * 28
    return 8 * (d * n + per_mat) <= LDS_LIMIT


def blocked_grad_supported(d, K):
    """csrc/blocked.hip blocked_grad_supported / grad_contract_lds."""
    return 8 * (256 + (2 * d + 2 * K) * 64 + K * d + 4 * (K + K * d)) <= LDS_LIMIT


def route(n, d, K):
    """csrc/capi.hip ccgp_loglik_grad_batch: blocked when n > kSmallMaxN or small_lds_bytes(n, d, 1) does not fit; else the
    register-resident instance when small_reg_inverse_supported, else the LDS evaluator of small.hip."""
    if n > 128 or small_lds_bytes(n, d, 1) > LDS_LIMIT:
        return "blocked"
    return "reg" if small_reg_inverse_supported(n, d, K) else "lds"


def scheduled(npad, nb):
    """csrc/blocked.hip sched_mode() at CCGP_OPT_SCHED = 3 (default): the persistent sweep for nt >= 16 tiles of 128 and
    chunks of 32 ... 128 matrices (on a whole 256-CU device)."""
    return npad // 128 >= 16 and 32 <= nb <= 128


# ----------------------------------------------------------------------------- helpers
def _rows(X, K, d, B, seed):
    rng = np.random.default_rng(seed)
    return np.stack([orc.conditioned_row(X, K, d, rng, KAPPA_MAX)[0] for _ in range(B)])


def _timed(handle, fn):
    handle.enable_timing(True)
    try:
        out = fn()
        t = handle.get_timing()
    finally:
        handle.enable_timing(False)
    return out, t


def check_draw(X, y, row, K, d, s2, got, tag, dtype=np.longdouble, c=orc.GRAD_TOL_C):
    """got = (ll, beta, grad) of one draw from the device; every component within its band."""
    parts = orc.loglik_grad_parts(X, y, row, K, d, s2, np.dtype(dtype).type)
    kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
    assert kappa <= KAPPA_MAX, (tag, kappa)
    g_ref, scale = orc.grad_from_parts(parts, X, row, K, d, s2)
    g_ref, scale = g_ref.astype(np.float64), scale.astype(np.float64)
    ll, beta, g = got
    unit = EPS * kappa * (1.0 + orc.expanded_form_magnitude(X, row, K, d))
    ratio = np.abs(g - g_ref) / (unit * scale)
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float(ratio.max()))
    bad = np.nonzero(~(ratio <= c))[0]
    assert bad.size == 0, "%s: components %s off by %s x eps cond1 scale (cond1 %.3g)" % (tag, bad[:8], ratio[bad[:8]], kappa)
    s_ll, s_beta = orc.loglik_beta_scales(parts, y)
    check_loglik_beta(float(parts["loglik"]), float(parts["beta"]), unit * s_ll, unit * s_beta, ll, beta, tag, c)


def check_loglik_beta(ll_ref, beta_ref, unit_ll, unit_beta, ll, beta, tag, c=orc.GRAD_TOL_C):
    """The log-likelihood and beta of one mode-0 draw: each within c of its unit = eps cond1 (1 + rho) times its
    cancellation-free size (oracle.loglik_beta_scales).  Returns the two ratios |dev - ref| / unit."""
    r_ll, r_beta = abs(ll - ll_ref) / unit_ll, abs(beta - beta_ref) / unit_beta
    assert r_ll <= c, (tag, ll, ll_ref, r_ll)
    assert r_beta <= c, (tag, beta, beta_ref, r_beta)
    return r_ll, r_beta


def _design(n, d, seed):
    X, y = synthetic_design(n, d, seed=seed)
    return X, y + 0.3 * X[:, 0]           # a trend: beta and alpha not symmetric in the design


# ----------------------------------------------------------------------------- n <= 128: register-resident instance
REG_CASES = [(2, 1, 1), (5, 4, 2), (5, 8, 8), (16, 5, 3), (17, 8, 4), (17, 9, 1), (63, 9, 7), (64, 1, 8), (64, 8, 8),
             (65, 4, 3), (100, 5, 8), (100, 9, 7), (127, 8, 2), (128, 9, 4), (128, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K", REG_CASES)
def test_register_gradient_exact(handle, n, d, K):
    assert route(n, d, K) == "reg"
    X, y = _design(n, d, seed=1000 + 17 * n + d)
    rows = _rows(X, K, d, 2, seed=n * 64 + d * 8 + K)
    (ll, beta, grad, st), t = _timed(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 0.8))
    assert t["fused"][1] > 0 and t["solve"][1] == 0 and not st.any()
    for b in range(2):
        check_draw(X, y, rows[b], K, d, 0.8, (ll[b], beta[b], grad[b]), "reg")


# ----------------------------------------------------------------------------- n <= 128: LDS evaluator (small.hip)
LDS_CASES = [(97, 56, 8), (97, 63, 4), (113, 24, 8), (100, 64, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K", LDS_CASES)
def test_lds_gradient_exact(handle, n, d, K):
    """The register instance does not fit these (d large with many components) but the LDS evaluator does."""
    assert route(n, d, K) == "lds"
    X, y = _design(n, d, seed=2000 + n + d)
    rows = _rows(X, K, d, 2, seed=n + d + K)
    (ll, beta, grad, st), t = _timed(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 1.1))
    assert t["fused"][1] > 0 and t["solve"][1] == 0 and not st.any()
    for b in range(2):
        check_draw(X, y, rows[b], K, d, 1.1, (ll[b], beta[b], grad[b]), "lds")


# ----------------------------------------------------------------------------- blocked: grad_contract_kernel<4|6|8|0>
D_MAX_K2 = max(dd for dd in range(1, 65) if blocked_grad_supported(dd, 2))
BLOCKED_CASES = [(129, 3, 1), (191, 6, 2), (192, 8, 8), (193, 9, 2), (255, 17, 1), (257, 33, 2), (257, 9, 8),
                 (383, D_MAX_K2, 2), (520, 6, 8), (520, 3, 2), (128, 64, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K", BLOCKED_CASES)
def test_blocked_gradient_exact(handle, n, d, K):
    """Around the 64-row contraction tiles and the 128-row Cholesky tiles; d <= 4, 6, 8 and the generic instance; n = 128
    with d = 64 is the blocked route below kSmallMaxN (the LDS evaluator does not fit)."""
    assert route(n, d, K) == "blocked" and blocked_grad_supported(d, K)
    X, y = _design(n, d, seed=3000 + n + d)
    rows = _rows(X, K, d, 2, seed=7 * n + d + K)
    (ll, beta, grad, st), t = _timed(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 1.3))
    assert t["fused"][1] == 0 and t["solve"][1] > 0 and t["sweep"][1] == 0 and not st.any()
    for b in range(2):
        check_draw(X, y, rows[b], K, d, 1.3, (ll[b], beta[b], grad[b]), "blocked")


def test_route_table_reaches_every_contraction_instance():
    """Host check of the case lists above: each instance of grad_contract_kernel and each small evaluator is covered."""
    inst = {4 if d <= 4 else 6 if d <= 6 else 8 if d <= 8 else 0 for _, d, _ in BLOCKED_CASES}
    assert inst == {0, 4, 6, 8} and D_MAX_K2 == 64
    assert all(route(*c) == "reg" for c in REG_CASES) and all(route(*c) == "lds" for c in LDS_CASES)
    assert {1, 2, 8} <= {k for _, _, k in BLOCKED_CASES}
    # several component groups (QG = 3 at d <= 8) and K = kMaxK on the register route
    assert {1, 2, 3, 4, 7, 8} <= {k for _, _, k in REG_CASES}


# ----------------------------------------------------------------------------- blocked: several chunks, failing draws
def _chunked(handle, fn, limit):
    handle.set_workspace_limit(limit)
    try:
        return _timed(handle, fn)
    finally:
        handle.set_workspace_limit(200 << 30)


@pytest.mark.gpu
def test_blocked_gradient_in_chunks_with_failing_draws(handle):
    """A workspace of ~8 MB holds two or three n = 257 matrices: the batch of 7 runs in chunks of 2 - 3.  Draws 1, 3 and 4
    have theta = 0 (R = 11', not positive definite): one inside a chunk or at its end, one at a chunk start, whatever the
    chunk size.  Their status is set and gradient NaN; every other draw passes the exact check."""
    n, d, K, B = 257, 3, 2, 7
    X, y = _design(n, d, seed=4257)
    rows = _rows(X, K, d, B, seed=4257)
    fail = [1, 3, 4]
    rows[fail, K:] = 0.0
    (ll, beta, grad, st), t = _chunked(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 1.3), 8 << 20)
    assert t["solve"][1] >= 3, t                       # one contraction per chunk: at most 3 matrices per chunk
    for b in range(B):
        if b in fail:
            assert st[b] != 0 and np.isnan(grad[b]).all()
        else:
            assert st[b] == 0
            check_draw(X, y, rows[b], K, d, 1.3, (ll[b], beta[b], grad[b]), "blocked-chunks")


# ----------------------------------------------------------------------------- blocked: persistent scheduler
@pytest.mark.gpu
@pytest.mark.parametrize("n,B", [(2048, 32), (2100, 33)])
def test_scheduled_gradient_against_fp64_closed_form(handle, n, B):
    d, K = 5, 3
    X, y = _design(n, d, seed=n)
    base, _ = orc.conditioned_row(X, K, d, np.random.default_rng(n), KAPPA_MAX)
    rows = np.stack([base * np.concatenate([np.ones(K), np.full(K * d, 1.0 + 0.02 * b)]) for b in range(B)])
    assert scheduled(128 * ((n + 127) // 128), B)
    (ll, beta, grad, st), t = _timed(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 1.0))
    assert t["sweep"][1] > 0 and t["solve"][1] > 0 and not st.any(), t
    for b in (0, B // 2, B - 1):
        check_draw(X, y, rows[b], K, d, 1.0, (ll[b], beta[b], grad[b]), "sched", np.float64, 2 * orc.GRAD_TOL_C)


@pytest.mark.gpu
def test_config4_gradient_at_n4096_against_fp64_closed_form(handle):
    """The draw of test_gpu_parity.py's n = 4096 central-difference test, now component by component."""
    n, d, K = 4096, 5, 3
    X, y = synthetic_design(n, d, seed=20140101)
    rng = np.random.default_rng(3)
    w = 0.15 + 0.55 * rng.dirichlet(np.ones(K))
    th = np.exp(rng.uniform(np.log(0.5), np.log(50.0), size=(K, d)))
    th[-1] = np.maximum(th[-1], 20.0)
    row = np.concatenate([w, th.ravel()])
    ll, beta, grad, st = handle.loglik_grad_batch(X, y, K, row[None], 1.0)
    assert st[0] == 0
    check_draw(X, y, row, K, d, 1.0, (ll[0], beta[0], grad[0]), "n4096", np.float64, 2 * orc.GRAD_TOL_C)


# ----------------------------------------------------------------------------- batch placement
def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K", [(65, 4, 3), (257, 6, 2)])
def test_gradient_bits_do_not_depend_on_batch_position(handle, n, d, K):
    """One draw at positions 0, middle and last of batches of 1, 9 and 66 (n <= 128), or of 1 and 7 in chunks of 2 - 3
    (blocked): the same bits for ll, beta and every gradient component."""
    X, y = _design(n, d, seed=5000 + n)
    probe = _rows(X, K, d, 1, seed=n)[0]
    fill = _rows(X, K, d, 2, seed=n + 1)
    ref = handle.loglik_grad_batch(X, y, K, probe[None], 1.2)
    assert ref[3][0] == 0
    sizes = (9, 66) if n <= 128 else (7,)
    for B in sizes:
        for pos in (0, B // 2, B - 1):
            rows = np.stack([fill[i % 2] for i in range(B)])
            rows[pos] = probe
            if n <= 128:
                got = handle.loglik_grad_batch(X, y, K, rows, 1.2)
            else:
                (got, t) = _chunked(handle, lambda: handle.loglik_grad_batch(X, y, K, rows, 1.2), 8 << 20)
                assert t["solve"][1] >= 3
            assert got[3][pos] == 0
            for k in range(3):
                assert np.array_equal(_bits(np.atleast_1d(got[k])[pos]), _bits(np.atleast_1d(ref[k])[0])), (B, pos, k)


# ----------------------------------------------------------------------------- explicit inverse
INV_C = 16.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 100, 128, 129, 193, 257, 520])
def test_explicit_inverse_componentwise(handle, n):
    """ccgp_logpost(..., out_Rinv) (GV prior, two isotropic components): the register instance with INV = 1 at n <= 128,
    rinv_tile_kernel<false> beyond.  Every element within INV_C n eps (|R^-1| |R| |R^-1|)_ij of the long-double inverse
    (the componentwise first-order bound of an inverse with backward error n eps |R|)."""
    from ccgp_amd import api
    d = 3
    X, y = _design(n, d, seed=6000 + n)
    rough = 2.0 * n ** (2.0 / d) / d
    p, t1, t2 = 0.7, 0.3 * rough, 1.5 * rough
    R = (p ** 2 * orc.component_corr(X, [t1] * d) + (1 - p) ** 2 * orc.component_corr(X, [t2] * d)) / (p ** 2 + (1 - p) ** 2)
    Rinv_ref = np.asarray(orc.solve_inverse_exact(R), dtype=np.float64)
    kappa = orc.cond1(R, Rinv_ref)
    assert kappa <= KAPPA_MAX
    theta_t = [math.log(t1), math.log(t2), math.log(p / (1 - p))]
    (r, tm) = _timed(handle, lambda: handle.logpost(X, y, 1.3, api.PRIOR_GV, theta_t))
    assert r["status"] == 0
    if n <= 128:
        assert small_reg_inverse_supported(n, d, 2) and tm["fused"][1] > 0 and tm["solve"][1] == 0
    else:
        assert tm["solve"][1] > 0
    A = np.abs(Rinv_ref)
    bound = n * EPS * (A @ np.abs(R) @ A)
    ratio = np.abs(r["R_inv"] - Rinv_ref) / bound
    tag = "inverse-small" if n <= 128 else "inverse-blocked"
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float(ratio.max()))
    assert ratio.max() <= INV_C, (n, ratio.max(), kappa)


@pytest.mark.gpu
def test_explicit_inverse_componentwise_lds_evaluator(handle):
    """The same check on the LDS evaluator of small.hip (launch_small_inverse), which ccgp_logpost reaches at n <= 128 when
    the register instance with INV = 1 does not fit: n = 121 with d = 22 and the two components of the GV prior (cond1 of
    this R is 4e4 in long double)."""
    from ccgp_amd import api
    n, d = 121, 22
    assert route(n, d, 2) == "lds" and not small_reg_inverse_supported(n, d, 2)
    X, y = _design(n, d, seed=6000 + n)
    rough = 2.0 * n ** (2.0 / d) / d
    p, t1, t2 = 0.7, 0.3 * rough, 1.5 * rough
    R = (p ** 2 * orc.component_corr(X, [t1] * d) + (1 - p) ** 2 * orc.component_corr(X, [t2] * d)) / (p ** 2 + (1 - p) ** 2)
    Rinv_ref = np.asarray(orc.solve_inverse_exact(R), dtype=np.float64)
    kappa = orc.cond1(R, Rinv_ref)
    assert kappa <= KAPPA_MAX
    theta_t = [math.log(t1), math.log(t2), math.log(p / (1 - p))]
    (r, tm) = _timed(handle, lambda: handle.logpost(X, y, 1.3, api.PRIOR_GV, theta_t))
    assert r["status"] == 0
    assert tm["fused"][1] > 0 and tm["solve"][1] == 0
    A = np.abs(Rinv_ref)
    bound = n * EPS * (A @ np.abs(R) @ A)
    ratio = np.abs(r["R_inv"] - Rinv_ref) / bound
    MAX_RATIO["inverse-lds"] = max(MAX_RATIO.get("inverse-lds", 0.0), float(ratio.max()))
    assert ratio.max() <= INV_C, (n, ratio.max(), kappa)


@pytest.mark.gpu
def test_zz_report_headroom():
    """Largest observed |dev - ref| / (eps cond1 (1 + rho) scale) per route (for the inverse: / (n eps |R^-1||R||R^-1|))."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-16s %.3g" % (k, MAX_RATIO[k]))
