"""The marginal likelihood (ccgp_loglik_batch in mean mode 1, cond.like HX:561-572) and the hyperprior grid built on it
(ccgp_grid_marginal, choose.hyperpars HX:584-595 / ADV:588-599: BASELINE configs 2 - 4) against an exact reference, on every
device route that computes them -- and, beside it, mode 0 through ccgp_loglik_batch, whose plain (identity-row-free)
instances the gradient module never runs.

Mode 1.  Sigma = Sigma0 + tau2 11', Sigma0 = sigma2 sum_c w_c^2 R_c, mean 0.  With alpha = Sigma^-1 y and M = (alpha alpha' -
Sigma^-1) / 2 the value moves by tr(M dSigma), so one relative fp64 rounding of every entry of Sigma moves it by at most eps
sum_ab |M_ab| |Sigma_ab|; errors of the kernel values (polynomial exp, the rounding ~eps rho of the expanded exponent, rho =
oracle.expanded_form_magnitude) touch Sigma0 only.  Every checked draw must satisfy

    |ll_dev - ll_ref| <= C unit,   unit = eps (sum |M| |Sigma| + rho sum |M| |Sigma0|),   C = oracle.MARGINAL_TOL_C,

ll_ref in long double (oracle.marginal_parts, hand-written Cholesky, eps 1.1e-19; n <= 520 as in the gradient module).  There
is no condition number in the band -- the gradient module's eps cond1 scale is vacuous here, cond1(Sigma) and |alpha|'|Sigma|
|alpha| both grow with tau2 n -- but first order only holds while eps cond1(Sigma) is small: every checked draw asserts
cond1(Sigma) <= oracle.MARGINAL_COND_MAX = 4e9 from the long-double inverse (the draws are made with conditioned_row's
kappa_max = KAPPA_R so that the reference alone stays inside; none is skipped).

Why this C.  tests/test_oracle.py evaluates the fp64 LAPACK likelihood with the exponent in the scripts' expanded form -- a
correct fp64 implementation -- on mode1_draws() below, this module's own case list, on every run: its largest |ll - ll_ref| /
unit is oracle.MARGINAL_LAPACK_MAX (the figure is recorded there).  C is 32 times that, for the device's own summation
orders, a 2-ulp exp and a Cholesky backward error growing like sqrt(n) up to n = 520, rounded up to a power of two and capped
at GRAD_TOL_C = 128.  The same host test shows that the band rejects, by at least 4 C, tau2 added before the scaling, sigma2
without sum w^2, tau for tau^2, tau2 missing on one 64 x 64 tile, a dropped or doubled tile of Sigma0, an unsquared weight and
a padded row leaking into row n - 1.  Nothing in the band comes from a device run; the device's measured share of C is
printed by test_zz_report_headroom and recorded in the README's tests row: at most 0.085 units on an MI355X (the 8 x 8
grid at n = 5), 2 % of C = 4; 0.022 of a grid node's band.  Mode 1 returns beta = 0: asserted exactly.

Mode 0 is held to the yardstick of tests/test_gpu_gradient_exact.py unchanged (check_loglik_beta: GRAD_TOL_C eps cond1 (1 +
rho) times the cancellation-free sizes of oracle.loglik_beta_scales).

Route of each case: the timing counters (`fused` for the n <= 128 evaluator, `diag` / `update` for the blocked launches,
`sweep` for the scheduled sweep, `solve` once per chunk) as in tests/test_gpu_failure_contract.py.  Inside the register
evaluator the counters cannot tell the grids apart; csrc/small_reg.hip dispatch() decides by n and by the batch: up to 64
draws of n <= 104 run four waves per matrix on the 16 x 16 grid (`wide`), more than 64 run one wave per matrix on the 8 x 8
grid (or the 16 x 16 grid under CCGP_OPT_SMALL_GRID16), n > 104 always the 16 x 16 grid.  Each n <= 104 case therefore runs
its two draws alone AND repeated to 66.  tests/route_witnesses.py's (loglik, blocked) witness is n = 129, d = 1, K = 1: no
Gaussian likelihood shape below 129 takes the sweep (asserted), so that witness is the first blocked case.

The grid.  Every out_logs[g, j] is compared with the long-double value at the library's own host nodes (api.halton_base2,
api.qigamma) within C unit + Q sum_j |d ll / d row_j| |row_j|, Q = oracle.GRID_NODE_Q = 2e-13: the relative accuracy
tests/test_special.py requires of the host quantile, granted to the device instance of the same source and no more; the
derivative is oracle.grad_from_parts on the mode-1 parts.  Every out[g] is compared with oracle.logmeanexp_exact of the
device's own out_logs row, which isolates row_logmeanexp_kernel: take_log = 1: |d| <= eps (2 |out| + log2 N + 6) -- one
rounding each for mx + log(.) and the division, a 2-ulp exp per term, a tree of depth log2 256 plus N / 256 serial adds;
take_log = 0: the same bound on the logarithm is a relative bound on the value, |d| <= eps (2 |log v| + log2 N + 6) v, and
where v is below the smallest normal double the device result must be 0 or subnormal, not NaN.

Left out: a failing node.  ccgp_grid_marginal's rows are (u_j, 1 - u_j, b / qgamma(.)): sum w^2 is a power of two at u = 1/2
only, no theta can be zeroed, and a design with two identical rows gives a second pivot of exactly 0 only where sigma2 sum w^2
+ tau^2 times its own reciprocal rounds to 1 -- at every other node the pivot is rounding noise of either sign.  Such an input
fails by rounding only, which tests/test_gpu_failure_contract.py's docstring already rules out for this entry point; its
NaN handling stays with tests/test_gpu_parity.py.
"""
import functools
import math

import numpy as np
import pytest

import route_witnesses
from conftest import load_maximin
from oracle import ccgp_oracle as orc
from test_gpu_failure_contract import _lds_fits, _reg_lds_doubles8
from test_gpu_gradient_exact import _bits, _design, _timed, check_loglik_beta

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
C = orc.MARGINAL_TOL_C
KAPPA_R = 1e3                       # conditioned_row's bound on cond1(R): keeps cond1(Sigma) <= MARGINAL_COND_MAX at (1, 25)
KAPPA_R_PAIRS = 1e2                 # ... and at every pair of PAIRS (sigma2 = 0.05 under tau2 = 1e4 multiplies it by ~1e7)
MAX_RATIO = {}                      # route -> largest |ll_dev - ll_ref| / unit seen (mode 0: / (eps cond1 (1 + rho) size))
S2_TAU2 = (1.0, 25.0)               # the pair of every case that is not about the pair
PAIRS = [(1.0, 0.0), (1.0, 2500.0), (0.05, 1e4), (30.0, 2500.0)]       # tau = 50 and tau = 100 are what the scripts use
TINY_TAU2 = [1e-300, 5e-324]

# (n, d, K): d from 1 to 9, K in {1, 2, 3, 8}
REG8_CASES = [(2, 1, 1), (5, 4, 2), (8, 9, 3), (9, 2, 8), (63, 7, 2), (64, 3, 3)]
WAVE_CASES = [(65, 5, 1), (72, 8, 8), (104, 6, 2)]
REG16_CASES = [(105, 1, 3), (127, 9, 2), (128, 4, 8)]
WITNESS = next((n, d, K) for op, r, n, d, K in route_witnesses.WITNESSES[0] if (op, r) == ("loglik", "b"))
BLOCKED_CASES = [WITNESS, (129, 3, 2), (191, 6, 8), (192, 8, 1), (193, 9, 2), (255, 2, 8), (256, 4, 1), (257, 5, 2),
                 (383, 3, 8), (385, 7, 1), (520, 6, 2)]
PAIR_SHAPES = [(14, 2, 2), (100, 3, 2), (128, 5, 3), (257, 4, 2)]
TINY_SHAPES = [(64, 3, 2), (257, 4, 2)]
SCHED_CASE = (385, 4, 2, 3)         # n, d, K, B
CHUNK_CASE = (257, 3, 2, 7)
POSITION_CASES = [(65, 4, 3), (257, 6, 2)]


# ----------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def make_case(n, d, K, B=2):
    """(X, y, rows[B]) of one shape: seeded, B conditioned draws with cond1(R) <= KAPPA_R (the shapes of PAIR_SHAPES:
    KAPPA_R_PAIRS)."""
    X, y = _design(n, d, seed=7000 + 31 * n + d)
    rng = np.random.default_rng(9000 + 64 * n + 8 * d + K)
    kappa_r = KAPPA_R_PAIRS if (n, d, K) in PAIR_SHAPES else KAPPA_R
    rows = np.stack([orc.conditioned_row(X, K, d, rng, kappa_r)[0] for _ in range(B)])
    rows.setflags(write=False)
    return X, y, rows


def mode1_draws():
    """Every (n, d, K, B, b, sigma2, tau2) whose mode-1 value this module holds to the band: the list tests/test_oracle.py
    measures the fp64 LAPACK evaluation on."""
    out = []
    for n, d, K in REG8_CASES + WAVE_CASES + REG16_CASES + BLOCKED_CASES:
        out += [(n, d, K, 2, b) + S2_TAU2 for b in range(2)]
    for n, d, K in PAIR_SHAPES:
        out += [(n, d, K, 2, b, s2, tau2) for s2, tau2 in PAIRS for b in range(2)]
    for n, d, K in TINY_SHAPES:
        out += [(n, d, K, 2, b, 1.0, tau2) for tau2 in [0.0] + TINY_TAU2 for b in range(2)]
    for n, d, K, B in (SCHED_CASE, CHUNK_CASE):
        out += [(n, d, K, B, b) + S2_TAU2 for b in range(B)]
    return out


@functools.lru_cache(maxsize=None)
def mode1_reference(n, d, K, B, b, s2, tau2):
    """(ll_ref, unit, cond1(Sigma)) of one draw in long double; computed once and shared."""
    X, y, rows = make_case(n, d, K, B)
    parts = orc.marginal_parts(X, y, rows[b], K, d, s2, tau2, np.longdouble)
    return float(parts["loglik"]), orc.marginal_unit(parts, X, rows[b], K, d), orc.cond1(parts["Sigma"], parts["Sinv"])


def check_mode1(case, b, s2, tau2, ll, beta, tag):
    ll_ref, unit, kappa = mode1_reference(*case, b, s2, tau2)
    assert kappa <= orc.MARGINAL_COND_MAX, (tag, case, b, kappa)
    assert beta == 0.0, (tag, case, b, beta)
    ratio = abs(ll - ll_ref) / unit
    print("%s %s draw %d (%g, %g): ll %.17g ref %.17g  %.3g units (cond1 %.3g)" % (tag, case, b, s2, tau2, ll, ll_ref, ratio, kappa))
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), ratio)
    assert ratio <= C, (tag, case, b, ll, ll_ref, ratio)


@functools.lru_cache(maxsize=None)
def mode0_reference(n, d, K, B, b, s2):
    """(ll_ref, beta_ref, unit_ll, unit_beta, cond1) of one draw in long double: what check_draw of the gradient module forms."""
    X, y, rows = make_case(n, d, K, B)
    parts = orc.loglik_grad_parts(X, y, rows[b], K, d, s2, np.longdouble)
    kappa = orc.cond1(parts["Sigma"], parts["Sinv"])
    s_ll, s_beta = orc.loglik_beta_scales(parts, y)
    unit = EPS * kappa * (1.0 + orc.expanded_form_magnitude(X, rows[b], K, d))
    return float(parts["loglik"]), float(parts["beta"]), unit * s_ll, unit * s_beta, kappa


def check_mode0(case, b, s2, ll, beta, tag):
    ll_ref, beta_ref, unit_ll, unit_beta, kappa = mode0_reference(*case, b, s2)
    assert kappa <= 1e8, (tag, case, kappa)
    r = check_loglik_beta(ll_ref, beta_ref, unit_ll, unit_beta, ll, beta, tag)
    MAX_RATIO[tag + "/mode0"] = max(MAX_RATIO.get(tag + "/mode0", 0.0), *r)


def _small(t):
    assert t["fused"][1] > 0 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t


def _blocked(t, n):
    assert t["fused"][1] == 0 and t["sweep"][1] == 0 and t["diag"][1] > 0 and (n <= 128 or t["update"][1] > 0), t


def _run_both_modes(handle, case, reps, tier, tag, pair=S2_TAU2):
    """The two draws of `case`, repeated `reps` times in one batch, in mode 1 and mode 0; every copy has the bits of the first."""
    n, d, K = case
    X, y, rows = make_case(n, d, K)
    batch = np.stack([rows[i % 2] for i in range(2 * reps)])
    s2, tau2 = pair
    for mode in (1, 0):
        (ll, beta, st), t = _timed(handle, lambda: handle.loglik_batch(X, y, K, batch, s2, mode, tau2))
        tier(t)
        assert not st.any(), (case, mode, st)
        for b in range(2):
            assert (_bits(ll[b::2]) == _bits(ll[b])).all() and (_bits(beta[b::2]) == _bits(beta[b])).all(), (case, mode, b)
            if mode == 1:
                check_mode1((n, d, K, 2), b, s2, tau2, ll[b], beta[b], tag)
            else:
                check_mode0((n, d, K, 2), b, s2, ll[b], beta[b], tag)


# ----------------------------------------------------------------------------- register evaluator
@pytest.mark.parametrize("reps", [1, 33], ids=["four-wave", "one-wave"])
@pytest.mark.parametrize("n,d,K", REG8_CASES)
def test_register_8x8_grid(handle, n, d, K, reps):
    """n <= 64: more than 64 draws run one wave per matrix on the 8 x 8 grid, the two draws alone the latency form."""
    _run_both_modes(handle, (n, d, K), reps, _small, "reg8" if reps > 1 else "reg-wide")


@pytest.mark.parametrize("grid16", [0, 1])
@pytest.mark.parametrize("reps", [1, 33], ids=["four-wave", "one-wave"])
@pytest.mark.parametrize("n,d,K", WAVE_CASES)
def test_register_one_wave_per_matrix(handle, n, d, K, reps, grid16):
    """64 < n <= 104 beyond 64 draws: one wave per matrix with up to 13 x 13 blocks per thread; CCGP_OPT_SMALL_GRID16 = 1
    sends the same batch to the 16 x 16 grid."""
    from ccgp_amd import api
    assert _lds_fits(_reg_lds_doubles8(n, d, K))
    handle.set_option(api.OPT_SMALL_GRID16, grid16)
    try:
        _run_both_modes(handle, (n, d, K), reps, _small, "reg-wide" if reps == 1 else "reg16-option" if grid16 else "wave")
    finally:
        handle.set_option(api.OPT_SMALL_GRID16, 0)


@pytest.mark.parametrize("n,d,K", REG16_CASES)
def test_register_16x16_grid(handle, n, d, K):
    _run_both_modes(handle, (n, d, K), 1, _small, "reg16")


# ----------------------------------------------------------------------------- blocked launches
@pytest.mark.parametrize("n,d,K", BLOCKED_CASES)
def test_blocked_launches(handle, n, d, K):
    """Around the 128-row tiles (129, 255 - 257, 383, 385), the 64-row halves (191 - 193) and n = 520; the first case is the
    (loglik, blocked) witness of tests/route_witnesses.py."""
    _run_both_modes(handle, (n, d, K), 1, lambda t: _blocked(t, n), "blocked")


# ----------------------------------------------------------------------------- scheduled sweep
def test_scheduled_sweep_same_band_same_bits(handle):
    """CCGP_OPT_SCHED = 1 and 2 force the persistent sweep at n = 385, B = 3: within the band, and the bits of the launches."""
    from ccgp_amd import api
    n, d, K, B = SCHED_CASE
    X, y, rows = make_case(n, d, K, B)
    s2, tau2 = S2_TAU2
    got = {}
    try:
        for sched in (0, 1, 2):
            handle.set_option(api.OPT_SCHED, sched)
            got[sched], t = _timed(handle, lambda: handle.loglik_batch(X, y, K, rows, s2, 1, tau2))
            assert (t["sweep"][1] > 0) == (sched != 0) and t["fused"][1] == 0, (sched, t)
    finally:
        handle.set_option(api.OPT_SCHED, 3)
    for sched in (0, 1, 2):
        ll, beta, st = got[sched]
        assert not st.any()
        for b in range(B):
            check_mode1((n, d, K, B), b, s2, tau2, ll[b], beta[b], "sched%d" % sched)
        assert np.array_equal(_bits(ll), _bits(got[0][0])) and np.array_equal(_bits(beta), _bits(got[0][1])), sched


# ----------------------------------------------------------------------------- chunks, batch position
class _limit:
    def __init__(self, h, nbytes):
        self.h, self.nbytes = h, nbytes

    def __enter__(self):
        self.h.set_workspace_limit(self.nbytes)

    def __exit__(self, *exc):
        self.h.set_workspace_limit(200 << 30)


def test_chunked_batch(handle):
    """A workspace limit of 8 MB holds three n = 257 matrices (384 x 512 + 3 x 128 x 128 doubles each, and the design): the
    batch of 7 runs in at least three chunks; every draw within the band."""
    n, d, K, B = CHUNK_CASE
    X, y, rows = make_case(n, d, K, B)
    s2, tau2 = S2_TAU2
    with _limit(handle, 8 << 20):
        (ll, beta, st), t = _timed(handle, lambda: handle.loglik_batch(X, y, K, rows, s2, 1, tau2))
    _blocked(t, n)
    assert t["solve"][1] >= 3 and not st.any(), t
    for b in range(B):
        check_mode1((n, d, K, B), b, s2, tau2, ll[b], beta[b], "blocked-chunks")


@pytest.mark.parametrize("n,d,K", POSITION_CASES)
def test_bits_do_not_depend_on_batch_position(handle, n, d, K):
    """One probe draw at positions 0, middle and last of batches of 1, 9 and 66 (n = 65), and of 7 in chunks (n = 257), mode 1:
    the same bits."""
    X, y, rows = make_case(n, d, K, 3)
    probe, fill = rows[0], rows[1:]
    s2, tau2 = S2_TAU2
    ref = handle.loglik_batch(X, y, K, probe[None], s2, 1, tau2)
    assert ref[2][0] == 0 and np.isfinite(ref[0][0]) and ref[1][0] == 0.0
    for B in ((1, 9, 66) if n <= 128 else (7,)):
        for pos in sorted({0, B // 2, B - 1}):
            batch = np.stack([fill[i % 2] for i in range(B)])
            batch[pos] = probe
            if n <= 128:
                ll, beta, st = handle.loglik_batch(X, y, K, batch, s2, 1, tau2)
            else:
                with _limit(handle, 8 << 20):
                    (ll, beta, st), t = _timed(handle, lambda: handle.loglik_batch(X, y, K, batch, s2, 1, tau2))
                assert t["solve"][1] >= 3, t
            assert st[pos] == 0 and _bits(ll[pos]) == _bits(ref[0][0]) and _bits(beta[pos]) == _bits(ref[1][0]), (B, pos)


# ----------------------------------------------------------------------------- (sigma2, tau2) pairs
@pytest.mark.parametrize("n,d,K", PAIR_SHAPES)
def test_sigma2_tau2_pairs(handle, n, d, K):
    """tau2 = 0, the scripts' tau = 50 and tau = 100, sigma2 small and large against tau2."""
    tier = _small if n <= 128 else (lambda t: _blocked(t, n))
    for s2, tau2 in PAIRS:
        X, y, rows = make_case(n, d, K)
        (ll, beta, st), t = _timed(handle, lambda: handle.loglik_batch(X, y, K, rows, s2, 1, tau2))
        tier(t)
        assert not st.any()
        for b in range(2):
            check_mode1((n, d, K, 2), b, s2, tau2, ll[b], beta[b], "pairs-small" if n <= 128 else "pairs-blocked")


@pytest.mark.parametrize("n,d,K", TINY_SHAPES)
def test_tiny_and_subnormal_tau2(handle, n, d, K):
    """tau2 = 1e-300 and the smallest subnormal: no NaN, and the value of tau2 = 0 within the band (each is also held to its
    own reference, which differs from tau2 = 0's by far less than a unit)."""
    X, y, rows = make_case(n, d, K)
    for tau2 in [0.0] + TINY_TAU2:
        ll, beta, st = handle.loglik_batch(X, y, K, rows, 1.0, 1, tau2)
        assert not st.any() and not np.isnan(ll).any()
        for b in range(2):
            check_mode1((n, d, K, 2), b, 1.0, tau2, ll[b], beta[b], "tiny-tau2")
            ll0, unit, _ = mode1_reference(n, d, K, 2, b, 1.0, 0.0)
            assert abs(ll[b] - ll0) <= C * unit, (n, tau2, b)


# ----------------------------------------------------------------------------- ccgp_grid_marginal
def _hyper(G, kind, scale):
    """G x 4 rows (a1, b1, a2, b2).  `shared`: shapes from {4, 5} only, a1 = a2 in row 0 and repeated down the rows (two
    distinct shapes in all: the de-duplication maps 2 G slots to 2 table rows); `distinct`: 2 G different shapes.  b: the
    inverse-gamma mean b / (a - 1) is `scale` (theta1) or 4 `scale` (theta2)."""
    H = np.empty((G, 4))
    for g in range(G):
        a1, a2 = (4.0 + (g % 2), 4.0 + ((g + 1) // 2) % 2) if kind == "shared" else (3.0 + g, 3.5 + g)
        H[g] = [a1, (a1 - 1.0) * scale * (1.0 + 0.1 * g), a2, (a2 - 1.0) * 4.0 * scale * (1.0 + 0.05 * g)]
    return H


def _grid_design(n, d, y_scale):
    if n == 14:
        D = load_maximin(14)
        y = np.array([orc.test_function_2d(a, b, 3) for a, b in D])
    else:
        D, y = _design(n, d, seed=8000 + n)
    return D, y * y_scale


# (n, d, aniso_lambda, tau, sigma2, G, N, hyper kind, y scale)
GRID_CASES = [(14, 2, -1.0, 50.0, 30.0, 5, 300, "shared", 1.0), (14, 2, -1.0, 100.0, 30.0, 3, 256, "distinct", 1.0),
              (14, 2, -1.0, 50.0, 30.0, 1, 1, "distinct", 1.0), (14, 2, -1.0, 100.0, 30.0, 1, 37, "shared", 1.0),
              (14, 2, -1.0, 50.0, 30.0, 3, 256, "shared", 1e3),
              (14, 2, 0.5, 50.0, 30.0, 3, 300, "distinct", 1.0), (14, 2, 0.5, 100.0, 30.0, 5, 37, "shared", 1.0),
              (21, 3, -1.0, 50.0, 30.0, 3, 37, "shared", 1.0), (21, 3, -1.0, 100.0, 30.0, 5, 256, "distinct", 1.0),
              (130, 3, -1.0, 50.0, 30.0, 3, 37, "shared", 1.0), (130, 3, -1.0, 100.0, 30.0, 1, 37, "distinct", 1.0)]


def grid_inputs(n, d, lam, tau, s2, G, N, kind, y_scale):
    X, y = _grid_design(n, d, y_scale)
    return X, y, _hyper(G, kind, 6.0 * n ** (2.0 / d) / d)


def grid_rows(H, N, d, lam):
    """The G x N parameter rows at the library's own host nodes: (u, 1 - u, theta1 x d, theta2 x d), or the anisotropic row."""
    from ccgp_amd import api
    u = api.halton_base2(N)
    rows = np.empty((H.shape[0], N, 2 + 2 * d))
    for g, (a1, b1, a2, b2) in enumerate(H):
        t1, t2 = api.qigamma(u, a1, b1), api.qigamma(u, a2, b2)
        for j in range(N):
            rows[g, j] = (orc.params_from_aniso(u[j], t1[j], t2[j], lam) if lam >= 0.0 else
                          orc.params_from_iso(u[j], t1[j], t2[j], d))
    return rows


@functools.lru_cache(maxsize=None)
def grid_reference(case):
    """(ll_ref[G, N], C unit[G, N], node term[G, N], largest cond1(Sigma)) in long double at the host nodes."""
    n, d, lam, tau, s2, G, N, kind, y_scale = case
    X, y, H = grid_inputs(*case)
    rows = grid_rows(H, N, d, lam)
    ll, unit, node = np.empty((G, N)), np.empty((G, N)), np.empty((G, N))
    kappa = 0.0
    for g in range(G):
        for j in range(N):
            parts = orc.marginal_parts(X, y, rows[g, j], 2, d, s2, tau * tau, np.longdouble)
            kappa = max(kappa, orc.cond1(parts["Sigma"], parts["Sinv"]))
            grad, _ = orc.grad_from_parts(parts, X, rows[g, j], 2, d, s2)
            ll[g, j] = float(parts["loglik"])
            unit[g, j] = orc.marginal_unit(parts, X, rows[g, j], 2, d)
            node[g, j] = orc.GRID_NODE_Q * float(np.abs(grad.astype(np.float64)) @ np.abs(rows[g, j]))
    return ll, unit, node, kappa


def check_logmeanexp(logs_row, got, take_log):
    """One value of row_logmeanexp_kernel against the long-double log-mean-exp of the same row (module docstring)."""
    N = logs_row.shape[0]
    lme = orc.logmeanexp_exact(logs_row, True)
    allow = EPS * (2.0 * abs(float(lme)) + math.log2(N) + 6.0)
    if take_log:
        assert abs(np.longdouble(got) - lme) <= allow, (got, float(lme), float(abs(np.longdouble(got) - lme)) / allow)
        return
    v = orc.logmeanexp_exact(logs_row, False)
    assert not np.isnan(got)
    if v < np.finfo(np.float64).tiny:
        assert 0.0 <= got < np.finfo(np.float64).tiny, (got, v)
    else:
        assert abs(np.longdouble(got) - v) <= allow * v, (got, float(v), float(abs(np.longdouble(got) - v) / (allow * v)))


@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: "n%d-d%d-lam%g-tau%g-G%d-N%d-%s-y%g" % (c[:4] + c[5:]))
def test_grid_marginal_logs_and_row_means(handle, case):
    n, d, lam, tau, s2, G, N, kind, y_scale = case
    X, y, H = grid_inputs(*case)
    shapes = {a for a in H[:, [0, 2]].ravel()}
    assert len(shapes) == (2 * G if kind == "distinct" else min(2, G))       # G = 1, shared: a1 == a2, one table row
    ll_ref, unit, node, kappa = grid_reference(case)
    assert kappa <= orc.MARGINAL_COND_MAX, kappa
    if y_scale != 1.0:
        assert (ll_ref.max(axis=1) - ll_ref.min(axis=1)).max() > 745.0        # terms underflow in exp(row - mx)
    (vals, arg, logs), t = _timed(handle, lambda: handle.grid_marginal(X, y, s2, H, N, tau, True, lam, want_logs=True))
    (vals0, arg0, logs0), _ = _timed(handle, lambda: handle.grid_marginal(X, y, s2, H, N, tau, False, lam, want_logs=True))
    assert t["cov"][1] > 0
    (_small(t) if n <= 128 else _blocked(t, n))
    assert not np.isnan(logs).any() and np.array_equal(_bits(logs), _bits(logs0))
    band = C * unit + node
    err = np.abs(logs - ll_ref)
    tag = "grid-small" if n <= 128 else "grid-blocked"
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float((err / band).max()))
    MAX_RATIO[tag + "/node-share"] = max(MAX_RATIO.get(tag + "/node-share", 0.0), float((node / band).max()))
    print("%s: largest |d| / band %.3g, largest share of the node term in a band %.3g, cond1 <= %.3g" % (
        tag, (err / band).max(), (node / band).max(), kappa))
    bad = np.argwhere(~(err <= band))
    assert bad.size == 0, (bad[:6].tolist(), (err / band).max())
    for g in range(G):
        check_logmeanexp(logs[g], vals[g], True)
        check_logmeanexp(logs[g], vals0[g], False)
    for v, a in ((vals, arg), (vals0, arg0)):
        assert not np.isnan(v).any() and a == int(np.argmax(v)) and v[a] == v.max() and (v[:a] < v[a]).all()


def test_zz_report_headroom():
    """Largest observed ratio per route: |ll_dev - ll_ref| / unit (mode 1, against MARGINAL_TOL_C), / band (grid), / (eps cond1
    (1 + rho) size) (mode 0, against GRAD_TOL_C)."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-22s %.3g" % (k, MAX_RATIO[k]))
