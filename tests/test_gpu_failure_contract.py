"""The failure contract of include/ccgp.h on every route that writes a status: status[b] is 0 or the 1-based index of
the FIRST bad pivot, a failed evaluation is NaN in every output, the other evaluations of the batch are untouched (same
bits as the same call made with only the passing draws), and the return value is the number of failed evaluations.

Inputs: tests/exact_designs.py -- designs whose mixed correlation matrix is 0/1 to the bit in any arithmetic and any
summation order, so a draw fails with a pivot of exactly 0 at a derived index (or has R = I), under both thresholds of
csrc/ccgp_internal.h pivot_tolerance.  tests/test_failure_contract_host.py proves the derived statuses on the host and
that exact_designs.check_contract, the one checker used here, rejects an off-by-one status, an off-by-one-tile status,
the last bad pivot instead of the first, a chunk-relative status, a finite word in a failed draw, a NaN in a passing
neighbour and a wrong return count.

Route of each case: the timing counters (`fused` for the n <= 128 evaluators, `diag` / `update` / `solve` for the blocked
launches, `sweep` for the scheduled sweep) plus route() of tests/test_gpu_gradient_exact.py and the witnesses of
tests/route_witnesses.py; kept-factor against extra-row prediction is the documented rule of include/ccgp.h
(CCGP_OPT_PREDICT_FACTOR, n <= 104, K <= 3), which no counter separates.

Where R = I the passing draws are also held to closed forms (exact_designs.identity_closed_forms; math.fsum, no
long-double reference needed): beta = mean(y), loglik = -(n log(2 pi c) + sum (y - ybar)^2 / c) / 2, a test site on
training point i predicts y_i with variance 0, a site at distance >= 1 from every training point predicts beta with
variance sigma2 (1 + 1/n) -- each within GRAD_TOL_C eps scale (cond1 = 1, no rounding in the exponent, so neither cond1
nor rho enters the band).

Mean mode 1 factorises sigma2 sum(w^2) R + tau2: it runs with tau2 = 0, K = 2 and sigma2 = 2 (exact_designs.mode1_sigma2),
so that the scaling keeps the matrix exact.

Out of scope, because no exact input exists for them: the iso / aniso entry points (ccgp_logpost, ccgp_logpost_batch,
ccgp_grid_marginal) cannot zero ONE dimension's theta, and the Matern and spline families have no exactly representable
kernel values.  Their failure tests stay as they are (tests/test_gpu_parity.py).
"""
import numpy as np
import pytest

import exact_designs as ex
import route_witnesses
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import _timed, route, scheduled

pytestmark = pytest.mark.gpu
C = orc.GRAD_TOL_C
EPS = ex.EPS
S2 = {0: 1.3, 1: ex.mode1_sigma2(2)}          # sigma2 per mean mode (every likelihood case has K = 2)
WITNESS = {(op, r): (n, d, K) for op, r, n, d, K in route_witnesses.WITNESSES[0]}


# ----------------------------------------------------------------------------- plumbing
class _Returned:
    """The C return values of the calls a Handle / MultiHandle makes inside the block (its _chk sees every one).  `calls`:
    how many checked calls the block must make -- a binding method that grew a second one fails here, not silently."""

    def __init__(self, h, calls=1):
        self.h, self.rcs, self.calls = h, [], calls

    def __enter__(self):
        orig = type(self.h)._chk.__get__(self.h)

        def chk(rc):
            self.rcs.append(rc)
            return orig(rc)
        self.h._chk = chk
        return self

    def __exit__(self, *exc):
        del self.h._chk
        if exc[0] is None:
            assert len(self.rcs) == self.calls, "expected %d checked C calls, saw %s" % (self.calls, self.rcs)


def _call(h, fn):
    """(fn(), its C return value, timing counters)"""
    def spied():
        with _Returned(h) as r:
            out = fn()
        return out, r.rcs[0]
    (out, rc), t = _timed(h, spied)
    return out, rc, t


def _contract(h, call, rows, exp):
    """call(rows) -> dict of outputs with "status".  The batch and the passing-only batch through the same call."""
    out, rc, t = _call(h, lambda: call(rows))
    ref, rc0, _ = _call(h, lambda: call(rows[exp == 0]))
    assert rc0 == 0
    ex.check_contract(exp, out, ref, rc)
    return out, t


def _small(t):
    assert t["fused"][1] > 0 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t


def _blocked(t, n):
    assert t["fused"][1] == 0 and t["sweep"][1] == 0 and t["diag"][1] > 0 and (n <= 128 or t["update"][1] > 0), t


class _option:
    def __init__(self, h, opt, value, default):
        self.a = (h, opt, value, default)

    def __enter__(self):
        self.a[0].set_option(self.a[1], self.a[2])

    def __exit__(self, *exc):
        self.a[0].set_option(self.a[1], self.a[3])


class _limit:
    def __init__(self, h, nbytes):
        self.h, self.nbytes = h, nbytes

    def __enter__(self):
        self.h.set_workspace_limit(self.nbytes)

    def __exit__(self, *exc):
        self.h.set_workspace_limit(200 << 30)


# ----------------------------------------------------------------------------- exact values where R = I
def _identity_loglik(out, exp, D, K, mode):
    ll, beta, b_ll, b_beta = ex.identity_closed_forms(D.y, S2[mode], K, mode)
    for b in np.nonzero(exp == 0)[0]:
        assert abs(out["ll"][b] - ll) <= b_ll, (b, out["ll"][b], ll, abs(out["ll"][b] - ll) / b_ll)
        assert abs(out["beta"][b] - beta) <= b_beta, (b, out["beta"][b], beta)


def _identity_predict(out, exp, D, on, K, s2):
    _, beta, _, b_beta = ex.identity_closed_forms(D.y, s2, K, 0)
    n = D.n
    for s in np.nonzero(exp == 0)[0]:
        assert abs(out["beta"][s] - beta) <= b_beta
        for t in range(len(on)):
            mean, var = out["mean"][s, t], out["var"][s, t]
            if on[t] >= 0:
                yi = D.y[on[t]]
                assert abs(mean - yi) <= C * EPS * (abs(yi) + abs(beta)), (s, t, mean, yi)
                assert abs(var) <= C * EPS * s2, (s, t, var)
            else:
                assert abs(mean - beta) <= b_beta, (s, t, mean, beta)
                assert abs(var - s2 * (1.0 + 1.0 / n)) <= C * EPS * s2, (s, t, var)


# ----------------------------------------------------------------------------- ccgp_loglik_batch
def _loglik(h, D, K, mode):
    def call(rows):
        ll, beta, st = h.loglik_batch(D.X, D.y, K, rows, S2[mode], mode, 0.0)
        return dict(ll=ll, beta=beta, status=st)
    return call


def _loglik_case(h, n, seps, mode, tier, zero_sets=None, K=2):
    D = ex.ExactDesign(n, seps)
    rows, exp = D.draws(K, zero_sets or D.mixed())
    out, t = _contract(h, _loglik(h, D, K, mode), rows, exp)
    tier(t)
    _identity_loglik(out, exp, D, K, mode)
    return t


def _repeat(zero_sets, more_than):
    """The batch repeated until it has more than `more_than` draws."""
    return zero_sets * (more_than // len(zero_sets) + 1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", sorted(ex.LOGLIK_REG8))
def test_loglik_register_tier_8x8(handle, n, mode):
    """csrc/small_reg.hip dispatch(): a shared-design likelihood batch runs one wave per matrix on the 8 x 8 grid only when
    `n <= 64 && !wide`, wide = `B <= 64`; the mixed batch is therefore repeated past 64 draws.  (The timing counters cannot
    tell the grids apart: this rests on that predicate.)"""
    D = ex.ExactDesign(n, ex.LOGLIK_REG8[n])
    zs = _repeat(D.mixed(), 64)
    assert len(zs) > 64
    _loglik_case(handle, n, ex.LOGLIK_REG8[n], mode, _small, zs)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", sorted(ex.LOGLIK_REG8) + sorted(ex.LOGLIK_WAVE))
def test_loglik_latency_form_of_small_batches(handle, n, mode):
    """At most 64 draws of n <= 104 (`wide` in dispatch()): four waves per matrix on the 16 x 16 grid, whatever n."""
    seps = {**ex.LOGLIK_REG8, **ex.LOGLIK_WAVE}[n]
    assert len(ex.ExactDesign(n, seps).mixed()) <= 64
    _loglik_case(handle, n, seps, mode, _small)


@pytest.mark.parametrize("grid16", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", sorted(ex.LOGLIK_WAVE))
def test_loglik_one_wave_per_matrix(handle, n, mode, grid16):
    """64 < n <= 104 takes one wave per matrix (8 x 8 grid, up to 13 x 13 blocks per thread) only beyond 64 draws -- dispatch():
    `n > 64 && n <= 104 && !wide && fits8 && !grid16` -- so the batch is the mixed one repeated past 64 draws;
    CCGP_OPT_SMALL_GRID16 = 1 sends the same batch to the 16 x 16 grid."""
    from ccgp_amd import api
    D = ex.ExactDesign(n, ex.LOGLIK_WAVE[n])
    zs = _repeat(D.mixed(), 64)
    assert len(zs) > 64
    with _option(handle, api.OPT_SMALL_GRID16, grid16, 0):
        _loglik_case(handle, n, ex.LOGLIK_WAVE[n], mode, _small, zs)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", sorted(ex.LOGLIK_REG16))
def test_loglik_register_tier_16x16(handle, n, mode):
    _loglik_case(handle, n, ex.LOGLIK_REG16[n], mode, _small)


@pytest.mark.parametrize("fuse_diag", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", sorted(ex.LOGLIK_BLOCKED))
def test_loglik_blocked_launches(handle, n, mode, fuse_diag):
    """Pivots on both sides of every 128-row tile seam; the diagonal block factorised by the update launch's workgroup
    (CCGP_OPT_FUSE_DIAG = 1) or by diag_kernel."""
    from ccgp_amd import api
    D = ex.ExactDesign(n, ex.LOGLIK_BLOCKED[n])
    assert D.same_tile_pairs(D.mixed()) >= 1       # two bad pivots inside one diagonal tile: the first one counts
    with _option(handle, api.OPT_FUSE_DIAG, fuse_diag, 1):
        _loglik_case(handle, n, ex.LOGLIK_BLOCKED[n], mode, lambda t: _blocked(t, n))


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_blocked_in_chunks(handle, mode):
    """The n = 300 batch of 7 under a workspace limit of 4 MB runs in chunks of 2 or 3 (at least three chunks); a failed
    draw sits at a chunk start and at a chunk end for either size, and its status is indexed from the batch."""
    with _limit(handle, 4 << 20):
        t = _loglik_case(handle, 300, ex.LOGLIK_BLOCKED[300], mode, lambda t: _blocked(t, 300), ex.CHUNK_ZERO)
    assert t["solve"][1] >= 3, t


@pytest.mark.parametrize("mode", [0, 1])
def test_loglik_scheduled_sweep(handle, mode):
    """n = 2048, B = 32: the persistent sweep at the default CCGP_OPT_SCHED.  Failures in the second tile, the ninth and at
    the very last pivot, in the first, middle and last draw.  Two calls per mode: the batch of 32, and the passing-only
    batch of 29 that the contract's third clause needs -- which is below 32 draws and therefore runs the per-phase
    launches, so the passing draws' bits are held across the two schedules as well."""
    n, B = ex.SCHED_N, ex.SCHED_B
    assert scheduled(n, B) and len(ex.SCHED_ZERO) == B
    t = _loglik_case(handle, n, ex.SCHED_SEPS, mode, lambda t: None, ex.SCHED_ZERO)
    assert t["sweep"][1] > 0 and t["fused"][1] == 0, t


def test_multi_loglik_status_is_indexed_from_the_batch(handle):
    """ccgp_multi_loglik_batch with one device listed twice: two shards of more than 64 draws each (the 8 x 8 grid, as in
    test_loglik_register_tier_8x8), failed draws in both."""
    from ccgp_amd import api
    D = ex.ExactDesign(64, ex.LOGLIK_REG8[64])
    rows, exp = D.draws(2, _repeat(D.mixed(), 130))
    assert len(exp) // 2 > 64
    half = (len(exp) + 1) // 2
    assert exp[:half].any() and exp[len(exp) // 2:].any() and len(set(exp[exp != 0])) >= 3
    with api.MultiHandle([0, 0]) as m:
        def call(r):
            ll, beta, st = m.loglik_batch(D.X, D.y, 2, r, S2[0])
            return dict(ll=ll, beta=beta, status=st)
        with _Returned(m, 2) as r:
            out = call(rows)
            ref = call(rows[exp == 0])
    assert r.rcs[1] == 0
    ex.check_contract(exp, out, ref, r.rcs[0])
    one = _loglik(handle, D, 2, 0)(rows)
    for k in out:
        np.testing.assert_array_equal(out[k], one[k])


# ----------------------------------------------------------------------------- ccgp_predict_batch
def _predict(h, D, K, Xt, s2):
    def call(rows):
        mean, var, beta, st = h.predict_batch(D.X, D.y, K, rows, Xt, s2)
        return dict(mean=mean, var=var, beta=beta, status=st)
    return call


def _predict_case(h, D, K, m, chunk, tier, zero_sets=None, s2=1.3):
    rows, exp = D.draws(K, zero_sets or D.mixed())
    Xt, on = D.sites(m, chunk)
    out, t = _contract(h, _predict(h, D, K, Xt, s2), rows, exp)
    tier(t)
    assert out["mean"].shape == (len(exp), m)
    _identity_predict(out, exp, D, on, K, s2)
    return out


@pytest.mark.parametrize("n,m,chunk", [(64, 31, 30), (128, 63, 62)])
@pytest.mark.parametrize("K", [1, 2])
def test_predict_extra_row_scheme(handle, n, m, chunk, K):
    """CCGP_OPT_PREDICT_FACTOR = 0: the sites ride through the elimination in chunks of 30 (8 x 8 grid) / 62 (16 x 16); m is
    one more than a chunk."""
    from ccgp_amd import api
    D = ex.ExactDesign(n, ex.predict_seps(n))
    with _option(handle, api.OPT_PREDICT_FACTOR, 0, 1):
        _predict_case(handle, D, K, m, chunk, _small)


# mirrors of csrc/small_layout.h (default build: CCGP_SMALL_EXP_TABLE = 0) and of the plan in csrc/capi.hip predict_run /
# csrc/small_reg.hip launch_small_reg_predict: no counter separates the kept-factor scheme from the extra-row scheme, or
# one chunk of draws from several, so the cases below assert through these what the library is bound to do with them
def _lds_fits(doubles, per_cu=1):
    return 8 * doubles <= 160 * 1024 // per_cu - 64


def _fac_npf(n):
    return (n + 7) // 8 * 8


def _fac_total(n):
    """FacLayout(n): (head, total)."""
    head = 8 + 3 * _fac_npf(n)
    return head, (head + n * (n - 1) // 2 + 7) // 8 * 8


def _reg_lds_doubles8(n, d, K):
    """reg_lds_doubles(8, (n + 7) / 8, 1, false, false, n, d, K): the factorising instance on the 8 x 8 grid."""
    NP = 8 * ((n + 7) // 8)
    per_mat = K * NP + K * d + K + 2 * (NP + 8) + NP + 2 * NP + 8
    return d * n + 4 * per_mat


def sites_supported(n, d, K):
    """small_reg_sites_supported: the kept-factor scheme exists for this shape."""
    if n > 104 or K > 3:
        return False
    npf, nbl = _fac_npf(n), _fac_npf(n) // 8
    solve = _fac_total(n)[0] + 32 * nbl * nbl + 8
    corr = (K * d + 7) // 8 * 8 + 8 + K * npf + K * d * npf + 4 * d * 64
    return _lds_fits(_reg_lds_doubles8(n, d, K)) and _lds_fits(solve, 2) and _lds_fits(corr, 2)


def sites_scratch(n, m):
    """small_reg_sites_scratch: bytes per draw."""
    return 8 * (_fac_total(n)[1] + (m + 63) // 64 * _fac_npf(n) * 64)


def draw_chunk_of_fresh_handle(n, m, S, limit):
    """Draws per pass on a handle without a workspace yet: predict_run grows it to min(want, cap / per * per), cap =
    max(limit / 2, 64 per), and launch_small_reg_predict takes ws_bytes / per draws at a time."""
    per = sites_scratch(n, m)
    cap = max(limit // 2, per * 64)
    return min(S, min(per * S, cap // per * per) // per, 32768)


@pytest.mark.parametrize("reps", [1, 10], ids=["four-wave", "one-wave"])
@pytest.mark.parametrize("n", [9, 64, 104])
@pytest.mark.parametrize("K", [1, 2])
def test_predict_kept_factor_scheme(handle, n, K, reps):
    """Default: one factorisation per draw, then one lane per site in batches of 64; m = 65.  The factor block of a failed
    draw is only written up to the bad pivot: whatever lies behind it must not reach the tables.  The factorisation that
    keeps its factor runs four waves per matrix (16 x 16 grid) up to CCGP_FAC_WIDE_MAX = 64 draws and one wave per matrix
    (8 x 8 grid) beyond (dispatch(): `wide`): the mixed batch of 9 draws is the first form, ten times it the second."""
    D = ex.ExactDesign(n, ex.predict_seps(n))
    assert sites_supported(D.n, D.d, K)
    zs = D.mixed() * reps
    assert (len(zs) > 64) == (reps > 1)
    _predict_case(handle, D, K, 65, 64, _small, zs)


def test_predict_four_components_fall_back_to_extra_rows(handle):
    """K = 4 is outside the kept-factor scheme (K <= 3): the extra-row scheme serves it under the default option."""
    D = ex.ExactDesign(64, ex.predict_seps(64))
    assert not sites_supported(D.n, D.d, 4) and sites_supported(D.n, D.d, 3)
    _predict_case(handle, D, 4, 31, 30, _small)


@pytest.mark.parametrize("chunk", [64, 65])
def test_predict_kept_factor_in_chunks_of_draws(chunk):
    """S = 130 on a fresh handle whose workspace limit holds the factor blocks of `chunk` draws only: chunks of 64, 64 and 2
    draws (the floor of the plan; each factorised in the four-wave form), or of 65 and 65 (the one-wave form), failed
    draws at the end of one chunk and the start of the next.  A fresh handle, because a workspace an earlier test grew
    would hold every draw at once; the chunk itself is asserted through the mirror of the plan above."""
    from ccgp_amd import api
    D = ex.ExactDesign(64, ex.predict_seps(64))
    S, m = 130, 65
    zs = (D.mixed() * 15)[:S]
    zs[chunk - 1], zs[chunk], zs[S - 2], zs[S - 1] = (1,), (2, 0), (), (2,)
    limit = (1 << 20) if chunk == 64 else 2 * chunk * sites_scratch(D.n, m)
    assert sites_supported(D.n, D.d, 2) and draw_chunk_of_fresh_handle(D.n, m, S, limit) == chunk
    h = api.Handle(0)
    try:
        h.set_workspace_limit(limit)
        _predict_case(h, D, 2, m, 64, _small, zs)
    finally:
        h.close()


@pytest.mark.parametrize("m", [1, 129])
def test_predict_blocked(handle, m):
    """n = 129: the cross-correlation rows ride as extra tile rows of the sweep, 128 sites per tile row."""
    D = ex.ExactDesign(129, ex.predict_seps(129))
    _predict_case(handle, D, 2, m, 128, lambda t: _blocked(t, 129))


def test_predict_blocked_below_129(handle):
    """The n <= 128 shape whose prediction takes the sweep (tests/route_witnesses.py): d = 63 = 2 base + 2 separator + 59
    padding dimensions."""
    n, d, K = WITNESS[("predict", "b")]
    D = ex.ExactDesign(n, (2, n), d - 4)
    assert (D.n, D.d, K) == (108, 63, 1)
    _predict_case(handle, D, K, 3, 128, lambda t: _blocked(t, n))


# ----------------------------------------------------------------------------- factor sets
@pytest.mark.parametrize("n", [64, 257])
def test_factor_set(handle, n):
    """ccgp_factor_batch reports status and count; the tables and summaries served from the set keep the contract; the set
    can still be freed.  n = 64: the set keeps the draws only (fused); n = 257: the kept tiles of the sweep."""
    from ccgp_amd import api
    D = ex.ExactDesign(n, ex.predict_seps(n))
    rows, exp = D.draws(2, D.mixed())
    Xt, on = D.sites(65, 64)
    probs = [0.05, 0.5, 0.95]

    def run(r):
        with _Returned(handle, 3) as ret:
            fs = handle.factor_batch(D.X, D.y, 2, r, 1.3)
            mean, var = fs.predict(Xt)
            summ = fs.summary(Xt, probs, y_at=np.zeros(65))
        nbytes = fs.nbytes
        assert api.lib().ccgp_factorset_free(handle._h, fs._fs) == 0
        fs._fs = None
        assert nbytes > 0 and ret.rcs[1] == 0
        table = np.column_stack([summ[k] for k in ("y_hat", "pred_var", "quant", "cdf_at", "quantiles")])
        return dict(ll=fs.loglik, beta=fs.beta, mean=mean, var=var, status=fs.status), ret.rcs[0], ret.rcs[2], table

    out, rc, rc_summary, table = run(rows)
    ref, rc0, rc0_summary, table0 = run(rows[exp == 0])
    assert rc0 == 0 and rc0_summary == 0 and rc_summary == np.count_nonzero(exp)
    ex.check_contract(exp, out, ref, rc)
    _identity_predict(out, exp, D, on, 2, 1.3)
    # summary_valid_kernel compacts the passing draws in their own order (one workgroup): the same sums, the same bits
    assert not np.isnan(table0).any() and np.array_equal(table.view(np.uint64), table0.view(np.uint64))


# ----------------------------------------------------------------------------- ccgp_predict_summary
@pytest.mark.parametrize("n", [64, 129])
def test_predict_summary_leaves_failed_draws_out(handle, n):
    """The summary of a batch with failed draws has the bits of the summary without them: csrc/summary.hip's
    summary_valid_kernel is ONE workgroup that writes the indices of the passing draws in ascending order (t.idx, t.count),
    so every sum runs over the same numbers in the same order.  A batch whose draws all fail is NaN throughout and returns S."""
    D = ex.ExactDesign(n, ex.predict_seps(n))
    rows, exp = D.draws(2, D.mixed())
    Xt, _ = D.sites(65, 64)
    probs, y_at = [0.05, 0.5, 0.95], np.linspace(-1.0, 2.0, 65)
    keys = ("y_hat", "pred_var", "quant", "cdf_at", "quantiles")
    got = handle.predict_summary(D.X, D.y, 2, rows, Xt, 1.3, probs, y_at)
    ref = handle.predict_summary(D.X, D.y, 2, rows[exp == 0], Xt, 1.3, probs, y_at)
    assert ref["n_failed"] == 0
    ex.check_contract(exp, dict(beta=got["beta"], status=got["status"]), dict(beta=ref["beta"], status=ref["status"]),
                      got["n_failed"])
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert not np.isnan(b).any() and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                        np.ascontiguousarray(b).view(np.uint64)), k
    bad_rows = rows[exp != 0]
    none = handle.predict_summary(D.X, D.y, 2, bad_rows, Xt, 1.3, probs, y_at)
    assert none["n_failed"] == len(bad_rows) and np.array_equal(none["status"], exp[exp != 0])
    assert np.isnan(none["beta"]).all() and all(np.isnan(np.asarray(none[k])).all() for k in keys)


# ----------------------------------------------------------------------------- ccgp_loglik_grad_batch
def _grad(h, D, K, s2):
    def call(rows):
        ll, beta, grad, st = h.loglik_grad_batch(D.X, D.y, K, rows, s2)
        return dict(ll=ll, beta=beta, grad=grad, status=st)
    return call


@pytest.mark.parametrize("n,n_pad,K,want", [(17, 0, 2, "reg"), (97, 52, 8, "lds"), (257, 0, 2, "blocked")],
                         ids=["register", "lds", "blocked"])
def test_gradient(handle, n, n_pad, K, want):
    """Register instance (n = 17, d = 4), the LDS evaluator's witness (n = 97, d = 56, K = 8 equal weights) and the blocked
    contraction (n = 257): the whole gradient row of a failed draw is NaN."""
    D = ex.ExactDesign(n, ex.GRAD_BLOCKED_SEPS if want == "blocked" else (2, n), n_pad)
    assert want != "blocked" or D.same_tile_pairs(D.mixed()) >= 1
    assert route(D.n, D.d, K) == want
    if want == "lds":
        assert WITNESS[("grad", "l")] == (D.n, D.d, K)
    rows, exp = D.draws(K, D.mixed())
    out, t = _contract(handle, _grad(handle, D, K, 1.3), rows, exp)
    if want == "blocked":
        _blocked(t, n)
        assert t["solve"][1] > 0
    else:
        _small(t)
        assert t["solve"][1] == 0
    assert out["grad"].shape == (len(exp), K + K * D.d)
    ll, beta, b_ll, b_beta = ex.identity_closed_forms(D.y, 1.3, K, 0)
    for b in np.nonzero(exp == 0)[0]:
        assert abs(out["ll"][b] - ll) <= b_ll and abs(out["beta"][b] - beta) <= b_beta


# ----------------------------------------------------------------------------- entropy criteria: designs differ, row shared
def test_mixed_logdet_designs(handle):
    designs, K, row, exp = ex.duplicate_designs()

    def call(ds):
        ld, st = handle.mixed_logdet_designs(ds, K, row)
        return dict(logdet=ld, status=st)
    out, t = _contract(handle, call, designs, exp)
    _small(t)
    assert out["logdet"][1] == 0.0                     # log det I


@pytest.mark.parametrize("n_fixed", [0, 5])
def test_mixed_logdet_grad_designs(handle, n_fixed):
    """n_fixed = 5: the duplicate of row 2 lies inside the fixed rows, which get no gradient but still enter R."""
    designs, K, row, exp = ex.duplicate_designs()

    def call(ds):
        ld, g, st = handle.mixed_logdet_grad_designs(ds, K, row, n_fixed)
        return dict(logdet=ld, grad=g, status=st)
    out, t = _contract(handle, call, designs, exp)
    _small(t)
    assert out["grad"].shape == (5, 20 - n_fixed, 2)
    assert out["logdet"][1] == 0.0 and not out["grad"][1].any()       # R = I: R^-1 has no off-diagonal entry
