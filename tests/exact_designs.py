"""Designs whose mixed correlation matrix is exactly 0/1 -- in every arithmetic and every summation order -- so that the
failure contract of include/ccgp.h (status[b] = 0 or the 1-based index of the FIRST bad pivot, NaN for a failed
evaluation, neighbours untouched, return value = number of failures) can be asserted exactly instead of "up to rounding".

Base dimensions (2): row i sits at the integer point (i % W, i // W), W = ceil(sqrt(n)).
Separator dimensions (one per entry of `seps`): separator j is 0 everywhere except a 1 in row p_j, and row p_j's base
coordinates are a copy of those of an earlier row q_j < p_j.  theta_sep_j = 0 makes rows q_j and p_j coincide;
theta_sep_j > 0 keeps them apart.
Padding dimensions (n_pad, all-zero coordinates) only bring d up to the shape a route witness needs.

Draws: component c has theta = 2048 (even c) or 4096 (odd c) on the base and padding dimensions, and 0 or that same
theta on each separator -- the same choice in every component.  Weights are all 1 and K is a power of two, so that
sum w^2 and the normalisation are powers of two.

Why exact: every product and sum of the expanded exponent u_a + u_b - 2 sum_k theta_k x_ak x_bk is an integer below 2^53,
so it is the same number in any order.  Distinct points have exponent <= -2048 -> exp gives exactly 0 (the device's
polynomial and table exp have underflowed to 0 there, as libm has; how far beyond that each stays 0 is what the FAR
magnitudes below are for); coincident points have exponent exactly 0 ->
exactly 1.  R is the identity plus ones at the coincident pairs, to the bit.

So a draw that zeroes the separators J fails with a pivot of exactly 0 at 1-based index min_{j in J} (p_j + 1) -- under
both thresholds of csrc/ccgp_internal.h pivot_tolerance (0 <= n eps and 0 <= 0) -- and a draw that zeroes none has R = I.
The expected status is derived here, never measured.  (Mean mode 1 factorises c R, c = sigma2 sum(w^2): the tests give
it a sigma2 for which c is a power of FOUR (mode1_sigma2), so that the scaling is exact in an L' D L' elimination and in a
Cholesky that takes square roots -- the oracle's and the CPU evaluator's -- alike.)

guard() asserts, on the host, that the fp64 oracle's matrix of each draw has entries in {0, 1} only.

Also here: the one checker of the contract (check_contract) that tests/test_gpu_failure_contract.py applies to every
route and tests/test_failure_contract_host.py feeds fabricated results, and the closed forms of the R = I draws.
"""
import math

import numpy as np

from oracle import ccgp_oracle as orc

EPS = float(np.finfo(np.float64).eps)
THETA = (2048.0, 4096.0)
# Magnitudes beyond exp's range (tests/test_gpu_far_arguments.py, tests/test_far_arguments_host.py): component rates
# (2^k, 2^(k+1)) in place of THETA.  k = 95: the first argument at which the unselected table exp is not 0; 140: the last
# at which the polynomial exp is still right; 200: the polynomial is +-Inf, the table 1e-195; 260: the table is +Inf; 1000:
# the largest that overflows nothing (coordinates <= 18, so u <= 2^1000 * 650 < 2^1010).  The exactness argument below carries
# over: each term of a component's expanded exponent is an integer below 2^53 times ONE power of two, so it is the same
# number in every order.  One magnitude per component: 2^k and 2^11 inside a component would not cancel in u_i + u_i - 2 s_ii.
FAR_K = (95, 140, 200, 260, 1000)
FAR = [(2.0 ** k, 2.0 ** (k + 1)) for k in FAR_K]
SLOW = 2.0 ** -4          # the dyadic rate of the two-scale mix's healthy component: exponents are multiples of 1/16


def mode1_sigma2(K):
    """sigma2 with sigma2 * K (= sigma2 sum w^2 at unit weights) a power of four."""
    return {1: 4.0, 2: 2.0, 4: 1.0, 8: 2.0}[K]


class ExactDesign:
    def __init__(self, n, seps, n_pad=0):
        """seps: the 1-based pivot indices p_j + 1 at which a draw can be made to fail (ascending, each >= 2)."""
        seps = tuple(int(s) for s in seps)
        assert len(seps) >= 1 and all(2 <= s <= n for s in seps) and list(seps) == sorted(set(seps))
        self.n, self.seps, self.n_pad = int(n), seps, int(n_pad)
        self.P = [s - 1 for s in seps]
        self.W = int(math.ceil(math.sqrt(n)))
        self.d = 2 + len(seps) + self.n_pad
        X = np.zeros((n, self.d))
        i = np.arange(n)
        X[:, 0], X[:, 1] = i % self.W, i // self.W
        self.Q, taken = [], set(self.P)
        for j, p in enumerate(self.P):
            q = p - 1
            while q in taken:
                q -= 1
            assert q >= 0, "no earlier row left to copy for separator %d" % j
            taken.add(q)
            self.Q.append(q)
            X[p, :2] = X[q, :2]
            X[p, 2 + j] = 1.0
        self.X = X
        self.y = np.sin(0.7 * i) + 0.3 * np.cos(2.1 * i) + 0.5

    # ---- draws ------------------------------------------------------------------------------------------------------
    def row(self, K, zero=(), theta=THETA):
        """One parameter row (w_1..w_K, theta_1,1..d, ..., theta_K,1..d) that zeroes the separators in `zero`; theta = (a, b):
        the rate of the even and of the odd components (default THETA; FAR: beyond exp's range)."""
        assert K in (1, 2, 4, 8)
        th = np.empty((K, self.d))
        for c in range(K):
            th[c] = theta[c % 2]
            for j in zero:
                th[c, 2 + j] = 0.0
        return np.concatenate([np.ones(K), th.ravel()])

    def expected(self, zero):
        return min((self.seps[j] for j in zero), default=0)

    def draws(self, K, zero_sets, theta=THETA):
        """(rows[B, K + K d], expected status[B]) for a list of separator subsets."""
        rows = np.stack([self.row(K, z, theta) for z in zero_sets])
        return rows, np.array([self.expected(z) for z in zero_sets], dtype=np.int32)

    def mixed(self):
        """Separator subsets of a batch that mixes passing draws, one failing draw per separator, and draws that zero two
        separators (the larger pivot listed first: they must report the smaller index) -- the last with the first and,
        with three separators or more, the two first and the two last, which at n = 129 (pivots 2, 128), at n = 257 with
        GRAD_BLOCKED_SEPS (2, 128) and at n = 300 (257, 300) puts both bad pivots inside ONE 128-row diagonal tile
        (same_tile_pairs); failed draws sit first, in the middle and last."""
        s = len(self.seps)
        assert s >= 2
        pairs = [(s - 1, 0)] + ([(1, 0), (s - 1, s - 2)] if s >= 3 else [])
        return [(0,), ()] + [(j,) for j in range(1, s)] + pairs + [(), (s - 1,)]

    def same_tile_pairs(self, zero_sets, tile=128):
        """How many of the draws have two bad pivots inside one tile of `tile` rows."""
        return sum(1 for z in zero_sets if len(z) == 2 and (self.seps[z[0]] - 1) // tile == (self.seps[z[1]] - 1) // tile)

    def guard(self, K, rows):
        """Host-side guard: the oracle's matrix of every (distinct) draw has entries in {0, 1} only."""
        for row in np.unique(np.asarray(rows), axis=0):
            R = orc.mixed_corr_matrix_general(self.X, *orc.unpack_params(row, K, self.d))
            assert np.isin(R, (0.0, 1.0)).all() and (np.diag(R) == 1.0).all()

    # ---- test sites -------------------------------------------------------------------------------------------------
    def sites(self, m, chunk):
        """m test sites: the table columns 0, chunk - 1, chunk and m - 1 (those below m) coincide with a training point
        each (r = e_i), every other column is at distance >= 1 from every training point (r = 0).  Returns (Xtest[m, d],
        on[m]): on[t] = the training row the site sits on, or -1.  The training rows differ from column to column, so a
        site riding in the wrong slot shows as a wrong y_i."""
        on = np.full(m, -1)
        cols = [t for t in sorted({0, chunk - 1, chunk, m - 1}) if 0 <= t < m]
        for k, t in enumerate(cols):
            on[t] = (5 + 11 * k) % self.n
        assert len(set(on[cols])) == len(cols)
        Xt = np.zeros((m, self.d))
        for t in range(m):
            if on[t] >= 0:
                Xt[t] = self.X[on[t]]
            else:
                Xt[t, 0], Xt[t, 1] = -(1.0 + t), -1.0
        return Xt, on


class TwoScaleDesign:
    """K = 2, unit weights, on the integer lattice of ExactDesign (no separators; n_pad all-zero dimensions): component 0 has a
    far rate (or THETA[0], its stand-in) on every dimension, so R_0 = I to the bit; component 1 has the dyadic rate SLOW =
    2^-4, whose exponents are multiples of 1/16 below 2^53 / 16 and exact in every order.  Base R's matrix is (I + R2) / 2 at
    every far magnitude: non-trivial, eigenvalues in [1/2, (1 + n) / 2].  rows(): the stand-in first, then one row per
    FAR magnitude -- every row of a call on them must equal row 0."""

    def __init__(self, n, n_pad=0):
        self.n, self.d, self.K = int(n), 2 + int(n_pad), 2
        self.W = int(math.ceil(math.sqrt(n)))
        i = np.arange(n)
        self.X = np.zeros((n, self.d))
        self.X[:, 0], self.X[:, 1] = i % self.W, i // self.W
        self.y = np.sin(0.7 * i) + 0.3 * np.cos(2.1 * i) + 0.5

    def row(self, a=THETA[0]):
        return np.concatenate([np.ones(2), np.full(self.d, float(a)), np.full(self.d, SLOW)])

    def rows(self):
        return np.stack([self.row()] + [self.row(a) for a, _ in FAR])

    def sites(self, m):
        """Integer points (exact exponents in both components): even columns on a training point, odd ones off the lattice."""
        Xt = np.zeros((m, self.d))
        on = np.full(m, -1)
        for t in range(m):
            if t % 2 == 0:
                on[t] = (5 + 11 * t) % self.n
                Xt[t] = self.X[on[t]]
            else:
                Xt[t, 0], Xt[t, 1] = -(1.0 + t), -1.0
        return Xt, on

    def matrix(self, a=THETA[0]):
        """The fp64 oracle's normalised mixed matrix of row(a)."""
        return orc.mixed_corr_matrix_general(self.X, *orc.unpack_params(self.row(a), 2, self.d))

    def guard(self):
        """The oracle's matrix is (I + R2) / 2 to the bit at every magnitude, and well conditioned (returns cond1)."""
        R2 = orc.corr_matrix(self.X, np.full(self.d, SLOW))
        want = (np.eye(self.n) + R2) / 2.0
        for a in [THETA[0]] + [a for a, _ in FAR]:
            assert np.array_equal(self.matrix(a), want), a
        return orc.cond1(want, np.linalg.inv(want))


class FarSiteDesign:
    """A far test site on a VALID factor.  One active dimension (the other d - 1 are all-zero padding), K = 1, rate 2^k on
    every dimension, training coordinates i 2^-(k // 2): theta x_i^2 = s i^2 and theta x_i x_j = s i j with s = 1 (k even) or
    2 (k odd), so the training exponents s (i - j)^2 are exact integers and R = exp(-s (i - j)^2) is the same well-conditioned
    matrix at every k.  The sites sit at coordinates -1, -2, ...: their exponent 2^k (t + x_i)^2 >= 2^k under any rounding
    (it is not exact and need not be), so r = 0, mean = beta and var = sigma2 (1 + 1 / 1'R^-1 1).  (-1 and not +1: at the
    stand-ins k = 11, 12 the training coordinates i / 32, i / 64 of n = 108 points reach +1 themselves.)  stand_in(): the
    design of the same parity at k = 11 (rate 2048) or 12 (rate 4096)."""

    def __init__(self, n, k, d=1):
        self.n, self.k, self.d, self.K = int(n), int(k), int(d), 1
        self.theta = 2.0 ** k
        i = np.arange(n)
        self.X = np.zeros((n, d))
        self.X[:, 0] = i * 2.0 ** -(k // 2)
        self.y = np.sin(0.7 * i) + 0.3 * np.cos(2.1 * i) + 0.5
        s = self.theta * self.X[1, 0] ** 2 if n > 1 else 1.0
        assert s in (1.0, 2.0) and np.array_equal(self.theta * self.X[:, 0] ** 2, s * i.astype(np.float64) ** 2)
        self.s = s

    def stand_in(self):
        return FarSiteDesign(self.n, 11 + (self.k + 1) % 2, self.d)

    def row(self):
        return np.concatenate([np.ones(1), np.full(self.d, self.theta)])

    def sites(self, m):
        Xt = np.zeros((m, self.d))
        Xt[:, 0] = -(1.0 + np.arange(m))
        return Xt

    def guard(self):
        """The oracle's training matrix is exp(-s (i - j)^2) to the bit, every cross entry is 0; returns cond1."""
        i = np.arange(self.n, dtype=np.float64)
        want = np.exp(-self.s * (i[:, None] - i[None, :]) ** 2)
        assert np.array_equal(orc.corr_matrix(self.X, np.full(self.d, self.theta)), want)
        for x in self.sites(3):
            assert not orc.corr_vec(x, self.X, np.full(self.d, self.theta)).any()
        return orc.cond1(want, np.linalg.inv(want))


def duplicate_designs(n=20, theta=THETA):
    """B = 5 candidate designs of n points in d = 2 that share one parameter row: TRUE duplicates instead of separators
    (here the designs differ and the row is shared).  Duplicates at 1-based rows 2 / none / n / 2 again (the first design
    twice) / both 2 and n.  Returns (designs[5, n, 2], K, row, expected status)."""
    W, i = int(math.ceil(math.sqrt(n))), np.arange(n)
    base = np.column_stack([i % W, i // W]).astype(np.float64)
    dup2, dupn, both = base.copy(), base.copy(), base.copy()
    dup2[1] = dup2[0]
    dupn[n - 1] = dupn[n - 2]
    both[1], both[n - 1] = both[0], both[n - 2]
    row = np.concatenate([np.ones(2), np.full(2, theta[0]), np.full(2, theta[1])])
    return np.stack([dup2, base, dupn, dup2.copy(), both]), 2, row, np.array([2, 0, n, 2, 2], dtype=np.int32)


# ---- plain references -----------------------------------------------------------------------------------------------
def first_bad_pivot(R, tol=0.0):
    """Plain LDL' without pivoting: 1-based index of the first pivot <= tol, or 0.  A zero multiplier subtracts nothing, so
    the rank-1 update only visits the rows whose multiplier is not zero."""
    A = np.array(R, dtype=np.float64)
    n = A.shape[0]
    for k in range(n):
        piv = A[k, k]
        if not piv > tol:
            return k + 1
        col = A[k + 1:, k]
        nz = k + 1 + np.nonzero(col)[0]
        if nz.size:
            A[np.ix_(nz, nz)] -= np.outer(A[nz, k] / piv, A[nz, k])
    return 0


def identity_closed_forms(y, sigma2, K, mean_mode=0):
    """R = I: (loglik, beta, band_ll, band_beta).  beta = mean(y) (mode 0) or 0 (mode 1), loglik = -(n log(2 pi c) +
    sum (y - beta)^2 / c) / 2 with c = sigma2 sum w^2 = sigma2 K, all sums by math.fsum.  Bands: GRAD_TOL_C eps scale with
    cond1 = 1 and no rho (no rounding in the exponent), scale from oracle.loglik_beta_scales on the closed-form parts."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    c = float(sigma2) * K
    beta = math.fsum(y) / n if mean_mode == 0 else 0.0
    q = math.fsum((float(v) - beta) ** 2 for v in y) / c
    ll = -(n * math.log(2.0 * math.pi * c) + q) / 2.0
    parts = dict(alpha=(y - beta) / c, Sigma=c * np.eye(n), u=np.full(n, 1.0 / n))
    s_ll, s_beta = orc.loglik_beta_scales(parts, y)
    return ll, beta, orc.GRAD_TOL_C * EPS * s_ll, orc.GRAD_TOL_C * EPS * s_beta


# ---- the checker ----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def check_contract(expected_status, outputs, passing_reference, returned=None):
    """The failure contract of a batched entry point.
    expected_status[B]: derived (ExactDesign.draws).
    outputs: dict with "status"[B] and any number of float arrays whose FIRST axis is the draw (ll, beta, the gradient rows,
             the rows of the S x m mean and variance tables, the log det, ...).
    passing_reference: the same dict from the same call made with only the passing draws, in order.
    returned: the C return value (None only where an entry point has none).
      1. status == expected, exactly
      2. every output of a failed draw is NaN everywhere
      3. every output of a passing draw has the bits of the passing-only call
      4. returned == count_nonzero(expected)"""
    exp = np.asarray(expected_status)
    st = np.asarray(outputs["status"])
    assert st.shape == exp.shape, (st.shape, exp.shape)
    assert np.array_equal(st, exp), "status %s, expected %s" % (st.tolist(), exp.tolist())
    ok = exp == 0
    ref_st = np.asarray(passing_reference["status"])
    assert ref_st.shape == (int(ok.sum()),) and not ref_st.any(), "passing-only call: status %s" % ref_st.tolist()
    names = sorted(k for k in outputs if k != "status")
    assert names == sorted(k for k in passing_reference if k != "status")
    for name in names:
        a = np.asarray(outputs[name], dtype=np.float64)
        assert a.shape[0] == exp.size, (name, a.shape)
        a = a.reshape(exp.size, -1)
        r = np.asarray(passing_reference[name], dtype=np.float64).reshape(int(ok.sum()), -1)
        assert np.isnan(a[~ok]).all(), "%s: a failed draw holds a value that is not NaN (draws %s)" % (
            name, np.nonzero(~np.isnan(a).all(axis=1) & ~ok)[0].tolist())
        assert not np.isnan(a[ok]).any(), "%s: NaN in a passing draw (draws %s)" % (
            name, np.nonzero(np.isnan(a).any(axis=1) & ok)[0].tolist())
        assert a[ok].shape == r.shape, (name, a[ok].shape, r.shape)
        same = _bits(a[ok]) == _bits(r)
        assert same.all(), "%s: passing draws %s differ from the passing-only call" % (
            name, np.nonzero(ok)[0][~same.all(axis=1)].tolist())
    if returned is not None:
        assert int(returned) == int(np.count_nonzero(exp)), "returned %d, %d draws must fail" % (returned, np.count_nonzero(exp))


# ---- the cases, shared by the host test (which proves the expected statuses) and the device tests -------------------
# ccgp_loglik_batch: n -> the 1-based pivots a draw can fail at
LOGLIK_REG8 = {9: (2, 9), 64: (8, 9, 64)}                       # register tier, 8 x 8 grid
LOGLIK_WAVE = {65: (64, 65), 104: (64, 65, 104)}                # one wave per matrix (or the 16 x 16 grid by option)
LOGLIK_REG16 = {105: (17, 105), 128: (17, 128)}                 # 16 x 16 grid
LOGLIK_BLOCKED = {129: (2, 128, 129), 300: (128, 129, 256, 257, 300)}
SCHED_N, SCHED_B, SCHED_SEPS = 2048, 32, (129, 1025, 2048)
SCHED_ZERO = [(0,)] + [()] * 15 + [(2,)] + [()] * 14 + [(1,)]   # failures first, in the middle, last
# the n = 300 batch of 7 in chunks of 2 or 3: draws 0, 2, 3, 5, 6 fail -- a failed draw at every chunk start but 4 and at
# every chunk end but 1, whichever of the two chunk sizes the workspace limit gives
CHUNK_ZERO = [(0,), (), (3,), (4, 1), (), (2,), (4,)]


GRAD_BLOCKED_SEPS = (2, 128, 257)                               # n = 257, blocked gradient


def predict_seps(n):
    return (2, n // 2 + 1, n)


def all_designs():
    """(design, K, zero_sets) of every likelihood / prediction / gradient case: what the host test walks."""
    out = []
    for table in (LOGLIK_REG8, LOGLIK_WAVE, LOGLIK_REG16, LOGLIK_BLOCKED):
        for n, seps in table.items():
            D = ExactDesign(n, seps)
            out.append((D, 2, D.mixed()))
    out.append((ExactDesign(300, LOGLIK_BLOCKED[300]), 2, CHUNK_ZERO))
    out.append((ExactDesign(SCHED_N, SCHED_SEPS), 2, SCHED_ZERO))
    for n in (9, 64, 104, 128, 129, 257):
        D = ExactDesign(n, predict_seps(n))
        for K in (1, 2):
            out.append((D, K, D.mixed()))
    out.append((ExactDesign(64, predict_seps(64)), 4, ExactDesign(64, predict_seps(64)).mixed()))
    D = ExactDesign(257, GRAD_BLOCKED_SEPS)
    out.append((D, 2, D.mixed()))
    for n, n_pad, K in ((108, 59, 1), (97, 52, 8), (17, 0, 2)):
        D = ExactDesign(n, (2, n), n_pad)
        out.append((D, K, D.mixed()))
    return out
