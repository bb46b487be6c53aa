"""Exact references and component-wise bands for the Gaussian correlations (CCGP_KERNEL_GAUSS: cov_kernel<0> of csrc/cov.hip
with cov_mix_term and the table-driven exp_cov, out of ccgp_corr_matrix, ccgp_corr_cross, ccgp_mixed_corr_matrix and
ccgp_mixed_corr_cross) and for the literal R.Inv helpers (rinv_terms_kernel and predict_factors_kernel of csrc/capi.hip, out of
ccgp_beta_mle, ccgp_sigma2_mle, ccgp_factors, ccgp_predict_from_factors and ccgp_predict_post).  Shared by
tests/test_gauss_corr_host.py (the kernels' arithmetic restated in numpy, no GPU) and by tests/test_gpu_gauss_corr_exact.py and
tests/test_gpu_rinv_helpers_exact.py (every entry out of the C ABI).  Nothing in a band comes from a device run.

Correlations
  Reference.  mpmath at DPS = 40 digits on the fp64 inputs as exact rationals: coordinates and rates become integers over a common
  power of two, so the argument sum_k theta_ck (a_ik - b_jk)^2 of every component is an exact integer ratio, and the entry is
  the DIRECT form sum_c w_c^2 exp(-arg_c) / sum_c w_c^2 -- not the device's expanded one, as in oracle/mp_check.py.

  Band, per entry, with u = 2^-53 and per component c:
      M_c     = sum_k theta_ck (|a_ik| + |b_jk|)^2     what the expanded form u_i + u_j - 2 s rounds against
      delta_c = 2 (d + 4) u M_c                        d + 1 roundings in the dot product (x_ik theta_ck, then d fused
                                                       multiply-adds), up to d + 2 in u_i and in u_j, each against its own
                                                       share of M_c, and 2 in fma(-2, s, u_i + u_j): (d + 3) u M_c, doubled
      band    = sum_c w_c^2 r_c (expm1(delta_c) + 4 u) / sum w^2 + (2 K + 4) u |ref|     (+ 2 quanta where ref < 2.3e-308)
  4 u is exp_cov's 2 ulp (tests/test_gpu_parity.py::test_device_exp_is_within_two_ulp_down_to_underflow); (2 K + 4) u covers w_c^2,
  their sum, its reciprocal, the K fused multiply-adds and the last product.  Where the design is dyadic and the rates are
  powers of two (the tile cases) every operation of the expanded distance is exact and delta_c is dropped: a few ulp remain.
  Two quanta on a subnormal reference: exp_cov's ldexp rounds once (half a quantum), w_c^2 e_c + acc rounds once per live
  component and the product with 1 / sum w^2 once more; with one live component that is ((w_c^2 + 1) / (2 sum w^2) + 1/2)
  quanta, 1.5 for the weights used here.

R.Inv helpers, with A = R.Inv as given (symmetric or not), e = fl(y - beta), c_j = sum_i |A_ij| and the kernels' orders (four
partial sums per row striding the columns, four lanes per column striding the rows, lane accumulators over 64-row passes, a
6-level shuffle tree and a 4-wave combine):
      mean.factor_i   (n/4 + 8) u sum_j |A_ij| (|y_j| + |beta|)
      colsum_j        (n/4 + 6) u c_j
      1'Ay            (n/4 + n/64 + 18) u sum_j |y_j| c_j                 (colsum's band carried through, + n/64 + 12 for the sum)
      sum(A)          (n/4 + n/64 + 18) u sum_j c_j                       = var.factor2
      e'Ae            (n/4 + n/64 + 20) u sum_i (|y_i| + |beta|) sum_j |A_ij| (|y_j| + |beta|)
      beta = a0 / a1  (D a0 + |beta| D a1) / |a1| + 2 u |beta|
      sigma2 = a2 / n D a2 / n + 2 u |sigma2|
      mean_t          (n/64 + 12) u sum_i |mean.factor_i r_ti| + 2 u |beta|
      var_t           sigma2 (D q + 2 |u_t| D s1 / v2 + 4 u (1 + |q| + u_t^2 / v2)),   u_t = 1 - s1,
                      D q = (n/4 + n/64 + 18) u |r_t|' |A| |r_t|,   D s1 = (n/64 + 10) u sum_i |v1_i r_ti|
  The variance band is absolute: near a training point, where 1 - q + u^2 / v2 cancels, the device is judged against what
  the sums can carry, not against a floor.  References: mpmath (exactly rounded dot products, mp.fdot) on the fp64 R.Inv, y, r,
  beta, mean.factor, v1 and v2 exactly as passed; no inverse is formed.
"""
import functools
import math

import mpmath as mp
import numpy as np

import family_exact as fx
from family_exact import Table, dyadic_grid, half_grid, near_coincident_design, worst_ratio  # noqa: F401  (re-exported)

DPS = 40
U = 2.0 ** -53
QUANTUM, TINY, MIX_W = fx.QUANTUM, fx.TINY, fx.MIX_W
EVALS = {"exp": 0}                     # 40-digit exponentials the references cost


# ----------------------------------------------------------------------------- exact integers
def _log2_den(v):
    return float(v).as_integer_ratio()[1].bit_length() - 1


def _scale(*arrays):
    """s with every finite entry of the arrays an integer multiple of 2^-s"""
    s = 0
    for a in arrays:
        for v in np.asarray(a, dtype=np.float64).ravel():
            if v == v and v != 0.0:
                s = max(s, _log2_den(v))
    return s


def _ints(a, s):
    """the entries of a times 2^s as Python integers (NaN -> 0: masked by the caller)"""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx, v in np.ndenumerate(a):
        if v != v:
            out[idx] = 0
        else:
            num, den = float(v).as_integer_ratio()
            out[idx] = num << (s - (den.bit_length() - 1))
    return out


@functools.lru_cache(maxsize=None)
def _exp_neg(num, shift):
    """exp(-num / 2^shift), an mpf at DPS digits"""
    EVALS["exp"] += 1
    with mp.workdps(DPS):
        return mp.exp(-mp.ldexp(mp.mpf(num), -shift))


def exp_neg(num, shift):
    if num == 0:
        return mp.mpf(1)
    t = min((num & -num).bit_length() - 1, shift)
    return _exp_neg(num >> t, shift - t)


# ----------------------------------------------------------------------------- one block of correlations
def table(w, Theta, XA, XB, symmetric=False, exact_distance=False):
    """The Table (family_exact.Table) of the block between the rows of XA [m, d] and of XB [n, d] under the weights w [K] and
    the rates Theta [K, d].  symmetric: XA is XB, only the lower triangle is evaluated.  exact_distance: delta_c = 0 (the
    caller asserts that the expanded distance is exact in fp64)."""
    XA, XB = np.asarray(XA, dtype=np.float64), np.asarray(XB, dtype=np.float64)
    Theta, w = np.asarray(Theta, dtype=np.float64), np.asarray(w, dtype=np.float64)
    (m, d), n, K = XA.shape, XB.shape[0], Theta.shape[0]
    assert XB.shape[1] == d and Theta.shape == (K, d) and w.shape == (K,)
    sx, st = _scale(XA, XB), _scale(Theta)
    A, B, Ti = _ints(XA, sx), _ints(XB, sx), _ints(Theta, st)
    D = A[:, None, :] - B[None, :, :]
    args = np.dot(D * D, Ti.T)                                   # [m, n, K] exact integers over 2^(2 sx + st)
    shift = 2 * sx + st
    nanA, nanB = np.isnan(XA).any(axis=1), np.isnan(XB).any(axis=1)
    absA, absB = np.abs(np.nan_to_num(XA)), np.abs(np.nan_to_num(XB))
    if exact_distance:
        growth = np.full((m, n, K), 4.0 * U)
    else:
        M = np.einsum("ck,ijk->ijc", Theta, (absA[:, None, :] + absB[None, :, :]) ** 2)
        growth = np.expm1(2.0 * (d + 4) * U * M) + 4.0 * U
    T = Table((m, n))
    seen = {}
    with mp.workdps(DPS):
        w2 = [mp.mpf(float(v)) ** 2 for v in w]
        sw = sum(w2)
        for i in range(m):
            if nanA[i]:
                continue
            for j in range(i + 1 if symmetric else n):
                if nanB[j]:
                    continue
                key = tuple(args[i, j])
                got = seen.get(key)
                if got is None:
                    terms = [w2[c] * exp_neg(key[c], shift) / sw for c in range(K)]
                    ref = sum(terms)
                    hi = float(ref)
                    got = seen[key] = (hi, float(ref - mp.mpf(hi)), np.array([float(t) for t in terms]), ref < TINY)
                hi, lo, terms, tiny = got
                band = float(terms @ growth[i, j]) + (2 * K + 4) * U * abs(hi) + (2.0 * QUANTUM if tiny else 0.0)
                T.hi[i, j], T.lo[i, j], T.band[i, j], T.has[i, j] = hi, lo, band, True
                if symmetric and j < i and not nanB[i] and not nanA[j]:
                    T.hi[j, i], T.lo[j, i], T.band[j, i], T.has[j, i] = hi, lo, band, True
    return T


_LIBM_EXP = np.frompyfunc(math.exp, 1, 1)          # libm's exp entry by entry: numpy's own vectorised exp differs between CPUs


def kernel_restatement(w, Theta, XA, XB, clamp=False):
    """cov_kernel<0> in numpy fp64, statement by statement without fused multiply-adds and with libm's exp: u = sum_k (x x)
    theta, s = sum_k (x_i theta) x_j, dist = (u_i + u_j) - 2 s (-2 s is exact: the fused form gives the same bits here), the
    components accumulated as w_c^2 e_c + acc, the product with 1 / sum w^2.  clamp: with the distance clamped at 0 by fmax, the
    planted mistake that the NaN cases must reject."""
    XA, XB = np.asarray(XA, dtype=np.float64), np.asarray(XB, dtype=np.float64)
    Theta, w = np.asarray(Theta, dtype=np.float64), np.asarray(w, dtype=np.float64)
    (m, d), n, K = XA.shape, XB.shape[0], Theta.shape[0]
    w2 = w * w
    sw = 0.0
    for c in range(K):
        sw += w2[c]
    inv_sw = 1.0 / sw
    acc = np.zeros((m, n))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for c in range(K):
            ua, ub, s = np.zeros(m), np.zeros(n), np.zeros((m, n))
            for k in range(d):
                ua = ua + (XA[:, k] * XA[:, k]) * Theta[c, k]
                ub = ub + (XB[:, k] * XB[:, k]) * Theta[c, k]
                s = (XA[:, k] * Theta[c, k])[:, None] * XB[None, :, k] + s
            dist = (ua[:, None] + ub[None, :]) + -2.0 * s
            if clamp:
                dist = np.fmax(dist, 0.0)
            acc = w2[c] * _LIBM_EXP(-dist).astype(np.float64) + acc
        return inv_sw * acc


class Case:
    """One call of a Gaussian correlation entry point.  Xnew None: the Gram matrix of X (ccgp_corr_matrix for one component of
    weight 1, ccgp_mixed_corr_matrix otherwise); else the cross block (ccgp_corr_cross / ccgp_mixed_corr_cross)."""

    def __init__(self, group, name, w, Theta, Xnew, X, exact_distance=False):
        self.group, self.id = group, "%s-%s" % (group, name)
        self.w, self.Theta = np.asarray(w, dtype=np.float64), np.atleast_2d(np.asarray(Theta, dtype=np.float64))
        self.K, self.d = self.Theta.shape
        self.X = np.asarray(X, dtype=np.float64).reshape(-1, self.d)
        self.Xnew = None if Xnew is None else np.asarray(Xnew, dtype=np.float64).reshape(-1, self.d)
        self.exact_distance = exact_distance
        self.single = self.K == 1 and self.w[0] == 1.0
        self._T = None

    def rows(self):
        return self.X if self.Xnew is None else self.Xnew

    def row(self):
        return np.concatenate([self.w, self.Theta.ravel()])

    def reference(self):
        """cached: the cases are built once per module"""
        if self._T is None:
            self._T = table(self.w, self.Theta, self.rows(), self.X, self.Xnew is None, self.exact_distance)
        return self._T

    def restated(self):
        return kernel_restatement(self.w, self.Theta, self.rows(), self.X)


# ----------------------------------------------------------------------------- the cases
TILE_N = (1, 63, 64, 65, 130)
TILE_MN = ((1, 130), (65, 1), (65, 63), (130, 65))
TILE_THETA = {1: np.array([[2.0, 0.5]]), 2: np.array([[2.0, 0.5], [8.0, 4.0]])}
WIDE_N, WIDE_M = 20, 7
WIDE_DK = ((9, 3), (22, 2), (64, 8), (64, 1))
NEAR_THETAS = (0.01, 0.5, 200.0)
RANGE_THETAS = (0.0037, 3.7)            # a factor 1000 apart
RANGE_ARGS = np.concatenate([np.logspace(-9.0, math.log10(745.0), 120), [708.0, 710.0, 740.0]])
RANGE_BEYOND = (750.0, 1e4)


def tile_design(n, d):
    """x_i = (i / 128, (37 i mod 128) / 128)[:d]: dyadic, and the second coordinate breaks every symmetry of the first"""
    i = np.arange(n)
    return np.stack([dyadic_grid(n), ((37 * i) % 128) / 128.0], axis=1)[:, :d]


def tile_sites(m, d):
    i = np.arange(m)
    return np.stack([half_grid(m), (2.0 * ((53 * i) % 128) + 1.0) / 256.0], axis=1)[:, :d]


def _weights(K):
    return (1.0,) if K == 1 else MIX_W


@functools.lru_cache(maxsize=None)
def tile_cases():
    out = []
    for d in (1, 2):
        for K in (1, 2):
            Th = TILE_THETA[K][:, :d]
            for n in TILE_N:
                out.append(Case("tile", "n%d-d%d-K%d" % (n, d, K), _weights(K), Th, None, tile_design(n, d), True))
            for m, n in TILE_MN:
                out.append(Case("tile", "m%d-n%d-d%d-K%d" % (m, n, d, K), _weights(K), Th, tile_sites(m, d), tile_design(n, d), True))
    return out


@functools.lru_cache(maxsize=None)
def wide_cases():
    out = []
    for d, K in WIDE_DK:
        rng = np.random.default_rng(1000 * d + K)
        X, Xnew = rng.random((WIDE_N, d)), rng.random((WIDE_M, d))
        Th = np.exp(rng.uniform(math.log(0.005), math.log(1.5), size=(K, d)))
        w = np.ones(1) if K == 1 else 0.2 + 0.8 * rng.random(K)
        out.append(Case("wide", "n%d-d%d-K%d" % (WIDE_N, d, K), w, Th, None, X))
        out.append(Case("wide", "m%d-n%d-d%d-K%d" % (WIDE_M, WIDE_N, d, K), w, Th, Xnew, X))
    return out


def near_design(offset):
    """n = 14, d = 2, unsorted: rows 4 and 10 lie 1e-7 from rows 1 and 0 (first coordinate), row 7 IS row 2, row 12 lies 1e-4
    from row 5."""
    x0 = near_coincident_design(0.0)
    x1 = np.array([0.13, 0.71, 0.29, 0.88, 0.71, 0.52, 0.07, 0.29, 0.94, 0.36, 0.13, 0.61, 0.52, 0.45])
    X = np.stack([x0, x1], axis=1)
    X[7] = X[2]
    return X + offset


@functools.lru_cache(maxsize=None)
def near_cases():
    out = []
    for offset in (0.0, 10.0):
        X = near_design(offset)
        for th in NEAR_THETAS:
            out.append(Case("near", "offset%g-theta%g-K1" % (offset, th), (1.0,), [[th, 2.0 * th]], None, X))
            out.append(Case("near", "offset%g-theta%g-K2" % (offset, th), MIX_W, [[th, 2.0 * th], [3.0 * th, th]], None, X))
    return out


def range_h(theta):
    """the column of h for the rate theta: theta h^2 over RANGE_ARGS, then RANGE_BEYOND (exactly 0), then h = 0"""
    return np.concatenate([np.sqrt(np.concatenate([RANGE_ARGS, RANGE_BEYOND]) / theta), [0.0]])


RANGE_SUBNORMAL = len(RANGE_ARGS) - 1           # the column of argument 740: exp(-740) = 4.2e-322


@functools.lru_cache(maxsize=None)
def range_cases():
    """One site at the origin against a column of h.  The mixes: rates a factor 1000 apart in both orders (the fast component
    has underflowed to 0 from argument 0.75 on while the slow one lives), then a zero weight on the fast component, first or
    second.  The live component is always the one of rate `slow`, so every case has the same three special columns."""
    out = []
    for th in RANGE_THETAS:
        out.append(Case("range", "theta%g" % th, (1.0,), [[th]], [[0.0]], range_h(th)[:, None]))
    slow, fast = RANGE_THETAS
    h = range_h(slow)[:, None]
    for name, w, Th in (("mix-slow-fast", MIX_W, (slow, fast)), ("mix-fast-slow", MIX_W, (fast, slow)),
                        ("zero-weight-second", (1.0, 0.0), (slow, fast)), ("zero-weight-first", (0.0, 1.0), (fast, slow))):
        out.append(Case("range", name, w, [[Th[0]], [Th[1]]], [[0.0]], h))
    return out


@functools.lru_cache(maxsize=None)
def nan_cases():
    """(case, NaN rows, NaN columns): one NaN coordinate in X (the Gram matrix: its row and column; the cross block: its
    column), then one in Xnew (its row)."""
    X = near_design(0.0)
    Xn = X.copy()
    Xn[5, 1] = np.nan
    sites = np.array([[0.1, 0.3], [0.41, 0.13], [0.7, 0.9]])
    sites_n = sites.copy()
    sites_n[1, 0] = np.nan
    out = []
    for Xnew, XX, rows, cols, name in ((None, Xn, [5], [5], "X-gram"), (sites, Xn, [], [5], "X-cross"), (sites_n, X, [1], [], "Xnew")):
        out.append((Case("nan", name + "-K1", (1.0,), [[0.5, 1.0]], Xnew, XX), rows, cols))
        out.append((Case("nan", name + "-K2", MIX_W, [[0.5, 1.0], [1.5, 0.5]], Xnew, XX), rows, cols))
    return out


def correlation_cases():
    return tile_cases() + wide_cases() + near_cases() + range_cases() + [c for c, _, _ in nan_cases()]


# ----------------------------------------------------------------------------- R.Inv helpers: references and bands
class Scalar:
    """ref = hi + lo, band; ratio(dev) = |dev - ref| / band in long double"""

    def __init__(self, ref, band):
        self.hi = float(ref)
        with mp.workdps(DPS):
            self.lo = float(ref - mp.mpf(self.hi))
        self.band = float(band)

    def ratio(self, dev):
        if dev != dev:
            return math.inf
        err = abs((np.longdouble(dev) - np.longdouble(self.hi)) - np.longdouble(self.lo))
        return float(err / np.longdouble(self.band)) if self.band > 0 else (0.0 if err == 0 else math.inf)


def _vector(refs, bands):
    T = Table((len(refs),))
    with mp.workdps(DPS):
        for i, ref in enumerate(refs):
            T.hi[i] = float(ref)
            T.lo[i] = float(ref - mp.mpf(T.hi[i]))
    T.band[:] = bands
    T.has[:] = True
    return T


def _mpf_rows(A):
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(A, dtype=np.float64)]


def rinv_terms_reference(A, y, beta):
    """dict(mean_factor, colsum: Tables [n]; beta_mle, sigma2, v2: Scalars) of rinv_terms_kernel's outputs for R.Inv = A, y
    and beta as passed: beta_mle does not depend on beta (ccgp_beta_mle runs the kernel with 0), sigma2 = e'Ae / n and
    mean.factor do."""
    A, y, beta = np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64), float(beta)
    n = y.size
    absA = np.abs(A)
    ymag = np.abs(y) + abs(beta)
    c = absA.sum(axis=0)
    s = n / 4.0 + n / 64.0
    with mp.workdps(DPS):
        rows = _mpf_rows(A)
        cols = [list(col) for col in zip(*rows)]
        ym = [mp.mpf(float(v)) for v in y]
        e = [v - mp.mpf(beta) for v in ym]
        mf = [mp.fdot(row, e) for row in rows]
        cs = [mp.fsum(col) for col in cols]
        a0, a1, a2 = mp.fdot(cs, ym), mp.fsum(cs), mp.fdot(e, mf)
        d0, d1 = (s + 18) * U * float(np.abs(y) @ c), (s + 18) * U * float(c.sum())
        d2 = (s + 20) * U * float(ymag @ (absA @ ymag))
        b = a0 / a1
        out = dict(mean_factor=_vector(mf, (n / 4.0 + 8) * U * (absA @ ymag)), colsum=_vector(cs, (n / 4.0 + 6) * U * c),
                   beta_mle=Scalar(b, (d0 + abs(float(b)) * d1) / abs(float(a1)) + 2 * U * abs(float(b))),
                   sigma2=Scalar(a2 / n, d2 / n + 2 * U * abs(float(a2 / n))), v2=Scalar(a1, d1))
    return out


def predict_reference(A, r, beta, mf, v1, v2, sigma2):
    """(mean, var): Tables [m] of predict_factors_kernel's outputs for the rows of r [m, n] (HX:667-670 on the caller's terms)"""
    A, r = np.asarray(A, dtype=np.float64), np.atleast_2d(np.asarray(r, dtype=np.float64))
    mf, v1 = np.asarray(mf, dtype=np.float64), np.asarray(v1, dtype=np.float64)
    m, n = r.shape
    absA = np.abs(A)
    means, variances, bm, bv = [], [], np.zeros(m), np.zeros(m)
    with mp.workdps(DPS):
        rows = _mpf_rows(A)
        mfm, v1m = [mp.mpf(float(v)) for v in mf], [mp.mpf(float(v)) for v in v1]
        for t in range(m):
            rt = [mp.mpf(float(v)) for v in r[t]]
            q = mp.fdot(rt, [mp.fdot(row, rt) for row in rows])
            s1, sm = mp.fdot(v1m, rt), mp.fdot(mfm, rt)
            ut = 1 - s1
            means.append(mp.mpf(float(beta)) + sm)
            variances.append(mp.mpf(float(sigma2)) * (1 - q + ut * ut / mp.mpf(float(v2))))
            ar = np.abs(r[t])
            dq = (n / 4.0 + n / 64.0 + 18) * U * float(ar @ (absA @ ar))
            ds1 = (n / 64.0 + 10) * U * float(np.abs(v1) @ ar)
            bm[t] = (n / 64.0 + 12) * U * float(np.abs(mf) @ ar) + 2 * U * abs(float(beta))
            bv[t] = float(sigma2) * (dq + 2 * abs(float(ut)) * ds1 / float(v2) + 4 * U * (1 + abs(float(q)) + float(ut) ** 2 / float(v2)))
    return _vector(means, bm), _vector(variances, bv)


# ----------------------------------------------------------------------------- R.Inv helpers: the kernels restated
def _wg4_sum(x):
    """wg4_sum of capi.hip on the 256 per-thread values: a shfl_down tree in each wave, then (w0 + w1) + (w2 + w3)"""
    red = []
    for wv in range(4):
        v = np.array(x[64 * wv:64 * wv + 64], dtype=np.float64)
        for off in (32, 16, 8, 4, 2, 1):
            v[:64 - off] = v[:64 - off] + v[off:]
        red.append(v[0])
    return (red[0] + red[1]) + (red[2] + red[3])


def _row_products(A, x):
    """(A x)_i as the kernels form it: four partial sums over the columns j = wave, wave + 4, ..., then (p0 + p1) + (p2 + p3)"""
    n = A.shape[0]
    part = np.zeros((4, n))
    for j in range(n):
        part[j % 4] = A[:, j] * x[j] + part[j % 4]
    return (part[0] + part[1]) + (part[2] + part[3])


def _lane_sums(terms):
    """per-lane accumulators of wave 0 over passes of 64 rows (acc = term + acc), the other waves 0: 256 values"""
    acc = np.zeros(256)
    for i0 in range(0, terms.size, 64):
        seg = terms[i0:i0 + 64]
        acc[:seg.size] = seg + acc[:seg.size]
    return acc


def rinv_terms_restatement(A, y, beta):
    """rinv_terms_kernel in numpy fp64 without fused multiply-adds: (mean_factor[n], colsum[n], a0, a1, a2)"""
    A, y = np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = y.size
    with np.errstate(invalid="ignore"):
        e = y - beta
        mf = _row_products(A, e)
        a2 = _wg4_sum(_lane_sums(e * mf))
        part = np.zeros((4, n))
        for i in range(n):
            part[i % 4] = part[i % 4] + A[i, :]
        cs = part[0] + part[1]                               # lane q = 0 after shfl_xor 1 ...
        cs = cs + (part[2] + part[3])                        # ... and after shfl_xor 2
        t0, t1 = np.zeros(256), np.zeros(256)
        for j0 in range(0, n, 64):                           # thread 4 (j - j0) owns column j
            seg = slice(j0, min(n, j0 + 64))
            k = 4 * np.arange(seg.stop - seg.start)
            t0[k] = cs[seg] * y[seg] + t0[k]
            t1[k] = t1[k] + cs[seg]
        return mf, cs, _wg4_sum(t0), _wg4_sum(t1), a2


def predict_restatement(A, r, beta, mf, v1, v2, sigma2):
    """predict_factors_kernel in numpy fp64 without fused multiply-adds: (mean[m], var[m])"""
    A, r = np.asarray(A, dtype=np.float64), np.atleast_2d(np.asarray(r, dtype=np.float64))
    mean, var = np.zeros(r.shape[0]), np.zeros(r.shape[0])
    with np.errstate(invalid="ignore"):
        for t, rt in enumerate(r):
            acc = _row_products(A, rt)
            q, s1, sm = _wg4_sum(_lane_sums(rt * acc)), _wg4_sum(_lane_sums(v1 * rt)), _wg4_sum(_lane_sums(mf * rt))
            ut = 1.0 - s1
            var[t] = sigma2 * (1.0 - q + ut * ut / v2)
            mean[t] = beta + sm
    return mean, var


# ----------------------------------------------------------------------------- R.Inv helpers: the cases
HELPER_N = (1, 3, 4, 5, 63, 64, 65, 129, 257)        # 4-way column striding, 64-row passes, 4 lanes per column
HELPER_SITES = {1: 1, 3: 5, 4: 65, 5: 5, 63: 5, 64: 1, 65: 65, 129: 5, 257: 5}
HELPER_SIGMA2 = 1.3
HELPER_COND = 1e8
FAR = 50.0


def _oracle():
    from oracle import ccgp_oracle as orc
    return orc


def conditioned_gauss(n, seed):
    """(X [n, 2], row, R) of a two-component Gaussian mix on a random design whose rates are scaled (bisection on the scale)
    until cond1(R) is about HELPER_COND; n = 1 has nothing to scale."""
    orc = _oracle()
    rng = np.random.default_rng(seed)
    X = rng.random((n, 2))
    w = np.array([0.8, 0.6])
    Th = np.exp(rng.uniform(math.log(0.5), math.log(4.0), size=(2, 2)))
    lo, hi = -30.0, 12.0                                     # log scale: cond1 falls as the rates grow
    for _ in range(60 if n > 1 else 0):
        mid = 0.5 * (lo + hi)
        kappa = np.linalg.cond(orc.mixed_corr_matrix_general(X, w, Th * math.exp(mid)), 1)
        lo, hi = (mid, hi) if kappa > HELPER_COND else (lo, mid)
    Th = Th * math.exp(hi)
    return X, np.concatenate([w, Th.ravel()]), orc.mixed_corr_matrix_general(X, w, Th)


class HelperCase:
    """One R.Inv with its y and the terms predict.post is handed.  kind 'asym': a visibly asymmetric matrix, sites r uniform in
    [0, 1).  kind 'gauss': the long-double inverse, rounded, of a Gaussian mixed matrix with cond1 ~ 1e8; the rows of r are
    that mix's correlations (the restated kernel's, as a caller would pass them) for a site ON training point n / 2, a site
    so far out (50 in every coordinate, or more where the rates are tiny) that r underflows to 0, and random interior sites.
    m = 1: the training point at n < 64, the far site otherwise.  beta, mean.factor, v1 and v2 are the fp64 oracle's: the kernels take them as passed."""

    def __init__(self, n, kind):
        orc = _oracle()
        self.n, self.kind, self.id, self.m = n, kind, "%s-n%d" % (kind, n), HELPER_SITES[n]
        rng = np.random.default_rng(77 + n)
        self.far = self.on = None
        if kind == "asym":
            self.A = rng.normal(size=(n, n)) + n * np.eye(n)
            self.y = rng.normal(size=n)
            self.r = rng.random((self.m, n))
            self.cond = None
        else:
            X, row, R = conditioned_gauss(n, 500 + n)
            Ainv = orc.solve_inverse_exact(R, np.longdouble)
            self.A = np.asarray(Ainv, dtype=np.float64)
            self.cond = orc.cond1(R, Ainv)
            self.y = np.sin(2 * np.pi * X).sum(axis=1) + 0.3
            far = max(FAR, math.ceil(math.sqrt(1000.0 / row[2:].min())))          # every exponent beyond -1000: r is exactly 0
            sites = np.vstack([X[n // 2][None], np.full((1, 2), far), rng.random((max(self.m - 2, 0), 2))])
            pick = [0 if n < 64 else 1] if self.m == 1 else list(range(self.m))
            self.on = pick.index(0) if 0 in pick else None
            self.far = pick.index(1) if 1 in pick else None
            self.X, self.row, self.sites = X, row, sites[pick]
            self.r = kernel_restatement(row[:2], row[2:].reshape(2, 2), self.sites, X)
        self.beta = float(orc.beta_mle(self.A, self.y))
        mf, v1, v2 = orc.factors(self.A, self.beta, self.y)
        self.mf, self.v1, self.v2 = np.asarray(mf, dtype=np.float64), np.asarray(v1, dtype=np.float64), float(v2)
        self._terms = self._predict = None

    def terms_reference(self):
        if self._terms is None:
            self._terms = rinv_terms_reference(self.A, self.y, self.beta)
        return self._terms

    def predict_reference(self):
        if self._predict is None:
            self._predict = predict_reference(self.A, self.r, self.beta, self.mf, self.v1, self.v2, HELPER_SIGMA2)
        return self._predict


HELPER_KEYS = [(kind, n) for kind in ("asym", "gauss") for n in HELPER_N]


@functools.lru_cache(maxsize=None)
def helper_case(kind, n):
    """built on first use, not when the test modules are collected"""
    return HelperCase(n, kind)


def helper_cases():
    return [helper_case(*k) for k in HELPER_KEYS]


NAN_N, NAN_M, NAN_Y, NAN_R = 65, 5, 7, (2, 9)               # y[7] = NaN; then r[2, 9] = NaN


@functools.lru_cache(maxsize=None)
def helper_nan_case():
    """the asymmetric n = 65 matrix with five sites"""
    c = HelperCase(NAN_N, "asym")
    c.m, c.r = NAN_M, c.r[:NAN_M].copy()
    c.id = "nan-n%d" % NAN_N
    return c


# ----------------------------------------------------------------------------- the literal chain
CHAIN_N = (14, 65)
CHAIN_M = 5
CHAIN_SIGMA2 = 1.3


@functools.lru_cache(maxsize=None)
def chain_case(n):
    """(X, y, row, K, Xt) of a literal chain: the maximin design at n = 14, a seeded one at n = 65; a draw with cond1 <= 1e8
    (oracle.conditioned_row); 5 sites: training point 3, a 1e-6 neighbour of training point 0, two interior sites, (50, 50)."""
    orc = _oracle()
    rng = np.random.default_rng(4000 + n)
    if n == 14:
        from conftest import load_maximin
        X = np.asarray(load_maximin(14), dtype=np.float64)
    else:
        X = rng.random((n, 2))
    d = X.shape[1]
    y = np.sin(2 * np.pi * X).sum(axis=1) + 0.3
    row = orc.conditioned_row(X, 2, d, rng, HELPER_COND)[0]
    Xt = np.vstack([X[3][None], X[0][None] + 1e-6 * np.eye(d)[0], rng.random((2, d)) * (X.max(axis=0) - X.min(axis=0)) + X.min(axis=0),
                    np.full((1, d), FAR)])
    return X, y, row, 2, Xt


def run_chain(n, mixed_corr_matrix, beta_mle, factors, predict_post):
    """Mixed.corr.matrix -> a long-double solve(R) on the host, rounded -> beta.MLE -> factors -> predict.post at the 5 sites,
    with the four callables the device's entry points or their restatements: (mean[5], var[5], beta)."""
    orc = _oracle()
    X, y, row, K, Xt = chain_case(n)
    R = np.asarray(mixed_corr_matrix(X, K, row), dtype=np.float64)
    R_inv = np.asarray(orc.solve_inverse_exact(R, np.longdouble), dtype=np.float64)
    beta = float(beta_mle(R_inv, y))
    f = np.asarray(factors(R_inv, beta, y))
    mean, var = predict_post(Xt, X, K, row, beta, f[:n], f[n:2 * n], f[2 * n], R_inv, CHAIN_SIGMA2)
    return np.asarray(mean), np.asarray(var), beta


@functools.lru_cache(maxsize=None)
def chain_reference(n):
    """(mean[5], var[5], beta: oracle/mp_check.predict at 50 digits, rounded; band: tests/test_gpu_predict_exact.py's, the
    dict of oracle.predict_bands around the long-double tables with C = PREDICT_TOL_C)"""
    from oracle import mp_check
    import test_gpu_predict_exact as tpe
    orc = _oracle()
    X, y, row, K, Xt = chain_case(n)
    w, Th = orc.unpack_params(row, K, X.shape[1])
    means, variances, beta = mp_check.predict(X, y, w, Th, CHAIN_SIGMA2, Xt)
    _, band, kappa = tpe.reference(X, y, row, K, Xt, CHAIN_SIGMA2)
    assert kappa <= HELPER_COND
    return np.array([float(v) for v in means]), np.array([float(v) for v in variances]), float(beta), band


def restated_chain(n):
    def corr(X, K, row):
        return kernel_restatement(row[:K], row[K:].reshape(K, -1), X, X)

    def post(Xt, X, K, row, beta, mf, v1, v2, R_inv, sigma2):
        r = kernel_restatement(row[:K], row[K:].reshape(K, -1), Xt, X)
        return predict_restatement(R_inv, r, beta, mf, v1, v2, sigma2)

    def beta_mle(R_inv, y):
        _, _, a0, a1, _ = rinv_terms_restatement(R_inv, y, 0.0)
        return a0 / a1

    def factors(R_inv, beta, y):
        mf, cs, _, a1, _ = rinv_terms_restatement(R_inv, y, beta)
        return np.concatenate([mf, cs, [a1]])

    return run_chain(n, corr, beta_mle, factors, post)
