"""Exact references and component-wise bands for the 1-D scripts' correlation families (CCGP_KERNEL_MATERN, D1:348-351;
CCGP_KERNEL_MATERN_SPLINE, D1F:346-357 and D1F:453-480), shared by tests/test_gpu_family_corr_exact.py (every entry out of the
C ABI), tests/test_gpu_family_end_to_end.py (Sigma and r built from these entries) and tests/test_family_corr_host.py (the
same cases against the kernel's arithmetic restated in libm, no GPU).

Reference.  The fp64 inputs are taken as exact rationals (fractions.Fraction): |h| = |x_i - x_j| and u = |h| / theta
exactly, z = 2 sqrt(nu) |h| / theta and f = z^nu K_nu(z) / (Gamma(nu) 2^(nu-1)) in mpmath at DPS = 40 digits, exactly 1 at
h = 0; the spline's cubic in exact rational arithmetic.  Cached by (nu, theta, |h|).

Bands (component-wise; no condition number, and no absolute floor apart from two subnormal quanta where ref < 2.3e-308):
  Matern  |dev - ref| <= (5e-14 + 4 eps z) ref.  5e-14 is what tests/test_special.py asks of the quadrature rule; 4 eps z
          covers the rounding of z (theta^2, the division, h, h^2, the product, the square root: 2 eps relative in z)
          and of the exponent nu log z - z, through |z f'| <= z f.
  spline  4 eps (A(u) + |u f'(u)|): A = 1 + 6 u^2 + 6 u^3 on the first branch (the sizes of the terms summed), A = f on the
          second (1 - u is exact there); the second term is the same 2 eps of u.  Exactly 0 for u >= 1 + 4 eps.  Within
          4 ulp of a knot (1/2, 1) the device's u may sit on the other branch and, at u = 1, a first-order band at the exact
          u misses the triple root: there the band is the largest of both branches' bands at u - 4 ulp, u and u + 4 ulp.
  mixes   the w^2-weighted sum of the component bands (normalised like the value) + 2 eps |ref|: with weights whose squares
          and their sum are exact in fp64 (MIX_W) the device rounds two fused multiply-adds, one reciprocal and one product,
          4 roundings of eps / 2.
"""
import functools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 40
EPS = 2.0 ** -52
QUANTUM = 2.0 ** -1074
TINY = 2.3e-308
NUS = (1.0001, 1.01, 1.1, 1.5, 2.0, 2.5, 5.0, 7.3, 10.0)
SWITCHES = (3e-10, 1e-5, 1.0)          # matern_corr: exactly 1 | two-term series (nu >= 1.5) | step 0.15 | step 0.15 / sqrt z
MIX_W = (0.75, 0.5)                    # w^2 = 0.5625, 0.25 and their sum 0.8125 are exact
EVALS = {"besselk": 0}                 # how many 40-digit Bessel evaluations the references cost (the module asserts the time)

_F = Fraction


def frac(x):
    return _F(float(x))


def _to_mp(q):
    return mp.mpf(q.numerator) / mp.mpf(q.denominator)


# ----------------------------------------------------------------------------- Matern
def matern_f(nu, z):
    """z^nu K_nu(z) / (Gamma(nu) 2^(nu-1)) at an mpf z > 0, DPS digits."""
    with mp.workdps(DPS):
        EVALS["besselk"] += 1
        nu = mp.mpf(nu)
        return z ** nu * mp.besselk(nu, z) / (mp.gamma(nu) * mp.mpf(2) ** (nu - 1))


@functools.lru_cache(maxsize=None)
def matern(nu, theta, habs):
    """(ref, band, z) as mpf for |h| = habs (a Fraction) under Matern(nu, theta)."""
    with mp.workdps(DPS):
        if habs == 0:
            return mp.mpf(1), mp.mpf(0), mp.mpf(0)
        z = 2 * mp.sqrt(mp.mpf(nu)) * _to_mp(habs / frac(theta))
        f = matern_f(nu, z)
        band = (mp.mpf(5e-14) + 4 * EPS * z) * f
        if f < TINY:
            band += 2 * mp.mpf(QUANTUM)
        return f, band, z


@functools.lru_cache(maxsize=None)
def first_subnormal_z(nu):
    """A z whose Matern(nu) value is subnormal: 1.001 times the root of f(z) = 2^-1022 (f decreases beyond z = 700)."""
    with mp.workdps(DPS):
        lo, hi, target = mp.mpf(700), mp.mpf(780), mp.mpf(2) ** -1022
        assert matern_f(nu, lo) > target > matern_f(nu, hi)
        for _ in range(30):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if matern_f(nu, mid) > target else (lo, mid)
        return float(hi) * 1.001


def sweep_z(nu):
    """The z of the domain sweep: 150 log-spaced over [1e-9, 800], both sides of every switch of the rule, 300, 700, 740 and
    a z whose value is subnormal."""
    zs = list(np.logspace(-9.0, math.log10(800.0), 150))
    for s in SWITCHES:
        zs += [s * (1.0 - 1e-12), s * (1.0 + 1e-12)]
    return np.array(zs + [300.0, 700.0, 740.0, first_subnormal_z(nu)])


def sweep_h(nu, theta):
    """The column of |h| for one (nu, theta): h = z theta / (2 sqrt nu) in fp64 for sweep_z, then z = 1e4 (must give exactly
    0) and h = 0 (must give exactly 1)."""
    z = np.concatenate([sweep_z(nu), [1e4]])
    return np.concatenate([z * theta / (2.0 * math.sqrt(nu)), [0.0]])


# ----------------------------------------------------------------------------- cubic spline
def _spline_first(u):
    return 1 - 6 * u ** 2 + 6 * u ** 3, 4 * _F(EPS) * (1 + 6 * u ** 2 + 6 * u ** 3 + abs(u * (-12 * u + 18 * u ** 2)))


def _spline_second(u):
    v = 1 - u
    return 2 * v ** 3, 4 * _F(EPS) * (abs(2 * v ** 3) + abs(u * 6 * v ** 2))


@functools.lru_cache(maxsize=None)
def spline(theta, habs):
    """(ref, band, u) as exact Fractions for |h| = habs under the spline with scale theta (D1F:346-357)."""
    u = habs / frac(theta)
    if u >= 1 + 4 * _F(EPS):
        return _F(0), _F(0), u
    ref = _spline_first(u)[0] if u <= _F(1, 2) else _spline_second(u)[0] if u <= 1 else _F(0)
    near_half, near_one = abs(u - _F(1, 2)) <= 2 * _F(EPS), abs(u - 1) <= 4 * _F(EPS)       # 4 ulp: ulp(1/2) = eps / 2, ulp(1) = eps
    if near_half:
        band = max(b(v)[1] for b in (_spline_first, _spline_second) for v in (u - 2 * _F(EPS), u, u + 2 * _F(EPS)))
    elif near_one:                                          # the other neighbour is the constant 0, whose band is 0
        band = max(_spline_second(v)[1] for v in (u - 4 * _F(EPS), u, u + 4 * _F(EPS)))
    else:
        band = (_spline_first if u < _F(1, 2) else _spline_second)(u)[1]
    return ref, band, u


# ----------------------------------------------------------------------------- one entry of a family, and blocks of them
def _entry_of_h(family, nu, w, thetas, habs, raw):
    """(ref, band) as mpf of one entry at an exact |h| (a Fraction).  family 1: Matern components with scales `thetas`;
    family 2: (Matern(thetas[0]), spline(thetas[1])).  w: the weights (len(thetas)); raw: the un-normalised sum
    sum w_c^2 f_c that include/ccgp.h documents for ccgp_mixed_corr_cross under family 2 (D1F:470-480)."""
    with mp.workdps(DPS):
        comps = []
        for c, th in enumerate(thetas):
            if family == 2 and c == 1:
                f, b, _ = spline(float(th), habs)
                comps.append((_to_mp(f), _to_mp(b)))
            else:
                comps.append(matern(float(nu), float(th), habs)[:2])
        if len(comps) == 1 and w[0] == 1.0:
            return comps[0]
        w2 = [frac(v) ** 2 for v in w]
        den = _F(1) if raw else sum(w2)
        ref = sum(_to_mp(q / den) * f for q, (f, _) in zip(w2, comps))
        band = sum(_to_mp(q / den) * b for q, (_, b) in zip(w2, comps)) + 2 * EPS * abs(ref)
        return ref, band


class Table:
    """The references of a block: ref = hi + lo (two float64 arrays: a 32-digit value), band (float64), has (False where a
    coordinate is NaN and there is no reference)."""

    def __init__(self, shape):
        self.hi, self.lo, self.band = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        self.has = np.zeros(shape, dtype=bool)

    def longdouble(self):
        return self.hi.astype(np.longdouble) + self.lo.astype(np.longdouble)


def table(family, nu, w, thetas, XA, XB, raw=False):
    """The Table of the block between the coordinates XA (rows) and XB (columns): one 40-digit evaluation per distinct |h|
    (the difference of two doubles as an exact rational)."""
    XA, XB = np.asarray(XA, dtype=np.float64).reshape(-1), np.asarray(XB, dtype=np.float64).reshape(-1)
    T = Table((XA.size, XB.size))
    fa, fb = [None if math.isnan(v) else frac(v) for v in XA], [None if math.isnan(v) else frac(v) for v in XB]
    seen = {}
    with mp.workdps(DPS):
        for i, a in enumerate(fa):
            for j, b in enumerate(fb):
                if a is None or b is None:
                    continue
                habs = abs(a - b)
                got = seen.get(habs)
                if got is None:
                    ref, band = _entry_of_h(family, nu, tuple(w), tuple(thetas), habs, raw)
                    hi = float(ref)
                    # the band rounded to fp64 (relative 1.1e-16: immaterial); subnormal references keep their quanta exactly
                    got = seen[habs] = (hi, float(ref - mp.mpf(hi)), float(band))
                T.hi[i, j], T.lo[i, j], T.band[i, j] = got
                T.has[i, j] = True
    return T


def worst_ratio(dev, T):
    """(largest |dev - ref| / band over the entries with a reference, the entries outside their band).  The difference is
    taken in long double from ref = hi + lo: exact to 1e-19 of ref.  band = 0: dev must equal ref (ratio 0 or inf)."""
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == T.hi.shape and np.finfo(np.longdouble).eps < 1e-18
    err = np.abs((dev.astype(np.longdouble) - T.hi.astype(np.longdouble)) - T.lo.astype(np.longdouble))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(T.band > 0, err / T.band.astype(np.longdouble), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
    ratio[np.isnan(dev)] = np.inf
    ratio[~T.has] = 0.0
    bad = [(tuple(int(v) for v in idx), float(dev[tuple(idx)]), float(T.hi[tuple(idx)]), float(ratio[tuple(idx)]))
           for idx in np.argwhere(~(ratio <= 1.0))]
    return float(ratio.max()) if ratio.size else 0.0, bad


# ----------------------------------------------------------------------------- designs of the cases
def near_coincident_design(offset):
    """n = 14, unsorted, with two pairs 1e-7 apart and two pairs 1e-4 apart."""
    base = np.array([0.41, 0.05, 0.2, 0.9, 0.05 + 1e-7, 0.66, 0.33, 0.2 + 1e-4, 0.57, 0.78, 0.41 + 1e-7, 0.97, 0.66 + 1e-4, 0.83])
    return base + offset


def dyadic_grid(n):
    return np.arange(n) / 128.0


def half_grid(m):
    return (2.0 * np.arange(m) + 1.0) / 256.0


# ----------------------------------------------------------------------------- the kernel's arithmetic in libm (host checks)
def spline_rule(u2):
    """csrc/ccgp_internal.h spline_corr, statement by statement."""
    u = math.sqrt(u2) if u2 == u2 else u2
    if u <= 0.5:
        return 1.0 - 6.0 * u * u + 6.0 * u * u * u
    if u <= 1.0:
        v = 1.0 - u
        return 2.0 * v * v * v
    return 0.0 if u > 1.0 else u


def kernel_restatement(matern_rule, family, nu, w, thetas, XA, XB, raw=False):
    """cov_kernel<1> in libm arithmetic: rate (x_i - x_j)^2 from the direct difference, the families' rules, the mix as the
    kernel accumulates it.  matern_rule: tests/test_special.py's restatement of matern_corr."""
    XA, XB = np.asarray(XA, dtype=np.float64).reshape(-1), np.asarray(XB, dtype=np.float64).reshape(-1)
    out = np.empty((XA.size, XB.size))
    w2 = [float(v) * float(v) for v in w]
    sw = 0.0
    for q in w2:
        sw += q
    inv_sw = 1.0 if raw else 1.0 / sw
    for i, a in enumerate(XA):
        for j, b in enumerate(XB):
            h = float(a) - float(b)
            acc = 0.0
            for c, th in enumerate(thetas):
                if family == 2 and c == 1:
                    f = spline_rule((1.0 / (th * th)) * (h * h))
                else:
                    f = matern_rule(nu, (4.0 * nu / (th * th)) * (h * h))
                acc = w2[c] * f + acc
            out[i, j] = inv_sw * acc
    return out


# ----------------------------------------------------------------------------- the cases of the entry-point tests
class Case:
    """One call of a correlation entry point.  Xnew None: the Gram matrix of X (ccgp_corr_matrix for K = 1,
    ccgp_mixed_corr_matrix for K = 2); otherwise the cross block (ccgp_corr_cross / ccgp_mixed_corr_cross), which under
    family 2 is the un-normalised sum."""

    def __init__(self, group, name, family, nu, w, thetas, Xnew, X):
        self.group, self.id = group, "%s-%s" % (group, name)
        self.family, self.nu, self.w, self.thetas = family, float(nu), tuple(w), tuple(float(t) for t in thetas)
        self.K = len(self.thetas)
        self.Xnew = None if Xnew is None else np.asarray(Xnew, dtype=np.float64).reshape(-1)
        self.X = np.asarray(X, dtype=np.float64).reshape(-1)
        self.raw = family == 2 and Xnew is not None
        assert (family == 1 and self.K in (1, 2)) or (family == 2 and self.K == 2)
        assert self.K == 2 or self.w == (1.0,)

    def rows(self):
        return self.X if self.Xnew is None else self.Xnew

    def reference(self):
        return table(self.family, self.nu, self.w, self.thetas, self.rows(), self.X, self.raw)

    def row(self):
        return np.array(self.w + self.thetas)

    def tag(self):
        """The MAX_RATIO key: what is being held."""
        if self.family == 1:
            return "matern" if self.K == 1 else "matern-mix"
        return "spline" if self.w[0] == 0.0 else "matern+spline" + ("-raw" if self.raw else "")


SWEEP_THETAS = (0.0037, 3.7)            # a factor 1000 apart: the same z through different rates
NEAR_THETAS = (0.5, 0.05, 0.01)
NEAR_NU = 2.5
TILE_N, TILE_M = (1, 63, 64, 65, 130), (1, 65)
TILE_NU, TILE_THETA, TILE_SPLINE = 2.5, 0.2, 0.7


def _families(group, name, nu, theta, spline_theta, Xnew, X, spline_alone=False):
    """The family variants of one shape: Matern, a Matern mix, Matern + spline (and the spline alone)."""
    out = [Case(group, name + "-matern", 1, nu, (1.0,), (theta,), Xnew, X),
           Case(group, name + "-matern-mix", 1, nu, MIX_W, (theta, 3.0 * theta), Xnew, X),
           Case(group, name + "-matern+spline", 2, nu, MIX_W, (theta, spline_theta), Xnew, X)]
    if spline_alone:
        out.append(Case(group, name + "-spline", 2, nu, (0.0, 1.0), (theta, spline_theta), Xnew, X))
    return out


def sweep_cases(nus=NUS):
    return [Case("sweep", "nu%g-theta%g" % (nu, th), 1, nu, (1.0,), (th,), [0.0], sweep_h(nu, th)) for nu in nus for th in SWEEP_THETAS]


def near_cases():
    out = []
    for offset in (0.0, 10.0):
        for th in NEAR_THETAS:
            out += _families("near", "offset%g-theta%g" % (offset, th), NEAR_NU, th, 2.0 * th, None, near_coincident_design(offset), True)
    return out


def tile_cases():
    out = []
    for n in TILE_N:
        out += _families("tile", "n%d" % n, TILE_NU, TILE_THETA, TILE_SPLINE, None, dyadic_grid(n))
        for m in TILE_M:
            out += _families("tile", "m%d-n%d" % (m, n), TILE_NU, TILE_THETA, TILE_SPLINE, half_grid(m), dyadic_grid(n))
    return out


def nan_cases():
    """(case, NaN rows, NaN columns): one NaN coordinate in X (the Gram matrix: its row and column; the cross block: its
    column), then one in Xnew (its row)."""
    X = near_coincident_design(0.0)
    Xn = X.copy()
    Xn[5] = np.nan
    sites = np.array([0.1, 0.41, 0.7])
    sites_n = np.array([0.1, np.nan, 0.7])
    out = []
    for Xnew, XX, rows, cols, name in ((None, Xn, [5], [5], "X-gram"), (sites, Xn, [], [5], "X-cross"), (sites_n, X, [1], [], "Xnew")):
        out += [(c, rows, cols) for c in _families("nan", name, NEAR_NU, 0.5, 1.0, Xnew, XX, True)]
    return out


def spline_branch_cases():
    """u at, 1 ulp below and 1 ulp above 1/2 and 1, u = 0, and u = 1 + 8 eps (must give exactly 0: the last column), from a
    site at the origin; theta = 1 (the device's u is exact) and theta = 0.3 (it is not)."""
    out = []
    for th in (1.0, 0.3):
        h = [0.0]
        for knot in (th / 2.0, th):
            h += [np.nextafter(knot, 0.0), knot, np.nextafter(knot, 2.0)]
        h.append(th * (1.0 + 8.0 * EPS))
        out.append(Case("branch", "theta%g" % th, 2, 2.5, (0.0, 1.0), (0.5, th), [0.0], h))
    return out
