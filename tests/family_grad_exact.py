"""Exact references and component-wise bands for d corr / d theta of the 1-D scripts' correlation families (csrc/ccgp_internal.h
matern_corr_grad, spline_corr_grad; CCGP_OPT_FAMILY_FUSED_GRAD), on top of tests/family_exact.py.  Shared by
tests/test_family_grad_host.py (the kernel's arithmetic restated in libm, no GPU) and tests/test_gpu_family_fused_grad.py (every
entry out of ccgp_family_corr_dtheta, and the gradients built from them).

Reference.  As in family_exact: the fp64 inputs are exact rationals, |h| = |x_i - x_j| and u = |h| / theta exactly.
  Matern  z = 2 sqrt(nu) |h| / theta, d f / d theta = z^(nu+1) K_(nu-1)(z) / (Gamma(nu) 2^(nu-1) theta) in mpmath at 40 digits
          (from d/dz [z^nu K_nu] = -z^nu K_(nu-1) and dz / d theta = -z / theta); exactly 0 at h = 0.
  spline  g(u) / theta with g = -u f'(u): 12 u^2 - 18 u^3 (u <= 1/2), 6 u (1 - u)^2 (u <= 1), 0 beyond, in exact rationals.

Bands (component-wise, no condition number; two subnormal quanta where ref < 2.3e-308):
  Matern  (5e-14 + 4 eps (z + (nu + 1)(1 + |ln z|))) ref.  5e-14 is tests/test_special.py's figure for the quadrature rule; the
          rest is the rounding of z and of the exponent (nu + 1) log z - z, whose size is (nu + 1) |ln z| + z.  Measured in
          libm arithmetic with exact z (nu 1.0001 ... 10, z 3e-10 ... 740) the rule uses at most 0.29 of the band without the
          `+ 1`; it exceeds the value's own 5e-14 + 4 eps z by 8 % at nu = 7.3, z = 1e-8, which is why the log term is there.
  spline  4 eps (A + |u g'(u)|) / theta + 2 eps ref: A = 12 u^2 + 18 u^3 on the first branch (the sizes of the terms summed),
          A = g on the second (1 - u is exact there); the second term is the 2 eps of u; 2 eps ref the division by theta.
          Knots as family_exact.spline treats them; exactly 0 for u >= 1 + 4 eps.
"""
import functools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

import family_exact as fx

_F = Fraction
EPS = fx.EPS
SWITCH_Z2 = 9e-20                      # matern_corr / matern_corr_grad: exactly (1, 0) up to here
BELOW_SWITCH = 2.1e-18                 # the true derivative there, times theta, stays below this


# ----------------------------------------------------------------------------- Matern
def matern_dtheta_f(nu, z, theta):
    """z^(nu+1) K_(nu-1)(z) / (Gamma(nu) 2^(nu-1) theta) at mpf z > 0 and theta, DPS digits."""
    with mp.workdps(fx.DPS):
        fx.EVALS["besselk"] += 1
        nu = mp.mpf(nu)
        return z ** (nu + 1) * mp.besselk(nu - 1, z) / (mp.gamma(nu) * mp.mpf(2) ** (nu - 1) * theta)


def matern_band(nu, z, ref):
    """The band of one derivative value at mpf z, ref."""
    band = (mp.mpf(5e-14) + 4 * EPS * (z + (mp.mpf(nu) + 1) * (1 + abs(mp.log(z))))) * ref
    if ref < fx.TINY:
        band += 2 * mp.mpf(fx.QUANTUM)
    return band


@functools.lru_cache(maxsize=None)
def matern_dtheta(nu, theta, habs):
    """(ref, band, z) as mpf for |h| = habs (a Fraction) under Matern(nu, theta)."""
    with mp.workdps(fx.DPS):
        if habs == 0:
            return mp.mpf(0), mp.mpf(0), mp.mpf(0)
        th = fx._to_mp(fx.frac(theta))
        z = 2 * mp.sqrt(mp.mpf(nu)) * fx._to_mp(habs / fx.frac(theta))
        ref = matern_dtheta_f(nu, z, th)
        return ref, matern_band(nu, z, ref), z


# ----------------------------------------------------------------------------- cubic spline
def _g_first(u):
    g = 12 * u ** 2 - 18 * u ** 3
    return g, 4 * _F(EPS) * (12 * u ** 2 + 18 * u ** 3 + abs(u * (24 * u - 54 * u ** 2)))


def _g_second(u):
    v = 1 - u
    g = 6 * u * v ** 2
    return g, 4 * _F(EPS) * (abs(g) + abs(u * 6 * v * (1 - 3 * u)))


@functools.lru_cache(maxsize=None)
def spline_dtheta(theta, habs):
    """(ref, band, u) as exact Fractions for |h| = habs under the spline with scale theta."""
    th = fx.frac(theta)
    u = habs / th
    if u >= 1 + 4 * _F(EPS):
        return _F(0), _F(0), u
    g = _g_first(u)[0] if u <= _F(1, 2) else _g_second(u)[0] if u <= 1 else _F(0)
    near_half, near_one = abs(u - _F(1, 2)) <= 2 * _F(EPS), abs(u - 1) <= 4 * _F(EPS)
    if near_half:
        band = max(b(v)[1] for b in (_g_first, _g_second) for v in (u - 2 * _F(EPS), u, u + 2 * _F(EPS)))
    elif near_one:                                          # the other neighbour is the constant 0, whose band is 0
        band = max(_g_second(v)[1] for v in (u - 4 * _F(EPS), u, u + 4 * _F(EPS)))
    else:
        band = (_g_first if u < _F(1, 2) else _g_second)(u)[1]
    ref = g / th
    return ref, band / th + 2 * _F(EPS) * abs(ref), u


# ----------------------------------------------------------------------------- blocks of entries
def dtable(family, nu, thetas, q, XA, XB):
    """The fx.Table of d R_q / d theta_q between the coordinates XA (rows) and XB (columns) for component q of the family:
    one 40-digit evaluation per distinct |h|."""
    XA, XB = np.asarray(XA, dtype=np.float64).reshape(-1), np.asarray(XB, dtype=np.float64).reshape(-1)
    T = fx.Table((XA.size, XB.size))
    fa, fb = [None if math.isnan(v) else fx.frac(v) for v in XA], [None if math.isnan(v) else fx.frac(v) for v in XB]
    seen = {}
    with mp.workdps(fx.DPS):
        for i, a in enumerate(fa):
            for j, b in enumerate(fb):
                if a is None or b is None:
                    continue
                habs = abs(a - b)
                got = seen.get(habs)
                if got is None:
                    if family == 2 and q == 1:
                        ref, band, _ = spline_dtheta(float(thetas[q]), habs)
                        ref, band = fx._to_mp(ref), fx._to_mp(band)
                    else:
                        ref, band, _ = matern_dtheta(float(nu), float(thetas[q]), habs)
                    hi = float(ref)
                    got = seen[habs] = (hi, float(ref - mp.mpf(hi)), float(band))
                T.hi[i, j], T.lo[i, j], T.band[i, j] = got
                T.has[i, j] = True
    return T


# ----------------------------------------------------------------------------- the kernel's arithmetic in libm (host checks)
def spline_grad_rule(u2, theta):
    """csrc/ccgp_internal.h spline_corr_grad's derivative, statement by statement."""
    u = math.sqrt(u2) if u2 == u2 else u2
    if u <= 0.5:
        return (12.0 * u * u - 18.0 * u * u * u) / theta
    if u <= 1.0:
        v = 1.0 - u
        return 6.0 * u * v * v / theta
    return 0.0 if u > 1.0 else u


def matern_grad_rule(nu, z2, theta):
    """csrc/ccgp_internal.h matern_corr_grad's derivative, statement by statement, in libm arithmetic (the value's sum, which
    shares the loop on the device, does not enter it); takes z^2 as the kernel does."""
    if not z2 > SWITCH_Z2:
        return 0.0 if z2 == z2 else z2
    z = math.sqrt(z2)
    hs = 0.15 / max(1.0, math.sqrt(z))
    num = nu - 1.0
    sd = 0.5
    for k in range(1, 6000):
        t = k * hs
        et = math.exp(t)
        c1 = 0.5 * (et + 1.0 / et) - 1.0
        g = 0.5 * (math.exp(num * t - z * c1) + math.exp(-num * t - z * c1))
        sd += g
        if g < 1e-17 * sd and num * t < z * c1:
            break
    norm = 1.0 / (math.gamma(nu) * 2.0 ** (nu - 1.0))
    e, fac = (nu + 1.0) * math.log(z) - z, (hs * sd * norm) / theta
    # below e = -700 the exponent is raised by 64 and exp(-64) goes into the factor: one rounding to a subnormal
    return math.exp(e + 64.0) * (fac * 1.6038108905486378e-28) if e < -700.0 else math.exp(e) * fac


def series_grad(nu, z2, theta):
    """What differentiating matern_corr's two-term series 1 - z^2 / (4 (nu - 1)) would give: z^2 / (2 (nu - 1) theta).  NOT
    what the kernel does: at nu = 1.5 it is off by a relative z."""
    return z2 / (2.0 * (nu - 1.0) * theta)


# ----------------------------------------------------------------------------- the closed-form gradient of a family
def family_grad_from_parts(parts, row, K, Dc, sigma2, dband=None):
    """(grad, scale, extra) of the profiled log-likelihood with respect to the C-ABI row (w_1 .. w_K, theta_1 .. theta_K) of a
    1-D family, in the dtype of parts (oracle.loglik_grad_parts(..., Rc=...)):
        d / d w_q     = 2 sigma2 w_q   sum_ab M_ab R_q,ab
        d / d theta_q =   sigma2 w_q^2 sum_ab M_ab D_q,ab,          D_q = d R_q / d theta_q (Dc: K arrays in that dtype)
    scale[j] is the cancellation-free size sum_ab |M_ab| |d Sigma_ab / d row_j|; extra[j] (theta columns, where dband gives the
    K arrays of the entries' bands) is sigma2 w_q^2 sum_ab |M_ab| dband_q,ab: what the derivative entries' own band moves."""
    M, Rc = parts["M"], parts["Rc"]
    dtype = M.dtype.type
    aM = np.abs(M)
    w = np.asarray(row[:K], dtype=np.float64)
    s2 = dtype(sigma2)
    grad, scale, extra = np.zeros(2 * K, dtype=dtype), np.zeros(2 * K, dtype=dtype), np.zeros(2 * K, dtype=dtype)
    for q in range(K):
        dw = dtype(2) * s2 * dtype(w[q]) * Rc[q]
        grad[q], scale[q] = (M * dw).sum(), (aM * np.abs(dw)).sum()
        dt = (s2 * dtype(w[q]) ** 2) * Dc[q]
        grad[K + q], scale[K + q] = (M * dt).sum(), (aM * np.abs(dt)).sum()
        if dband is not None:
            extra[K + q] = (s2 * dtype(w[q]) ** 2) * (aM * np.asarray(dband[q], dtype=dtype)).sum()
    return grad, scale, extra
