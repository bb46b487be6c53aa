"""Reference for ccgp_loo_batch / ccgp_loo_summary -- leave-one-out cross-validation of the Combined GP in closed form --
shared by tests/test_loo_ref.py (host) and tests/test_gpu_loo.py (device).  Nothing here runs on the device.

The closed form (Dubrule 1983), in long double from oracle._chol_inverse of the normalised mixed matrix R (built from
oracle.component_corr, or for the 1-D families from the exact entries of tests/family_exact.py passed as Rc):
    v1 = R^-1 1,  v2 = 1'v1,  beta = v1'y / v2,  a = R^-1 (y - beta 1),  Q = (y - beta 1)'a
    g_i = (R^-1)_ii,  c_i = g_i - v1_i^2 / v2
    mean_i = y_i - a_i / c_i
    var_i  = sigma2 / c_i                          ORDINARY   (predict.post on the n - 1 other points, HX:669)
           = sigma2 / g_i                          PLUGIN     (mlegp's se.fit^2)
           = (Q - a_i^2 / c_i) / (n - 2) / c_i     UNBIASED   (D1:504-516 on n - 1 points)
tests/test_loo_ref.py holds all of them to long-double predict.post on every subset.

The bands.  unit = eps cond1(R) (1 + rho): an entry of R^-1 computed in fp64 from kernel values that carry a relative error
eps (1 + rho) each -- rho the size of the expanded exponent's terms (oracle.expanded_form_magnitude), for the 1-D families the
largest band / (eps |entry|) of tests/family_exact.py (tests/test_gpu_family_end_to_end._rho) -- is off by about
cond1(R) eps (1 + rho) of its own size, and so is every sum of such entries relative to the sum of their absolute values.
The cancellation-free sizes, with s_i = sum_j |R^-1_ij| and S = sum_i s_i:
    sz_beta = sum_i |v1_i / v2| |y_i|                                        (oracle.loglik_beta_scales)
    sz_a_i  = sum_j |R^-1_ij| (|y_j| + |beta|) + s_i sz_beta
    sz_c_i  = g_i + 2 |v1_i| s_i / v2 + v1_i^2 S / v2^2
    sz_Q    = |y - beta 1|'|R^-1||y - beta 1|
and from them to first order, C = oracle.PREDICT_TOL_C:
    mean      C unit (sz_a_i / c_i + |a_i| sz_c_i / c_i^2)
    ORDINARY  C unit sigma2 sz_c_i / c_i^2
    PLUGIN    C unit sigma2 / g_i
    UNBIASED  the ORDINARY band at sigma2 = (Q - a_i^2 / c_i) / (n - 2), plus
              C unit (sz_Q + 2 |a_i| sz_a_i / c_i + a_i^2 sz_c_i / c_i^2) / ((n - 2) c_i)
    beta      C unit sz_beta          Q    C unit sz_Q
(the last two are not in the tables; the entry points return them, so they are held the same way).  No floor."""
import functools

import numpy as np

from oracle import ccgp_oracle as orc

EPS = float(np.finfo(np.float64).eps)
C = orc.PREDICT_TOL_C
KAPPA_MAX = 1e8
ORDINARY, PLUGIN, UNBIASED = 0, 1, 2
FORMS = (ORDINARY, PLUGIN, UNBIASED)
FORM_NAMES = {ORDINARY: "ordinary", PLUGIN: "plugin", UNBIASED: "unbiased"}
B = 3
SIGMA2 = 1.3 * 10.0 ** (np.arange(B) - 1.0)      # one per row: a row that read another row's sigma2 misses its band
NU = 2.5

# (n, d, K) of the Gaussian exactness cases of tests/test_gpu_loo.py, route by route
REG_SHAPES = [(2, 1, 1), (14, 3, 2), (50, 9, 2), (64, 4, 2), (65, 2, 2)]


def reg_shapes():
    """REG_SHAPES and the largest n that small_route_loo still sends to the register instance at d = 2, K = 2, taken from the
    mirror of its predicate (tests/test_gpu_gradient_exact.small_reg_inverse_supported)."""
    from test_gpu_gradient_exact import small_reg_inverse_supported
    return REG_SHAPES + [(max(n for n in range(2, 200) if small_reg_inverse_supported(n, 2, 2)), 2, 2)]


BLOCKED_SHAPES = [(97, 56, 8), (129, 3, 2), (257, 3, 2)]
# (family, n): Matern(2.5) K = 2 at both sizes, Matern + spline at n = 14 (the closed form on the normalised R only)
FAMILY_CASES = [(1, 14), (1, 129), (2, 14)]


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def closed_form(Rinv, y):
    """The closed form from an inverse, in the inverse's dtype: dict(v1, v2, beta, a, Q, g, c, mean, n)."""
    dtype = Rinv.dtype.type
    yv = np.asarray(y, dtype=dtype).reshape(-1)
    v1 = Rinv.sum(axis=1)
    v2 = v1.sum()
    beta = (v1 @ yv) / v2
    yc = yv - beta
    a = Rinv @ yc
    g = np.diag(Rinv).copy()
    c = g - v1 * v1 / v2
    return dict(v1=v1, v2=v2, beta=beta, a=a, Q=yc @ a, g=g, c=c, mean=yv - a / c, n=yv.shape[0], y=yv)


def variance(cf, form, sigma2=None):
    """The form's variance [n] in cf's dtype; UNBIASED takes no sigma2."""
    dtype = cf["c"].dtype.type
    if form == PLUGIN:
        return dtype(sigma2) / cf["g"]
    if form == UNBIASED:
        return (cf["Q"] - cf["a"] ** 2 / cf["c"]) / dtype(cf["n"] - 2) / cf["c"]
    return dtype(sigma2) / cf["c"]


def mixed_matrix(X, row, K, dtype=np.longdouble, Rc=None):
    """R = sum_c w_c^2 R_c / sum_c w_c^2 in dtype; Rc: the component matrices of another family than the Gaussian."""
    dtype = np.dtype(dtype).type
    X = np.asarray(X, dtype=np.float64)
    w, Th = orc.unpack_params(row, K, X.shape[1])
    w2 = np.asarray(w, dtype=dtype) ** 2
    R = np.zeros((X.shape[0], X.shape[0]), dtype=dtype)
    for c in range(K):
        R += w2[c] * (orc.component_corr(X, Th[c], dtype) if Rc is None else Rc[c])
    return R / w2.sum()


def reference(X, y, row, K, Rc=None, rho=None):
    """One draw in long double: closed_form's dict plus R, Rinv, cond1 and rho."""
    orc.require_extended_precision()
    R = mixed_matrix(X, row, K, np.longdouble, Rc)
    Rinv, _ = orc._chol_inverse(R, np.longdouble)
    ref = closed_form(Rinv, y)
    ref.update(R=R, Rinv=Rinv, cond1=orc.cond1(R, Rinv),
               rho=orc.expanded_form_magnitude(X, row, K, np.asarray(X).shape[1]) if rho is None else rho)
    return ref


def bands(ref, unit=None):
    """dict(unit, mean[n], sz_a[n], sz_c[n], sz_Q, beta, Q) around reference(); unit: C eps cond1 (1 + rho)
    unless given (tests/test_loo_ref.py passes the long-double unit to hold the closed form to the subsets)."""
    if unit is None:
        unit = C * EPS * ref["cond1"] * (1.0 + ref["rho"])
    A = np.abs(_f64(ref["Rinv"]))
    y, v1, a, g, c = (_f64(ref[k]) for k in ("y", "v1", "a", "g", "c"))
    v2, beta = float(ref["v2"]), float(ref["beta"])
    s = A.sum(axis=1)
    S = float(s.sum())
    sz_beta = float(np.abs(v1 / v2) @ np.abs(y))
    sz_a = A @ (np.abs(y) + abs(beta)) + s * sz_beta
    sz_c = g + 2.0 * np.abs(v1) * s / v2 + v1 * v1 * S / v2 ** 2
    yc = np.abs(y - beta)
    sz_Q = float(yc @ A @ yc)
    return dict(unit=unit, mean=unit * (sz_a / c + np.abs(a) * sz_c / c ** 2), sz_a=sz_a, sz_c=sz_c, sz_Q=sz_Q,
                beta=unit * sz_beta, Q=unit * sz_Q)


def variance_band(ref, bnd, form, sigma2=None):
    """The form's band [n]."""
    a, g, c = (_f64(ref[k]) for k in ("a", "g", "c"))
    unit, n = bnd["unit"], ref["n"]
    if form == PLUGIN:
        return unit * sigma2 / g
    if form == UNBIASED:
        s2 = (float(ref["Q"]) - a * a / c) / (n - 2)
        return unit * s2 * bnd["sz_c"] / c ** 2 + unit * (bnd["sz_Q"] + 2.0 * np.abs(a) * bnd["sz_a"] / c + a * a * bnd["sz_c"] / c ** 2) / ((n - 2) * c)
    return unit * sigma2 * bnd["sz_c"] / c ** 2


def fp64_evaluation(R64, y):
    """The closed form in plain fp64 numpy from an fp64 matrix: LAPACK's Cholesky inverse, then closed_form."""
    Rinv, _ = orc._chol_inverse(np.asarray(R64, dtype=np.float64), np.float64)
    return closed_form(Rinv, np.asarray(y, dtype=np.float64))


# ----------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def gauss_case(n, d, K):
    """(X, y, rows[B]) of a Gaussian shape: the design and conditioned draws of tests/test_gpu_predict_exact.make_case."""
    from test_gpu_predict_exact import make_case
    X, y, P, _ = make_case(n, d, K, 1)
    assert len(P) == B
    for a in (X, y, P):
        a.setflags(write=False)
    return X, y, P


@functools.lru_cache(maxsize=None)
def gauss_reference(n, d, K, b):
    X, y, P = gauss_case(n, d, K)
    ref = reference(X, y, P[b], K)
    assert ref["cond1"] <= KAPPA_MAX, (n, d, K, b, ref["cond1"])
    return ref, bands(ref)


def gauss_fp64_matrix(n, d, K, b):
    """R in fp64 with the exponent in the scripts' expanded form (oracle.corr_matrix), as a correct fp64 implementation has it."""
    X, _, P = gauss_case(n, d, K)
    w, Th = orc.unpack_params(P[b], K, d)
    return orc.mixed_corr_matrix_general(X, w, Th)


@functools.lru_cache(maxsize=None)
def family_case(family, n):
    """(x[n], y[n], rows[2, 4]) of tests/test_gpu_family_end_to_end.make_case."""
    import test_gpu_family_end_to_end as fe
    x, y, rows, _ = fe.make_case(family, n)
    return x, y, rows


@functools.lru_cache(maxsize=None)
def family_reference(family, n, b):
    """(ref, bands, R in fp64 from the exact entries rounded to fp64) of one draw of a 1-D family."""
    import test_gpu_family_end_to_end as fe
    x, y, rows = family_case(family, n)
    gram = fe._component_tables(family, rows[b], x, x)
    val, band = fe._mix(rows[b], gram)
    off = band * (1.0 - np.eye(n))                         # the device's diagonal is exactly 1
    ref = reference(x[:, None], y, rows[b], 2, Rc=[T.longdouble() for T in gram], rho=fe._rho(off, val))
    assert ref["cond1"] <= KAPPA_MAX, (family, n, b, ref["cond1"])
    return ref, bands(ref), val
