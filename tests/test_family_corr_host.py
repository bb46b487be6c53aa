"""tests/family_exact.py's references and bands, without a GPU: the cases of tests/test_gpu_family_corr_exact.py against the
kernel's arithmetic restated in libm (family_exact.kernel_restatement: the direct difference, tests/test_special.py's
matern_rule, spline_corr's statements), and against the arithmetic the kernel had before -- the expanded distance with
clamps, the two-term series below z = 1e-6 -- which the same bands must reject.  So a band that passes the device is known
to be one that a correct fp64 implementation meets and the earlier one does not."""
import math

import numpy as np
import pytest

import family_exact as fx
from test_special import matern_rule

HOST_NUS = (1.0001, 2.5, 10.0)


def _cases():
    tiles = [c for c in fx.tile_cases() if c.id.split("-")[1] in ("n65", "m65") and "n65" in c.id]
    return fx.sweep_cases(HOST_NUS) + fx.near_cases() + tiles + fx.spline_branch_cases()


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.id)
def test_restated_kernel_is_inside_every_band(case):
    dev = fx.kernel_restatement(matern_rule, case.family, case.nu, case.w, case.thetas, case.rows(), case.X, case.raw)
    worst, bad = fx.worst_ratio(dev, case.reference())
    assert not bad, (case.id, worst, bad[:4])
    if case.group == "sweep":
        assert dev[0, -1] == 1.0 and dev[0, -2] == 0.0 and 0.0 < dev[0, -3] < 2.3e-308
    if case.group == "near":
        assert (np.diag(dev) == 1.0).all() and np.array_equal(dev, dev.T)
    if case.group == "branch":
        assert dev[0, 0] == 1.0 and dev[0, -1] == 0.0


@pytest.mark.parametrize("case,rows,cols", fx.nan_cases(), ids=lambda v: v.id if isinstance(v, fx.Case) else "")
def test_restated_kernel_propagates_nan(case, rows, cols):
    dev = fx.kernel_restatement(matern_rule, case.family, case.nu, case.w, case.thetas, case.rows(), case.X, case.raw)
    T = case.reference()
    want = np.zeros(dev.shape, dtype=bool)
    want[rows, :] = True
    want[:, cols] = True
    assert np.array_equal(np.isnan(dev), want) and np.array_equal(~T.has, want)
    assert not fx.worst_ratio(np.where(want, 0.0, dev), T)[1]
    assert math.isnan(fx.spline_rule(float("nan"))) and math.isnan(matern_rule(2.5, float("nan")))


# ----------------------------------------------------------------------------- what the bands must reject
def _earlier_matern(nu, z2):
    """matern_corr before: the two-term series up to z = 1e-6, clamped."""
    if not z2 > 1e-12:
        return 1.0 - (z2 if z2 > 0.0 else 0.0) / (4.0 * (nu - 1.0))
    return matern_rule(nu, z2)


def _earlier_block(nu, theta, X):
    """cov_kernel<1> before: the Gaussian scripts' expanded distance (u_i + u_j) - 2 (x_i rate) x_j."""
    rate = 4.0 * nu / (theta * theta)
    u = X * X * rate
    return np.array([[_earlier_matern(nu, (u[i] + u[j]) + -2.0 * ((X[i] * rate) * X[j])) for j in range(X.size)] for i in range(X.size)])


def test_bands_reject_the_two_term_series_near_nu_1():
    for nu, least in ((1.0001, 1e4), (1.01, 100.0), (1.1, 1.0)):
        z = 1e-6 * (1.0 - 1e-12)
        h = z * 0.0037 / (2.0 * math.sqrt(nu))
        ref, band, zz = fx.matern(nu, 0.0037, fx.frac(h))
        got = _earlier_matern(nu, float(zz) ** 2)
        assert abs(got - ref) / band > least, (nu, float(abs(got - ref) / band))


def test_bands_reject_the_expanded_distance():
    X = fx.near_coincident_design(10.0)
    T = fx.table(1, 2.5, (1.0,), (0.01,), X, X)
    dev = _earlier_block(2.5, 0.01, X)
    worst, bad = fx.worst_ratio(dev, T)
    assert worst > 1e3 and len(bad) > 14 and np.abs(np.diag(dev) - 1.0).max() > 1e-11, (worst, len(bad))
    assert (np.diag(T.hi) == 1.0).all() and (np.diag(T.band) == 0.0).all()

