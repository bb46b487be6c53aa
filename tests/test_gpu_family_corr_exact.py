"""The Matern and cubic-spline correlations of the 1-D scripts (CCGP_KERNEL_MATERN, CCGP_KERNEL_MATERN_SPLINE: cov_kernel<1>,
matern_corr and spline_corr of csrc/ccgp_internal.h) against an exact reference, entry by entry, out of the C ABI:
ccgp_corr_matrix, ccgp_corr_cross, ccgp_mixed_corr_matrix, ccgp_mixed_corr_cross.

Reference and bands: tests/family_exact.py (mpmath at 40 digits on the fp64 inputs as exact rationals; Matern (5e-14 + 4 eps z)
ref, spline 4 eps (A(u) + |u f'(u)|), mixes the w^2-weighted sum + 2 eps |ref|; component-wise, no condition number, no floor
apart from two quanta on subnormal references).  Nothing in a band comes from a device run.  tests/test_family_corr_host.py
runs the same cases against the kernel's arithmetic restated in libm, without a GPU.

Cases (the smallest at which each thing can go wrong):
  sweep   one site at the origin through ccgp_corr_cross, X a column of h: every nu of family_exact.NUS (ccgp_set_kernel accepts
          1 < nu <= 10), 150 z log-spaced over [1e-9, 800], both sides of every switch of the rule (3e-10, 1e-5, 1), z = 300,
          700, 740, a subnormal value; z = 1e4 exactly 0, h = 0 exactly 1; two theta a factor 1000 apart.
  near    n = 14 with pairs 1e-7 and 1e-4 apart, design offsets 0 and 10, theta in (0.5, 0.05, 0.01): every diagonal entry
          exactly 1, every entry the bits of its transpose.
  tile    x_i = i / 128, n in (1, 63, 64, 65, 130) (64 x 64 tiles, 16 columns per wave), sites on the half grid with m in
          (1, 65): |h| is exact and the cross blocks are not symmetric, so a transposed or shifted tile fails.
  nan     one NaN coordinate in X, then in Xnew: the row and the column it touches NaN, everything else inside its band.
          (With weights (0, 1) the Matern component's NaN reaches the entry too: the spline's own propagation is held by
          tests/test_family_corr_host.py on spline_corr's restatement.)
  branch  the spline at, 1 ulp below and 1 ulp above u = 1/2 and u = 1, u = 0, and u = 1 + 8 eps exactly 0.

Measured on an MI355X (test_zz_report_headroom prints it; largest |dev - ref| / band, limit 1): Matern 0.33, Matern mix
0.13, Matern + spline 0.20 (the un-normalised cross rows 0.032), spline 0.10.  The same module on the kernel as it was
before -- the expanded distance of the Gaussian scripts with its clamps, the two-term series below z = 1e-6 -- gave: sweep
4.1e4 at nu = 1.0001, 305 at nu = 1.01, 2.2 at nu = 1.1 (all just below z = 1e-6); near 3.8e3 at offset 0 and 1.0e6 at offset
10 (theta = 0.01; the spline alone 5.2e5), diagonal entries of 1 - 2.4e-12 at offset 0, and an entry of exactly 1.0 where
the reference is 1 - 1.7e-10; tile 4 - 16 on the mixes (their diagonal is not 1); and 1.0 in place of every NaN.

Cost: the references of the whole module take about 12 s of host time (4800 40-digit Bessel evaluations, cached by
(nu, theta, |h|)); test_zz_report_headroom asserts REFERENCE_SECONDS_MAX = 30.  No fixture is needed at that cost.
"""
import time

import numpy as np
import pytest

import family_exact as fx

pytestmark = pytest.mark.gpu

MAX_RATIO = {}                      # what is held -> largest |dev - ref| / band seen
REFERENCE_SECONDS = [0.0]           # host time spent on references by this module
REFERENCE_SECONDS_MAX = 30.0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _reference(case):
    t0 = time.perf_counter()
    T = case.reference()
    REFERENCE_SECONDS[0] += time.perf_counter() - t0
    return T


def device_block(handle, case):
    """The block of `case` out of the C ABI: [rows, columns]."""
    from ccgp_amd import api
    X = case.X[:, None]
    try:
        handle.set_kernel(api.KERNEL_MATERN if case.family == 1 else api.KERNEL_MATERN_SPLINE, case.nu)
        if case.K == 1:
            return handle.corr_matrix(X, case.thetas) if case.Xnew is None else handle.corr_cross(case.Xnew[:, None], X, case.thetas)
        if case.Xnew is None:
            return handle.mixed_corr_matrix(X, 2, case.row())
        return handle.mixed_corr_cross(case.Xnew[:, None], X, 2, case.row())
    finally:
        handle.set_kernel(api.KERNEL_GAUSS, 0.0)


def check(handle, case, nan_rows=(), nan_cols=()):
    """Every entry with a reference inside its band; the rows and columns of a NaN coordinate NaN, and nothing else."""
    T = _reference(case)
    dev = np.asarray(device_block(handle, case))
    assert dev.shape == T.hi.shape, (case.id, dev.shape)
    want_nan = np.zeros(dev.shape, dtype=bool)
    want_nan[list(nan_rows), :] = True
    want_nan[:, list(nan_cols)] = True
    assert np.array_equal(want_nan, ~T.has), case.id
    assert np.array_equal(np.isnan(dev), want_nan), (case.id, np.argwhere(np.isnan(dev) != want_nan)[:6].tolist())
    worst, bad = fx.worst_ratio(dev, T)
    print("%-44s %5d entries, largest |d| / band %.3g" % (case.id, int(T.has.sum()), worst))
    MAX_RATIO[case.tag()] = max(MAX_RATIO.get(case.tag(), 0.0), worst)
    assert not bad, (case.id, len(bad), bad[:6])
    return dev


# ----------------------------------------------------------------------------- 1. domain sweep
@pytest.mark.parametrize("case", fx.sweep_cases(), ids=lambda c: c.id)
def test_matern_domain_sweep(handle, case):
    dev = check(handle, case)[0]
    assert dev[-1] == 1.0, dev[-1]                       # h = 0
    assert dev[-2] == 0.0, dev[-2]                       # z = 1e4
    assert 0.0 < dev[-3] < 2.3e-308, dev[-3]             # the subnormal value is neither flushed nor normal


# ----------------------------------------------------------------------------- 2. near-coincident points, offsets
@pytest.mark.parametrize("case", fx.near_cases(), ids=lambda c: c.id)
def test_near_coincident_points_and_offsets(handle, case):
    dev = check(handle, case)
    assert (np.diag(dev) == 1.0).all(), (case.id, np.abs(np.diag(dev) - 1.0).max())
    assert np.array_equal(_bits(dev), _bits(dev.T)), case.id


# ----------------------------------------------------------------------------- 3. tile indexing
@pytest.mark.parametrize("case", fx.tile_cases(), ids=lambda c: c.id)
def test_tile_indexing(handle, case):
    dev = check(handle, case)
    if case.Xnew is None:
        assert (np.diag(dev) == 1.0).all() and np.array_equal(_bits(dev), _bits(dev.T)), case.id


# ----------------------------------------------------------------------------- 4. NaN
@pytest.mark.parametrize("case,rows,cols", fx.nan_cases(), ids=lambda v: v.id if isinstance(v, fx.Case) else "")
def test_nan_coordinate_propagates(handle, case, rows, cols):
    check(handle, case, rows, cols)


# ----------------------------------------------------------------------------- 5. spline branches
@pytest.mark.parametrize("case", fx.spline_branch_cases(), ids=lambda c: c.id)
def test_spline_branches(handle, case):
    dev = check(handle, case)[0]
    assert dev[0] == 1.0 and dev[-1] == 0.0, (dev[0], dev[-1])


def test_zz_report_headroom():
    """Largest |dev - ref| / band per family over the module, and the host time the references took."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-22s %.3g" % (k, MAX_RATIO[k]))
    print("references: %.1f s of host time, %d Bessel evaluations" % (REFERENCE_SECONDS[0], fx.EVALS["besselk"]))
    assert REFERENCE_SECONDS[0] <= REFERENCE_SECONDS_MAX
