"""The Gaussian correlations (CCGP_KERNEL_GAUSS: cov_kernel<0>, the dense launch of csrc/cov.hip, with cov_mix_term and the
table-driven exp_cov) against an exact reference, entry by entry, out of the C ABI: ccgp_corr_matrix, ccgp_corr_cross,
ccgp_mixed_corr_matrix, ccgp_mixed_corr_cross -- what every script that is not 1-D calls.

Reference and bands: tests/gauss_exact.py (mpmath at 40 digits on the fp64 inputs as exact rationals, the DIRECT form
sum_c w_c^2 exp(-sum_k theta_ck (a_ik - b_jk)^2) / sum_c w_c^2; per entry and component M_c = sum_k theta_ck (|a_ik| + |b_jk|)^2,
delta_c = 2 (d + 4) u M_c, band = sum_c w_c^2 r_c (expm1(delta_c) + 4 u) / sum w^2 + (2 K + 4) u |ref|, u = 2^-53, two quanta on a
subnormal reference; delta_c = 0 where the expanded distance is exact).  Nothing in a band comes from a device run;
tests/test_gauss_corr_host.py runs the same cases against the kernel's arithmetic restated in numpy, without a GPU.

Cases (the smallest at which each thing can go wrong: 64 x 64 tiles, lane = row, 16 columns per wave):
  tile      x_ik dyadic, rates powers of two (the expanded distance is exact: a few ulp of band), n in (1, 63, 64, 65, 130), cross
            blocks (m, n) in ((1, 130), (65, 1), (65, 63), (130, 65)) with sites on the half grid, d in (1, 2), K in (1, 2): here,
            and only here, the diagonal is exactly 1 and the bits equal the transpose's.
  wide      n = 20, m = 7, (d, K) in ((9, 3), (22, 2), (64, 8), (64, 1)), rates log-uniform in [0.005, 1.5]; (64, 8) is the LDS
            carve above 64 KiB.
  near      n = 14, d = 2, pairs 1e-7 and 0 apart, offsets 0 and 10, theta in (0.01, 0.5, 200): the diagonal is exp(-rounding)
            as in R, inside its band, and entries exceed 1 only by their band.  No symmetry is asserted.
  range     one site at the origin against a column of h through ccgp_corr_cross, arguments log-spaced over [1e-9, 745], then
            708, 710, 740 (subnormal: neither flushed nor normal), 750 and 1e4 (exactly 0), h = 0 (exactly 1); mixes with rates
            a factor 1000 apart in both orders (one component underflowed, the other not) and a zero weight on either.
  nan       one NaN coordinate in X, then in Xnew: exactly the row and the column it touches NaN.
  wrappers  CombinedGP("HX") corr_matrix_ISO, corr_vec_ISO, Mixed_corr_matrix, Mixed_corr_vec and CombinedGP("ANI") corr_matrix,
            corr_vec, Mixed_corr_matrix, Mixed_corr_vec on a near and a tile design: the bits of the C-ABI call each wraps,
            with the row written out by hand (argument order, ISO broadcasting).

Measured on an MI355X (test_zz_report_headroom prints it; largest |dev - ref| / band, limit 1):
    tile 0.31, wide 0.083, near 0.17, range 0.5 (one quantum against the two allowed, at argument 745 of a mix whose reference
    is 0.39 quanta; 0.17 elsewhere), nan 0.14, wrappers 0.17.
The restatement of tests/test_gauss_corr_host.py gives 0.28, 0.082, 0.17, 0.5, 0.085 for the first five groups: the device does what
the statements say.  No entry left its band, every NaN pattern was exact, and no kernel was changed for this module.

Mutation check (not committed; four one-line mutants of the library, this module and tests/test_gpu_rinv_helpers_exact.py on
each, beside test_corr_kernels_qian, test_corr_kernels_aniso and the two helper tests of tests/test_gpu_parity.py):
  the store's column index off by one           72 tests here fail       the older tests fail too (qian, aniso, predict.post)
  a distance clamped at 0 in cov_mix_term       the 6 nan tests fail     all four older tests pass
  exp_cov's index floor at -700 (a fifth)       the 6 range tests fail   all four older tests pass
The clamp moves no finite entry out of its band -- it pulls entries whose expanded distance rounds negative back to 1 -- but
fmax swallows the NaN: 1.0 comes back in place of every NaN.

Cost: the references of the whole module take 0.6 s of host time (12 560 40-digit exponentials, cached by argument; the dyadic
designs repeat their distances); test_zz_report_headroom asserts REFERENCE_SECONDS_MAX = 30.
"""
import time

import numpy as np
import pytest

import gauss_exact as gx

pytestmark = pytest.mark.gpu

MAX_RATIO = {}                      # group -> largest |dev - ref| / band seen
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
    if case.single:
        return handle.corr_matrix(case.X, case.Theta[0]) if case.Xnew is None else handle.corr_cross(case.Xnew, case.X, case.Theta[0])
    if case.Xnew is None:
        return handle.mixed_corr_matrix(case.X, case.K, case.row())
    return handle.mixed_corr_cross(case.Xnew, case.X, case.K, case.row())


def check(handle, case, nan_rows=(), nan_cols=()):
    """The shape; the rows and columns of a NaN coordinate NaN, and nothing else; every other entry inside its band."""
    T = _reference(case)
    dev = np.asarray(device_block(handle, case))
    assert dev.shape == T.hi.shape, (case.id, dev.shape)
    want_nan = np.zeros(dev.shape, dtype=bool)
    want_nan[list(nan_rows), :] = True
    want_nan[:, list(nan_cols)] = True
    assert np.array_equal(want_nan, ~T.has), case.id
    assert np.array_equal(np.isnan(dev), want_nan), (case.id, np.argwhere(np.isnan(dev) != want_nan)[:6].tolist())
    worst, bad = gx.worst_ratio(dev, T)
    print("%-40s %5d entries, largest |d| / band %.3g" % (case.id, int(T.has.sum()), worst))
    MAX_RATIO[case.group] = max(MAX_RATIO.get(case.group, 0.0), worst)
    assert not bad, (case.id, len(bad), bad[:6])
    return dev, T


# ----------------------------------------------------------------------------- 1. tile indexing
@pytest.mark.parametrize("case", gx.tile_cases(), ids=lambda c: c.id)
def test_tile_indexing(handle, case):
    dev, _ = check(handle, case)
    if case.Xnew is None:
        assert (np.diag(dev) == 1.0).all(), (case.id, np.abs(np.diag(dev) - 1.0).max())
        assert np.array_equal(_bits(dev), _bits(dev.T)), case.id


# ----------------------------------------------------------------------------- 2. wide designs, many components
@pytest.mark.parametrize("case", gx.wide_cases(), ids=lambda c: c.id)
def test_wide_designs_and_many_components(handle, case):
    check(handle, case)


# ----------------------------------------------------------------------------- 3. near-coincident points, offsets
@pytest.mark.parametrize("case", gx.near_cases(), ids=lambda c: c.id)
def test_near_coincident_points_and_offsets(handle, case):
    dev, T = check(handle, case)
    i = np.arange(dev.shape[0])
    assert (np.abs(dev[i, i] - 1.0) <= T.band[i, i]).all() and (T.hi[i, i] == 1.0).all(), case.id      # exp(-rounding), as in R
    assert ((dev - 1.0) <= T.band).all(), (case.id, float((dev - 1.0 - T.band).max()))


# ----------------------------------------------------------------------------- 4. the range of the argument
@pytest.mark.parametrize("case", gx.range_cases(), ids=lambda c: c.id)
def test_argument_range_down_to_underflow(handle, case):
    dev = check(handle, case)[0][0]
    assert dev[-1] == 1.0, dev[-1]                                       # h = 0
    assert (dev[-3:-1] == 0.0).all(), dev[-3:-1]                         # arguments 750 and 1e4
    assert 0.0 < dev[gx.RANGE_SUBNORMAL] < gx.TINY, dev[gx.RANGE_SUBNORMAL]          # neither flushed nor normal


# ----------------------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize("case,rows,cols", gx.nan_cases(), ids=lambda v: v.id if isinstance(v, gx.Case) else "")
def test_nan_coordinate_propagates(handle, case, rows, cols):
    check(handle, case, rows, cols)


# ----------------------------------------------------------------------------- 6. the R surface's wrappers
def _wrapper_designs():
    return [("near", gx.near_design(10.0), gx.near_design(10.0)[3] + 0.01), ("tile", gx.tile_design(65, 2), gx.tile_sites(3, 2)[2])]


@pytest.mark.parametrize("name,X,x", _wrapper_designs(), ids=lambda v: v if isinstance(v, str) else "")
def test_wrappers_give_the_bits_of_the_calls_they_wrap(handle, name, X, x):
    """corr.matrix.ISO(X, theta) is one rate for every dimension; corr.matrix(X, theta1, theta2) of the anisotropic script one
    per dimension; Mixed.corr.matrix(D, p, theta1, theta2) weights (p, 1 - p) with rates theta1 and theta2 (HX:408-415), and
    (D, p, theta1, theta2, lambda) the rates (theta1, theta2) and (1 + lambda) (theta1, theta2) (ANI:399-406)."""
    from ccgp_amd.rsurface import CombinedGP
    hx, ani = CombinedGP("HX", handle=handle), CombinedGP("ANI", handle=handle)
    p, t1, t2, lam = 0.75, 0.5, 2.0, 3.0
    xs = x[None, :]
    same = lambda a, b: a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    assert same(hx.corr_matrix_ISO(X, t1), handle.corr_matrix(X, np.array([t1, t1])))
    assert same(hx.corr_vec_ISO(x, X, t1), handle.corr_cross(xs, X, np.array([t1, t1]))[0])
    row = np.array([p, 1.0 - p, t1, t1, t2, t2])
    assert same(hx.Mixed_corr_matrix(X, p, t1, t2), handle.mixed_corr_matrix(X, 2, row))
    assert same(hx.Mixed_corr_vec(x, X, p, t1, t2), handle.mixed_corr_cross(xs, X, 2, row)[0])
    assert same(ani.corr_matrix(X, t1, t2), handle.corr_matrix(X, np.array([t1, t2])))
    assert same(ani.corr_vec(x, X, t1, t2), handle.corr_cross(xs, X, np.array([t1, t2]))[0])
    row = np.array([p, 1.0 - p, t1, t2, (1.0 + lam) * t1, (1.0 + lam) * t2])
    assert same(ani.Mixed_corr_matrix(X, p, t1, t2, lam), handle.mixed_corr_matrix(X, 2, row))
    assert same(ani.Mixed_corr_vec(x, X, p, t1, t2, lam), handle.mixed_corr_cross(xs, X, 2, row)[0])
    # and the calls they wrap are held themselves: the two mixes and the two single-component rows of this design
    for tag, w, Th in (("iso", (1.0,), [[t1, t1]]), ("ani", (1.0,), [[t1, t2]]), ("hx-mix", (p, 1.0 - p), [[t1, t1], [t2, t2]]),
                       ("ani-mix", (p, 1.0 - p), [[t1, t2], [(1.0 + lam) * t1, (1.0 + lam) * t2]])):
        check(handle, gx.Case("wrappers", "%s-%s" % (name, tag), w, Th, None, X))
        check(handle, gx.Case("wrappers", "%s-%s-vec" % (name, tag), w, Th, xs, X))


def test_zz_report_headroom():
    """Largest |dev - ref| / band per group over the module, and the host time the references took."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-10s %.3g" % (k, MAX_RATIO[k]))
    print("references: %.1f s of host time, %d 40-digit exponentials" % (REFERENCE_SECONDS[0], gx.EVALS["exp"]))
    assert REFERENCE_SECONDS[0] <= REFERENCE_SECONDS_MAX
