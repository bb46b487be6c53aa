"""tests/gauss_exact.py's references and bands, without a GPU: every case of tests/test_gpu_gauss_corr_exact.py and of
tests/test_gpu_rinv_helpers_exact.py against the kernels' arithmetic restated in numpy fp64 (gauss_exact.kernel_restatement:
the expanded distance, the per-component accumulation, the product with 1 / sum w^2; rinv_terms_restatement and
predict_restatement: the 4-way partial sums, the lane accumulators, the shuffle tree, in the kernels' combination order) --
no fused multiply-adds, libm's exp.  So a band that the device must meet is known to be one that correct fp64 arithmetic meets,
with room: test_zz_restatement_headroom asserts that no group needs more than HEADROOM = 0.5 of its band, and prints the largest
|restated - ref| / band per group.  Where a band is wrong, it shows here first.

What the bands must reject is checked here too, on the restatement: a shifted column, a dropped column of R.Inv, a dropped wave
partial, a distance clamped at 0."""
import numpy as np
import pytest

import gauss_exact as gx

HEADROOM = 0.5
MAX_RATIO = {}


def _note(group, worst):
    MAX_RATIO[group] = max(MAX_RATIO.get(group, 0.0), worst)


def _nan_mask(shape, rows, cols):
    want = np.zeros(shape, dtype=bool)
    want[list(rows), :] = True
    want[:, list(cols)] = True
    return want


# ----------------------------------------------------------------------------- correlations
@pytest.mark.parametrize("case", gx.tile_cases() + gx.wide_cases() + gx.near_cases() + gx.range_cases(), ids=lambda c: c.id)
def test_restated_kernel_is_inside_every_band(case):
    dev, T = case.restated(), case.reference()
    assert T.has.all()
    worst, bad = gx.worst_ratio(dev, T)
    print("%-40s %5d entries, largest |d| / band %.3g, band / ref %.3g .. %.3g" % (
        case.id, dev.size, worst, (T.band / np.maximum(T.hi, 1e-300)).min(), (T.band / np.maximum(T.hi, 1e-300)).max()))
    _note(case.group, worst)
    assert not bad, (case.id, worst, bad[:4])
    if case.group == "tile" and case.Xnew is None:
        assert (np.diag(dev) == 1.0).all() and np.array_equal(dev, dev.T)
    if case.group == "near":
        assert ((dev - 1.0) <= T.band).all()
    if case.group == "range":
        assert dev[0, -1] == 1.0 and (dev[0, -3:-1] == 0.0).all() and 0.0 < dev[0, gx.RANGE_SUBNORMAL] < gx.TINY
        assert (T.hi[0, -3:-1] == 0.0).all() and 0.0 < T.hi[0, gx.RANGE_SUBNORMAL] < gx.TINY


@pytest.mark.parametrize("case,rows,cols", gx.nan_cases(), ids=lambda v: v.id if isinstance(v, gx.Case) else "")
def test_restated_kernel_propagates_nan(case, rows, cols):
    dev, T = case.restated(), case.reference()
    want = _nan_mask(dev.shape, rows, cols)
    assert np.array_equal(np.isnan(dev), want) and np.array_equal(~T.has, want)
    worst, bad = gx.worst_ratio(np.where(want, 0.0, dev), T)
    _note("nan", worst)
    assert not bad, (case.id, worst, bad[:4])


def test_case_lists_are_the_sizes_that_matter():
    """the shapes the kernels' structure asks for: 64 x 64 tiles, 16 columns per wave, the LDS carve above 64 KiB"""
    tiles = gx.tile_cases()
    assert {c.X.shape[0] for c in tiles if c.Xnew is None} == {1, 63, 64, 65, 130}
    assert {(c.Xnew.shape[0], c.X.shape[0]) for c in tiles if c.Xnew is not None} == {(1, 130), (65, 1), (65, 63), (130, 65)}
    assert {(c.d, c.K) for c in tiles} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {(c.d, c.K) for c in gx.wide_cases()} == {(9, 3), (22, 2), (64, 8), (64, 1)}
    assert 8 * (256 + 2 * 64 * 64 + 2 * 8 * 64 + 8 * 64 + 8) > 64 * 1024          # cov_lds(64, 8)
    for c in gx.wide_cases():
        assert c.Theta.min() >= 0.005 and c.Theta.max() <= 1.5 and c.X.shape[0] == 20 and c.rows().shape[0] in (7, 20)
    X = gx.near_design(0.0)
    assert (X[7] == X[2]).all() and abs(X[4, 0] - X[1, 0] - 1e-7) < 1e-15 and X[4, 1] == X[1, 1] and X.shape == (14, 2)
    # every tile case is exact in fp64: the restated distance is the reference's argument, bit for bit
    for c in tiles:
        A, B = c.rows(), c.X
        for th in c.Theta:
            direct = sum(th[k] * (A[:, None, k] - B[None, :, k]) ** 2 for k in range(c.d))
            expanded = (((A * A) * th).sum(axis=1)[:, None] + ((B * B) * th).sum(axis=1)[None, :]) - 2.0 * ((A * th) @ B.T)
            assert np.array_equal(direct, expanded), c.id


# ----------------------------------------------------------------------------- what the correlation bands must reject
def test_bands_reject_a_shifted_column_and_a_clamped_distance():
    c = [c for c in gx.tile_cases() if c.id == "tile-m130-n65-d2-K2"][0]
    dev, T = c.restated(), c.reference()
    assert len(gx.worst_ratio(np.roll(dev, 1, axis=1), T)[1]) > 1000 and len(gx.worst_ratio(dev[::-1], T)[1]) > 1000
    # a distance clamped at 0 (fmax) moves no finite entry out of its band -- it only pulls entries whose expanded distance
    # rounds negative back to 1 -- but it swallows every NaN: the NaN cases are what rejects it
    over = sum(int((c.restated() > 1.0).sum()) for c in gx.near_cases())
    assert over > 0, "no near case has an entry whose expanded distance rounds negative"
    for c, rows, cols in gx.nan_cases():
        clamped = gx.kernel_restatement(c.w, c.Theta, c.rows(), c.X, clamp=True)
        assert not np.isnan(clamped).any() and _nan_mask(clamped.shape, rows, cols).any()


# ----------------------------------------------------------------------------- R.Inv helpers
def _check_terms(case, got, group):
    """got = (mean_factor, colsum, beta_mle, sigma2, v2) against case.terms_reference()"""
    ref = case.terms_reference()
    mf, cs, beta, sigma2, v2 = got
    out = {}
    for name, dev in (("mean_factor", mf), ("colsum", cs)):
        worst, bad = gx.worst_ratio(dev, ref[name])
        assert not bad, (case.id, name, worst, bad[:4])
        out[name] = worst
    for name, dev in (("beta_mle", beta), ("sigma2", sigma2), ("v2", v2)):
        out[name] = ref[name].ratio(dev)
        assert out[name] <= 1.0, (case.id, name, dev, ref[name].hi, out[name])
    print("%-12s cond1 %-8s %s" % (case.id, "%.2g" % case.cond if case.cond else "-", "  ".join("%s %.3g" % kv for kv in out.items())))
    _note(group, max(out.values()))


def restated_terms(case):
    _, _, a0, a1, _ = gx.rinv_terms_restatement(case.A, case.y, 0.0)
    mf, cs, _, v2, a2 = gx.rinv_terms_restatement(case.A, case.y, case.beta)
    return mf, cs, a0 / a1, a2 / case.n, v2


@pytest.mark.parametrize("key", gx.HELPER_KEYS, ids=lambda k: "%s-n%d" % k)
def test_restated_helpers_are_inside_every_band(key):
    case = gx.helper_case(*key)
    _check_terms(case, restated_terms(case), "rinv terms")
    mean, var = gx.predict_restatement(case.A, case.r, case.beta, case.mf, case.v1, case.v2, gx.HELPER_SIGMA2)
    Tm, Tv = case.predict_reference()
    for name, dev, T in (("mean", mean, Tm), ("var", var, Tv)):
        worst, bad = gx.worst_ratio(dev, T)
        _note("predict " + name, worst)
        assert not bad, (case.id, name, worst, bad[:4])
    if case.kind == "gauss":
        assert case.n == 1 or 0.3 * gx.HELPER_COND <= case.cond <= 3.0 * gx.HELPER_COND, case.cond
        if case.on is not None and case.n > 1:               # on a training point the exact variance all but vanishes
            assert abs(Tv.hi[case.on]) <= 1e-4 * gx.HELPER_SIGMA2 and Tv.band[case.on] <= 1e-3 * gx.HELPER_SIGMA2
        if case.far is not None:
            assert (case.r[case.far] == 0.0).all()
            assert abs(Tv.hi[case.far] - gx.HELPER_SIGMA2 * (1.0 + 1.0 / case.v2)) <= Tv.band[case.far]
    else:
        assert np.abs(case.A - case.A.T).max() > 0.1 or case.n == 1


def test_helper_case_lists_are_the_sizes_that_matter():
    cases = gx.helper_cases()
    assert {c.n for c in cases} == {1, 3, 4, 5, 63, 64, 65, 129, 257} and {c.m for c in cases} == {1, 5, 65}
    assert {c.kind for c in cases} == {"asym", "gauss"}
    assert any(c.on is not None and c.m == 65 for c in cases) and any(c.far is not None and c.m == 1 for c in cases)


def test_restated_helpers_propagate_nan():
    c = gx.helper_nan_case()
    y = c.y.copy()
    y[gx.NAN_Y] = np.nan
    mf, cs, a0, a1, a2 = gx.rinv_terms_restatement(c.A, y, c.beta)
    assert np.isnan(mf).all() and np.isnan(a0) and np.isnan(a2) and np.isfinite(cs).all() and np.isfinite(a1)
    r = c.r.copy()
    r[gx.NAN_R] = np.nan
    mean, var = gx.predict_restatement(c.A, r, c.beta, c.mf, c.v1, c.v2, gx.HELPER_SIGMA2)
    want = np.arange(c.m) == gx.NAN_R[0]
    assert np.array_equal(np.isnan(mean), want) and np.array_equal(np.isnan(var), want)


def test_helper_bands_reject_a_dropped_column_and_a_dropped_partial():
    """the two planted mistakes of the helpers, on the restatement: rinv_terms_kernel starting its columns at wave + 4 (columns
    0 .. 3 never read) and predict_factors_kernel leaving part[3] out of its combine"""
    for c in (c for c in gx.helper_cases() if c.n in (5, 65, 257)):
        ref = c.terms_reference()
        A4 = c.A.copy()
        A4[:, :4] = 0.0                                      # what the row products see without columns 0 .. 3
        mf = gx.rinv_terms_restatement(A4, c.y, c.beta)[0]
        assert gx.worst_ratio(mf, ref["mean_factor"])[1], c.id
        A3 = c.A.copy()
        A3[:, 3::4] = 0.0                                    # what acc sees without the fourth wave's partial
        _, var = gx.predict_restatement(A3, c.r, c.beta, c.mf, c.v1, c.v2, gx.HELPER_SIGMA2)
        assert gx.worst_ratio(var, c.predict_reference()[1])[1], c.id


# ----------------------------------------------------------------------------- the literal chain
@pytest.mark.parametrize("n", gx.CHAIN_N)
def test_restated_chain_is_inside_the_predict_band(n):
    mean, var, beta = gx.restated_chain(n)
    want_mean, want_var, want_beta, band = gx.chain_reference(n)
    ratios = dict(mean=float((np.abs(mean - want_mean) / band["mean"]).max()), var=float((np.abs(var - want_var) / band["var"]).max()),
                  beta=abs(beta - want_beta) / band["beta"])
    print("chain n = %d: %s" % (n, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    _note("chain", max(ratios.values()))
    assert max(ratios.values()) <= 1.0, (n, ratios)


def test_zz_restatement_headroom():
    """the restatement's largest |restated - ref| / band per group: no more than HEADROOM of any band"""
    for k in sorted(MAX_RATIO):
        print("restatement max ratio %-14s %.3g" % (k, MAX_RATIO[k]))
    assert all(v <= HEADROOM for v in MAX_RATIO.values()), MAX_RATIO
