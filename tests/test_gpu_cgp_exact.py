"""The CGP comparator on the device (ccgp_cgp_state_batch, ccgp_cgp_predict and their sets forms) held to the condition-free
bands and closed forms of tests/cgp_exact.py: checks (b) to (f) a posteriori from the kept state, the jackknife bit for bit
against the design with the row deleted, the lattice closed form (g), and the arguments beyond exp's range.  Nothing in a band
comes from a device run; tests/test_cgp_exact_host.py proves the same bands on the CPU with a factor of two to spare.
test_zz_report_headroom prints the largest fraction of each band the device used; DESIGN.md (K9) records them.
"""
import numpy as np
import pytest

import cgp_exact as cx
from conftest import synthetic_design
from ccgp_amd import cgp

pytestmark = pytest.mark.gpu

SEEN = cx.Tally()


def _inside(t, what):
    SEEN.merge(t)
    assert not t.outside(1.0), (what, t.outside(1.0))


def _bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


# --------------------------------------------------------------------------------------------------- (b) - (f), every shape
@pytest.mark.parametrize("b", [0, 1], ids=["lambda0.001", "lambda1"])
@pytest.mark.parametrize("n,d", cx.CASES)
def test_kept_state_and_predictions_inside_the_bands(handle, n, d, b):
    Xs, y, rows, Xt, on = cx.case(n, d)
    row = rows[b]
    val, beta, tau2, _, st = handle.cgp_state_batch(Xs, y, row[None])
    out, keep, s1 = handle.cgp_predict(Xs, y, row, Xt)
    assert st[0] == 0 and s1 == 0 and np.all(np.isfinite(out))
    assert _bits(keep["beta"], beta[0]) and _bits(keep["tau2"], tau2[0])
    ill = (n, d, float(row[0])) == cx.ILL
    t, p, nans = cx.check_evaluation(Xs, y, row, keep, val[0], Xt, out, {4: on}, logdet=n <= 65 or ill)
    assert not nans
    if ill:
        assert p.cond1() >= 1e6
    print("n %d d %d lambda %g cond1 %.3g: %s" % (n, d, row[0], p.cond1(), t))
    _inside(t, (n, d, b))


# ---------------------------------------------------------------------------------------------------------------- jackknife
@pytest.mark.parametrize("which", [0, 1, 2], ids=["first", "middle", "last"])
@pytest.mark.parametrize("n", cx.JACK_N)
def test_jackknife_is_the_deleted_design_bit_for_bit(handle, n, which):
    """only addresses depend on the full n (the strides of the design and of the working matrix): the sums run over the
    compacted points, so val, beta and tau2 are the plain call's on the design with the row deleted.  loo is summed in another
    order than cgp_predict_kernel's Yp and is held to band (f) from the deleted design's kept state."""
    Xs, y, rows, _, _ = cx.case(n, 2)
    skip = (0, n // 2, n - 1)[which]
    pick = np.arange(n) != skip
    val, beta, tau2, loo, st = handle.cgp_state_batch(Xs, y, rows, skip=np.array([skip, skip]))
    v1, b1, t1, _, s1 = handle.cgp_state_batch(Xs[pick], y[pick], rows)
    assert np.all(st == 0) and np.all(s1 == 0)
    assert _bits(val, v1) and _bits(beta, b1) and _bits(tau2, t1), (val - v1, beta - b1, tau2 - t1)
    b = which % 2
    _, keep, s2 = handle.cgp_predict(Xs[pick], y[pick], rows[b], Xs[skip:skip + 1])
    assert s2 == 0 and _bits(keep["beta"], beta[b]) and _bits(keep["tau2"], tau2[b])
    t = cx.Tally()
    p = cx.Posterior(Xs[pick], y[pick], rows[b], keep)
    p.check_solve(t)
    p.check_tau2(t)
    cx.loo_check(t, p, Xs[skip], loo[b])
    print("n %d skip %d lambda %g: %s" % (n, skip, rows[b, 0], t))
    _inside(t, (n, skip))


# -------------------------------------------------------------------------------------------------------------- closed form
def _lattice_run(handle, lc, Xt):
    skip = None if lc.skip < 0 else np.array([lc.skip])
    val, beta, tau2, loo, st = handle.cgp_state_batch(lc.X, lc.y, lc.row[None], skip=skip)
    out, keep, s1 = handle.cgp_predict(lc.Xe, lc.ye, lc.row, Xt)
    assert st[0] == 0 and s1 == 0
    if lc.skip < 0:
        assert _bits(keep["beta"], beta[0]) and _bits(keep["tau2"], tau2[0])
    return dict(val=val[0], beta=beta[0], tau2=tau2[0], loo=None if loo is None else loo[0], keep=keep if lc.skip < 0 else None), out


@pytest.mark.parametrize("skip", [-1, 2], ids=["plain", "heldout"])
@pytest.mark.parametrize("variant", cx.VARIANTS)
@pytest.mark.parametrize("n", [9, 65])
def test_lattice_closed_form(handle, n, variant, skip):
    lc = cx.LatticeCase(n, variant, skip)
    Xt = lc.sites()
    dev, out = _lattice_run(handle, lc, Xt)
    t = cx.Tally()
    cx.lattice_check(t, lc, dev, Xt, out)
    print("n %d %s skip %d: %s" % (n, variant, skip, t))
    _inside(t, (n, variant, skip))


@pytest.mark.parametrize("distance", [1e60, np.inf], ids=["1e60", "inf"])
def test_arguments_beyond_the_range_of_exp_give_zero(handle, distance):
    """Base R has exp(-1e60) = exp(-Inf) = 0, so a lattice whose off-diagonal distances are 1e60 or +Inf has the matrices of the
    rates-of-1000 lattice and must have its outputs bit for bit.  No product on the way to a distance is NaN: the differences
    are 0 or at least 1.5, the rates are finite, bw = 1."""
    n = 9
    base = cx.LatticeCase(n, "gbw_identity")
    rate = 1e308 if np.isinf(distance) else distance / cx.LATTICE_STEP ** 2
    far = cx.LatticeCase(n, "gbw_identity", rate=rate)
    with np.errstate(over="ignore"):
        D = ((far.X[:, None, :] - far.X[None, :, :]) ** 2 * rate).sum(-1)
    off = D[~np.eye(n, dtype=bool)]
    assert off.min() >= distance and not np.isnan(D).any() and np.all(np.diag(D) == 0)
    Xt = base.sites()
    want, want_out = _lattice_run(handle, base, Xt)
    got, got_out = _lattice_run(handle, far, Xt)
    for k in ("val", "beta", "tau2"):
        assert _bits(got[k], want[k]), (k, got[k], want[k])
    for k in ("s", "res2", "temp", "sf"):
        assert _bits(got["keep"][k], want["keep"][k]), k
    assert np.array_equal(got_out, want_out, equal_nan=True), (got_out, want_out)
    skip = np.array([2])
    a = handle.cgp_state_batch(base.X, base.y, base.row[None], skip=skip)
    c = handle.cgp_state_batch(far.X, far.y, far.row[None], skip=skip)
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, c))


# --------------------------------------------------------------------------------------------------------------- sets forms
def test_sets_forms_inside_the_bands(handle):
    n, d = 65, 2
    Xs, y, rows, Xt, on = cx.case(n, d)
    X2, y2 = synthetic_design(n, d, 4242)
    X2, _ = cgp.standardise(X2)
    rows2 = cx.rows_in_the_box(X2, 2, 99)
    Xt2 = np.random.default_rng(5).random((7, d))
    Xt2[4] = X2[7]
    designs, ys, sites = np.stack([Xs, X2]), np.stack([y, y2]), np.stack([Xt, Xt2])
    params, set_of = np.stack([rows[0], rows2[1]]), np.array([0, 1], dtype=np.int32)
    val, beta, tau2, _, st = handle.cgp_state_batch_sets(designs, ys, params, set_of)
    out, keeps, s1 = handle.cgp_predict_sets(designs, ys, params, set_of, sites)
    assert np.all(st == 0) and np.all(s1 == 0)
    for b, onb in ((0, on), (1, 7)):
        assert _bits(keeps[b]["beta"], beta[b]) and _bits(keeps[b]["tau2"], tau2[b])
        t, _, nans = cx.check_evaluation(designs[b], ys[b], params[b], keeps[b], val[b], sites[b], out[b], {4: onb})
        assert not nans
        print("set %d: %s" % (b, t))
        _inside(t, ("sets", b))


def test_zz_report_headroom():
    print("largest fraction of each band used by the device: %s" % SEEN)
    assert SEEN.worst() <= 1.0
