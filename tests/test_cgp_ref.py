"""Host checks of the CGP comparator (tests/cgp_ref.py, ccgp_amd.cgp): the restatement against the reference's recorded
table, fp64 against long double, and the fit routine on the host stand-in for the device handle."""
import os

import numpy as np
import pytest

import cgp_ref
from conftest import DATA, golden, load_gv, load_maximin
from ccgp_amd import cgp
from ccgp_amd.tables import read_table


def recorded_cgp():
    names, res = read_table(os.path.join(DATA, "gv", "results_50_1.txt"))
    col = {n: i for i, n in enumerate(names)}
    return res[:, :9], res[:, [col["y.hat.CGP"], col["LL.CGP"], col["UL.CGP"]]]


def test_restatement_reproduces_the_recorded_cgp_columns():
    """predict.CGP at the recovered fit (tests/golden/recover_cgp_gv.py) against the 150 x 3 recorded numbers."""
    fx = golden("gv_cgp_recovered.json")
    D, y, _, _ = load_gv(50)
    Dt, rec = recorded_cgp()
    out, st = cgp_ref.predict(D, y, fx["row"], Dt)
    resid = float(np.abs(out[:, [0, 4, 5]] - rec).max())
    print("largest residual against the recorded table: %.3g" % resid)
    assert st["status"] == 0 and resid <= 1e-10
    # the fixture is what it says: the standardised vector back-transforms to the row, variables off `free` sit on a bound,
    # and the objective is var.MLE.DK on the standardised design
    ww, lo, hi = (np.array(fx[k]) for k in ("ww", "lower", "upper"))
    Xs, scales = cgp.standardise(D)
    row = cgp.rows_from_ww(ww)[0]
    np.testing.assert_allclose(np.concatenate([[row[0]], row[1:10] / scales ** 2, row[10:19] / scales ** 2, [row[19]]]),
                               fx["row"], rtol=1e-15)
    l2, h2 = cgp.bounds(Xs)
    np.testing.assert_allclose(l2, lo, rtol=1e-14)
    np.testing.assert_allclose(h2, hi, rtol=1e-14)
    fixed = np.setdiff1d(np.arange(12), fx["free"])
    assert np.all((ww[fixed] == lo[fixed]) | (ww[fixed] == hi[fixed])) and np.all((ww >= lo) & (ww <= hi))
    assert float(cgp_ref.state(Xs, y, row)["val"]) == pytest.approx(fx["objective"], abs=1e-9)


@pytest.mark.parametrize("lam", [0.001, 1.0])
def test_fp64_against_long_double(lam):
    """The fp64 restatement's own error, per output, on the Ground-Vibrations set: inside the band the device is held to."""
    fx = golden("gv_cgp_recovered.json")
    D, y, Dt, _ = load_gv(50)
    row = np.array(fx["row"])
    row[0] = lam
    worst = {}
    for skip in (-1, 0, 17, 49):
        a, b = cgp_ref.state(D, y, row, skip, np.float64), cgp_ref.state(D, y, row, skip, np.longdouble)
        pa = pb = None
        if skip < 0:
            pa, pb = cgp_ref.predict(D, y, row, Dt[:20], np.float64, a)[0], cgp_ref.predict(D, y, row, Dt[:20], np.longdouble, b)[0]
        sc, c1 = cgp_ref.scales(b, y, pb), cgp_ref.cond1(b)
        errs = {k: abs(float(a[k] - b[k])) for k in (("val", "beta", "tau2") + (("loo",) if skip >= 0 else ()))}
        if pa is not None:
            errs.update({k: float(np.abs(pa[:, i] - pb[:, i]).max()) for i, k in enumerate(cgp_ref.COLS)})
        for k, e in errs.items():
            frac = e / cgp_ref.band(b["n"], c1, sc[k])
            worst[k] = max(worst.get(k, 0.0), frac)
            assert frac <= 1.0, (k, skip, e, frac)
    print("lambda %g: largest fraction of the band fp64 uses: %s" % (lam, {k: "%.3g" % v for k, v in worst.items()}))


def smooth(D):
    return np.sin(3.0 * D[:, 0]) + np.cos(2.0 * D[:, 1]) * D[:, 0] + 0.5 * D[:, 1] ** 2


@pytest.fixture(scope="module")
def fit14():
    D = load_maximin(14)
    y = smooth(D)
    h = cgp_ref.NumpyHandle()
    est = cgp.CGP(h, D, y, rng=3)
    h.calls_of_fit, h.points_of_fit = h.calls, h.points
    return D, y, h, est


def test_fit_is_no_worse_than_its_starts_and_stays_in_the_box(fit14):
    D, y, h, est = fit14
    Xs, _ = cgp.standardise(D)
    f0 = np.array([float(cgp_ref.state(Xs, y, r)["val"]) for r in cgp.rows_from_ww(est["starts"])])
    assert est["starts"].shape == (5, 5) and np.all(est["objval"] <= f0)
    assert np.all(est["f_starts"] <= f0) and est["objval"] == est["f_starts"].min()
    assert np.all((est["x_starts"] >= est["lower"]) & (est["x_starts"] <= est["upper"]))
    assert np.all((est["par"] >= est["lower"]) & (est["par"] <= est["upper"]))
    # the returned objective is var.MLE.DK at the returned point, and the back-transform is GV:164-165
    assert float(cgp_ref.state(Xs, y, cgp.rows_from_ww(est["par"])[0])["val"]) == est["objval"]
    np.testing.assert_allclose(np.ravel(est["alpha"]) - np.ravel(est["theta"]), est["par"][3] / est["scales"] ** 2, rtol=1e-12)


def test_rmscv_is_the_explicit_leave_one_out_loop(fit14):
    D, y, h, est = fit14
    row = cgp.param_row(est)
    loo = np.empty(14)
    for j in range(14):
        keep = np.arange(14) != j
        loo[j] = cgp_ref.predict(D[keep], y[keep], row, D[j:j + 1])[0][0, 0]
    np.testing.assert_allclose(est["Yp_jackknife"], loo, rtol=0, atol=1e-11 * np.abs(y).max())
    assert est["rmscv"] == pytest.approx(np.sqrt(np.sum((y - loo) ** 2) / 14), rel=1e-10)
    # the final state is the reference's: predicting the design reproduces Yp = beta + q'temp with the kept fields
    p = cgp.predict_CGP(h, est, D, PI=True)
    assert np.all(p["Y_low"] <= p["Yp"]) and np.all(p["Yp"] <= p["Y_up"]) and est["Sig_matrix"].shape == (14,)
    assert np.mean(est["Sig_matrix"]) == pytest.approx(1.0, rel=1e-12)
    q = cgp.predict_CGP(h, est, D)
    assert q["Y_low"] is None and np.all(q["lp"] == 0.0) and np.array_equal(q["Yp"], p["Yp"])


def test_device_calls_are_far_fewer_than_evaluations(fit14):
    _, _, h, est = fit14
    print("calls %d, evaluations %d" % (est["calls"], est["evaluations"]))
    assert est["calls"] == h.calls_of_fit and est["evaluations"] == h.points_of_fit + 1 >= 505 + 14 + 1
    assert est["calls"] * 10 < est["evaluations"]
