"""The yardstick of tests/test_gpu_cgp_exact.py proved on the CPU: cgp_state_kernel and cgp_predict_kernel restated in numpy
fp64 in the kernel's operation order (cgp_exact.restate) must use at most HALF of every band of tests/cgp_exact.py on every case
the device module runs, and planted mistakes in that restatement must each leave a band.  For each planted mistake the module
also records whether the older yardstick (tests/test_gpu_cgp.py: max(8 n eps cond1 scale, 8 x the fp64 restatement's own error)
against long double) would have accepted it on the same case.  No GPU.
"""
import functools
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import cgp_exact as cx
import cgp_ref

HALF = 0.5
SEEN = cx.Tally()
CLOCK = {"t": 0.0}


@pytest.fixture(autouse=True)
def _clock():
    t0 = time.perf_counter()
    yield
    CLOCK["t"] += time.perf_counter() - t0


def _inside(t, what):
    SEEN.merge(t)
    assert not t.outside(HALF), (what, t.outside(HALF))


# ----------------------------------------------------------------------------------------------- the restatement, every case
@pytest.mark.parametrize("b", [0, 1], ids=["lambda0.001", "lambda1"])
@pytest.mark.parametrize("n,d", cx.CASES)
def test_restatement_stays_inside_half_of_every_band(n, d, b):
    Xs, y, rows, Xt, on = cx.case(n, d)
    r = cx.restate(Xs, y, rows[b], -1, Xt)
    assert r["status"] == 0
    t, p, nans = cx.check_evaluation(Xs, y, rows[b], r["keep"], r["val"], Xt, r["out"], {4: on})
    assert not nans
    if (n, d, float(rows[b, 0])) == cx.ILL:
        assert p.cond1() >= 1e6
    print("n %d d %d lambda %g cond1 %.3g: %s" % (n, d, rows[b, 0], p.cond1(), t))
    _inside(t, (n, d, b))


@pytest.mark.parametrize("n", cx.JACK_N)
def test_restated_jackknife_stays_inside_half_of_every_band(n):
    d = 2
    Xs, y, rows, _, _ = cx.case(n, d)
    for skip in (0, n // 2, n - 1) if n < 128 else (n // 2,):
        b = skip % 2
        r = cx.restate(Xs, y, rows[b], skip)
        pick = np.arange(n) != skip
        t, p, _ = cx.check_evaluation(Xs[pick], y[pick], rows[b], r["keep"], r["val"])
        cx.loo_check(t, p, Xs[skip], r["loo"])
        print("n %d skip %d lambda %g: %s" % (n, skip, rows[b, 0], t))
        _inside(t, (n, skip))


def test_both_orders_of_the_gbw_rate_stay_inside():
    """band (a) covers sum_k (theta_k bw) df^2 and (sum_k theta_k df^2) bw alike: the state restated with either, at arguments
    beyond 10, where the two orders differ by tens of roundings of exp's result"""
    Xs, y, rows, Xt, on = cx.case(14, 2)
    Xt = Xt[:6]                                   # without the far site: it is placed for the case's own rates
    row = rows[1].copy()
    row[1:3], row[5] = [15.0, 23.0], 0.7371
    one, other = np.exp(-cx._dist(Xs, Xs, row[1:3] * row[5])), np.exp(-cx._dist(Xs, Xs, row[1:3]) * row[5])
    assert -math.log(one.min()) > 10.0 and np.count_nonzero(one != other) > 20, "the two orders must differ in the fp64 bits"
    kept = []
    for order in ("state", "predict"):
        r = cx.restate(Xs, y, row, -1, Xt, gbw_order=order)
        t, _, _ = cx.check_evaluation(Xs, y, row, r["keep"], r["val"], Xt, r["out"], {4: on})
        kept.append(r["keep"]["s"])
        _inside(t, order)
    assert not np.array_equal(kept[0], kept[1])


# ----------------------------------------------------------------------------------------------------------- planted mistakes
def _old_yardstick_accepts(Xs, y, row, skip, Xt, r):
    """Tally.check of tests/test_gpu_cgp.py on the outputs it compares"""
    ref, r64 = cgp_ref.state(Xs, y, row, skip, np.longdouble), cgp_ref.state(Xs, y, row, skip, np.float64)
    c1, m = cgp_ref.cond1(ref), ref["n"]
    pairs = [(k, r[k], r64[k], ref[k]) for k in ("val", "beta", "tau2")]
    p = None
    if skip < 0 and Xt is not None:
        p, p64 = cgp_ref.predict(Xs, y, row, Xt, np.longdouble, ref)[0], cgp_ref.predict(Xs, y, row, Xt, np.float64, r64)[0]
        pairs += [(k, r["out"][:, i], p64[:, i], p[:, i]) for i, k in enumerate(cgp_ref.COLS)]
    sc = cgp_ref.scales(ref, y, p)
    if skip < 0:
        sc["temp"] = float(np.abs(ref["temp"]).max())
        sc["s"] = float(ref["s"].max()) * (1.0 + 2.0 * float(np.abs(y).max()) / float(np.sqrt(ref["res2"].max())))
        pairs += [(k, r["keep"][k], r64[k], ref[k]) for k in ("temp", "s")]
    for k, got, want64, want in pairs:
        err = float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)))
        own = float(np.max(np.abs(np.asarray(want64, dtype=np.longdouble) - want)))
        if not err <= max(cgp_ref.band(m, c1, sc[k]), 8.0 * own):
            return False
    return True


PLANTED = (
    # plant, (n, d), row index, skip, the band that must reject it
    ("s_prev", (14, 2), 0, -1, "s"),
    ("sf_prev", (14, 2), 0, -1, "sf"),
    ("tau2_n0", (14, 2), 1, 7, "tau2"),
    ("temp_1e-10", (128, 2), 0, -1, "resid"),
    ("rinv_1e-12", (14, 2), 0, -1, "resid"),
    ("exp_1e-13", (14, 2), 1, -1, "resid"),
    ("qq_dnext", (14, 2), 1, -1, "Y_up"),
)

@functools.lru_cache(maxsize=None)
def _planted(plant, shape, b, skip):
    """(Tally without the mistake, Tally with it, whether the older yardstick accepts it) on one case"""
    Xs, y, rows, Xt, on = cx.case(*shape)
    n = shape[0]
    sites = Xt if skip < 0 else None
    good, bad = cx.restate(Xs, y, rows[b], skip, sites), cx.restate(Xs, y, rows[b], skip, sites, plant=plant)
    pick = np.arange(n) != skip
    tg, _, _ = cx.check_evaluation(Xs[pick], y[pick], rows[b], good["keep"], good["val"], sites, good["out"], {4: on})
    tb, _, _ = cx.check_evaluation(Xs[pick], y[pick], rows[b], bad["keep"], bad["val"], sites, bad["out"], {4: on})
    return tg, tb, _old_yardstick_accepts(Xs, y, rows[b], skip, sites, bad)


@pytest.mark.parametrize("plant,shape,b,skip,key", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_mistake_leaves_its_band(plant, shape, b, skip, key):
    assert plant in cx.PLANTS
    if plant == "temp_1e-10":
        assert (shape[0], shape[1], float(cx.case(*shape)[2][b, 0])) == cx.ILL
    tg, tb, old = _planted(plant, shape, b, skip)
    assert not tg.outside(HALF)
    assert tb.frac[key] > 1.0, (plant, key, tb.frac[key])
    print("%s: %s band used %.3g times over (unplanted %.3g); the older yardstick %s it" % (
        plant, key, tb.frac[key], tg.frac[key], "ACCEPTS" if old else "rejects"))


def test_the_older_yardstick_accepts_the_rounding_sized_ones():
    """what DESIGN.md K9 records: rounding-sized mistakes pass the cond1 band"""
    old = {p[0]: _planted(p[0], p[1], p[2], p[3])[2] for p in PLANTED}
    print({k: ("accepted" if v else "rejected") for k, v in old.items()})
    assert old["temp_1e-10"] and old["rinv_1e-12"] and old["exp_1e-13"]


# ----------------------------------------------------------------------------------------------------------- the closed form
def _frac_of_longdouble(x):
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


@pytest.mark.parametrize("variant", cx.VARIANTS)
@pytest.mark.parametrize("n", [9, 65])
def test_fraction_chain_is_the_long_double_restatement(n, variant):
    lc = cx.LatticeCase(n, variant)
    assert lc.smin >= Fraction(1, 1000)
    ld = cgp_ref.state(lc.X, lc.y, lc.row, -1, np.longdouble)
    assert ld["status"] == 0
    worst = 0.0
    for got, want in ([(ld["beta"], lc.beta), (ld["tau2"], lc.tau2), (ld["sf"], lc.sf)] + list(zip(ld["temp"], lc.temp))
                      + list(zip(ld["s"], lc.s)) + list(zip(ld["res2"], lc.res2))):
        worst = max(worst, float(abs(_frac_of_longdouble(got) - want) / abs(want)))
    import mpmath as mp
    with mp.workdps(cx.DPS):
        worst = max(worst, float(abs(cx._fm(_frac_of_longdouble(ld["val"])) - lc.val) / abs(lc.val)))
    print("n %d %s: long double against the Fraction chain, largest relative difference %.2g" % (n, variant, worst))
    assert worst <= 1e-17


def test_l_all_ones_has_no_chain():
    with pytest.raises(cx.DegenerateChain):
        cx.LatticeCase(9, "l_rows", one_block=True)


@pytest.mark.parametrize("skip", [-1, 2])
@pytest.mark.parametrize("variant", cx.VARIANTS)
@pytest.mark.parametrize("n", [9, 65])
def test_restated_lattice_stays_inside_half_of_the_running_bands(n, variant, skip):
    lc = cx.LatticeCase(n, variant, skip)
    Xt = lc.sites()
    r = cx.restate(lc.X, lc.y, lc.row, skip)
    r["out"] = cx.restate(lc.Xe, lc.ye, lc.row, -1, Xt)["out"]
    t = cx.Tally()
    cx.lattice_check(t, lc, r, Xt, r["out"])
    print("n %d %s skip %d: %s" % (n, variant, skip, t))
    _inside(t, (n, variant, skip))


def test_lattice_rejects_a_weight_carried_from_the_pass_before():
    """passes 1 to 4 are not observable a posteriori: the closed form holds their carried state"""
    lc = cx.LatticeCase(9, "gbw_identity")
    r = cx.restate(lc.X, lc.y, lc.row, -1, plant="s_prev")
    t = cx.Tally()
    cx.lattice_check(t, lc, r)
    assert t.frac["lattice s"] > 1.0 and t.frac["lattice beta"] > 1.0


def test_zz_report_headroom_and_time():
    print("largest fraction of each band used by the fp64 restatement: %s" % SEEN)
    print("module time %.1f s" % CLOCK["t"])
    assert SEEN.worst() <= HALF
    assert CLOCK["t"] < 60.0
