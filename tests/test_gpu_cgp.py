"""The CGP comparator on the device (ccgp_cgp_state_batch, ccgp_cgp_predict, ccgp_amd.cgp) against tests/cgp_ref.py.

The yardstick.  A device output is compared with the long-double restatement of the same formulas, component-wise, under

    tol = max( C n eps cond_1(Q_final) scale ,  8 x the fp64 restatement's own error against long double on the same case )

with C = 8, n the points of the evaluation, and `scale` the output's cancellation-free magnitude (cgp_ref.scales).  The first
term is the band of one backward-stable solve.  It is a floor: an evaluation chains five solves, each reweighted by the
residuals of the one before, and where that chain amplifies rounding it does so for the fp64 restatement too, whose own
error then stands in for the conditioning of the chain (the device sums in another order).  Every test prints the largest
fraction of `tol` and of the band alone that the device used; DESIGN.md (K9) records them.
"""
import os

import numpy as np
import pytest

import cgp_ref
from conftest import DATA, golden, load_gv, load_qian, synthetic_design
from ccgp_amd import api, cgp
from ccgp_amd.tables import read_table

pytestmark = pytest.mark.gpu

STATE_KEYS = ("val", "beta", "tau2")


def recorded_cgp():
    names, res = read_table(os.path.join(DATA, "gv", "results_50_1.txt"))
    col = {n: i for i, n in enumerate(names)}
    return res[:, :9], res[:, [col["y.hat.CGP"], col["LL.CGP"], col["UL.CGP"]]], res[:, col["y.true"]]


def rows_in_the_box(Xs, B, seed):
    """B parameter rows drawn uniformly inside CGP's own bounds for the standardised design Xs (GV:77-89), lambda alternating
    between its lower bound 0.001 and its upper bound 1."""
    lo, hi = cgp.bounds(Xs)
    ww = lo + np.random.default_rng(seed).random((B, lo.shape[0])) * (hi - lo)
    ww[0::2, 0] = 0.001
    ww[1::2, 0] = 1.0
    return cgp.rows_from_ww(ww)


class Tally:
    """Largest fraction of the tolerance, and of the band alone, used per output."""

    def __init__(self):
        self.tol, self.band, self.beyond = {}, {}, 0

    def check(self, key, got, want64, want, n, cond, scale, where):
        err = float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)))
        own = float(np.max(np.abs(np.asarray(want64, dtype=np.longdouble) - want)))
        band = cgp_ref.band(n, cond, scale)
        tol = max(band, 8.0 * own)
        self.tol[key] = max(self.tol.get(key, 0.0), err / tol)
        self.band[key] = max(self.band.get(key, 0.0), err / band)
        self.beyond += err > band
        assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))) and err <= tol, (key, where, err, band, own)

    def report(self, what):
        print("%s: fraction of tol used %s; of the band alone %s; comparisons beyond the band %d" % (
            what, {k: "%.2g" % v for k, v in self.tol.items()}, {k: "%.2g" % v for k, v in self.band.items()}, self.beyond))


# ---------------------------------------------------------------------------------------------------- recorded table
def test_recorded_cgp_columns(handle):
    """predict.CGP on the device at the recovered fit against the reference's recorded y.hat.CGP / LL.CGP / UL.CGP."""
    fx = golden("gv_cgp_recovered.json")
    D, y, _, _ = load_gv(50)
    Dt, rec, _ = recorded_cgp()
    out, keep, st = handle.cgp_predict(D, y, fx["row"], Dt)
    resid = float(np.abs(out[:, [0, 4, 5]] - rec).max())
    print("largest residual against the recorded table: %.3g" % resid)
    assert st == 0 and resid <= 1e-8
    val, _, _, _, s2 = handle.cgp_state_batch(cgp.standardise(D)[0], y, cgp.rows_from_ww(fx["ww"]))
    assert s2[0] == 0 and val[0] == pytest.approx(fx["objective"], abs=1e-8)
    assert keep["s"].shape == (50,) and np.mean(keep["s"]) == pytest.approx(1.0, rel=1e-12)


# ---------------------------------------------------------------------------------------- state against long double
@pytest.mark.parametrize("d", [1, 2, 9])
@pytest.mark.parametrize("n", [5, 14, 63, 64, 65, 100, 128])
def test_state_and_predict_against_long_double(handle, n, d):
    X, y = synthetic_design(n, d, 1000 + 10 * n + d)
    Xs, _ = cgp.standardise(X)
    skips = [-1, 0, n - 1, n // 2]
    rows = np.repeat(rows_in_the_box(Xs, 2, 7 * n + d), 4, axis=0)          # lambda 0.001 and 1, each with the four skips
    skip = np.array(skips * 2, dtype=np.int32)
    val, beta, tau2, loo, st = handle.cgp_state_batch(Xs, y, rows, skip=skip)
    assert np.all(st == 0)
    got = dict(val=val, beta=beta, tau2=tau2, loo=loo)
    Xt = np.random.default_rng(n + d).random((7, d))
    tally = Tally()
    for b in range(8):
        ref, r64 = cgp_ref.state(Xs, y, rows[b], skip[b], np.longdouble), cgp_ref.state(Xs, y, rows[b], skip[b], np.float64)
        assert ref["status"] == 0
        p = p64 = out = None
        if skip[b] < 0:
            p, p64 = cgp_ref.predict(Xs, y, rows[b], Xt, np.longdouble, ref)[0], cgp_ref.predict(Xs, y, rows[b], Xt, np.float64, r64)[0]
            out, keep, s1 = handle.cgp_predict(Xs, y, rows[b], Xt)
            assert s1 == 0
        sc, c1, m = cgp_ref.scales(ref, y, p), cgp_ref.cond1(ref), ref["n"]
        where = (n, d, int(skip[b]), float(rows[b, 0]))
        for k in STATE_KEYS + (("loo",) if skip[b] >= 0 else ()):
            tally.check(k, got[k][b], r64[k], ref[k], m, c1, sc[k], where)
        if skip[b] < 0:
            assert np.isnan(loo[b])
            for i, k in enumerate(cgp_ref.COLS):
                tally.check(k, out[:, i], p64[:, i], p[:, i], m, c1, sc[k], where)
            # the kept state is the one the batch call evaluated, and out_state is what predict.CGP reads from the fit
            assert keep["beta"] == beta[b] and keep["tau2"] == tau2[b]
            tally.check("temp", keep["temp"], r64["temp"], ref["temp"], m, c1, float(np.abs(ref["temp"]).max()), where)
            tally.check("s", keep["s"], r64["s"], ref["s"], m, c1,
                        float(ref["s"].max()) * (1.0 + 2.0 * float(np.abs(y).max()) / float(np.sqrt(ref["res2"].max()))), where)
    tally.report("n %d d %d" % (n, d))


# ------------------------------------------------------------------------------------------------- batch independence
def test_a_row_has_the_same_bits_alone_in_a_batch_and_across_a_split():
    X, y = synthetic_design(14, 2, 5)
    Xs, _ = cgp.standardise(X)
    B = 12500
    rows = rows_in_the_box(Xs, B, 11)
    skip = np.full(B, -1, dtype=np.int32)
    skip[1::3] = np.arange(B)[1::3] % 14
    h = api.Handle(0)
    try:
        picks = [0, 1, 317, 599, 12400, B - 1]
        alone = [h.cgp_state_batch(Xs, y, rows[b:b + 1], skip=skip[b:b + 1]) for b in picks]
        small = h.cgp_state_batch(Xs, y, rows[:600], skip=skip[:600])
        whole = h.cgp_state_batch(Xs, y, rows, skip=skip)
        ws_whole = h.workspace_bytes()[0]
        # a row costs 8 (2 d + 2 + 4) + 12 = 92 bytes of workspace: 1 MiB, the smallest limit, holds 11 397 of the 12 500
        h2 = api.Handle(0)
        try:
            h2.set_workspace_limit(1 << 20)
            cut = h2.cgp_state_batch(Xs, y, rows, skip=skip)
            assert h2.workspace_bytes()[0] < ws_whole and h2.workspace_bytes()[0] <= (1 << 20) + 4096
        finally:
            h2.close()
    finally:
        h.close()
    for a, b in zip(alone, picks):
        for k in (0, 1, 2, 3, 4):
            assert a[k][0].tobytes() == whole[k][b].tobytes() == cut[k][b].tobytes(), (b, k)
            if b < 600:
                assert a[k][0].tobytes() == small[k][b].tobytes(), (b, k)
    for k in (0, 1, 2, 3, 4):
        assert whole[k].tobytes() == cut[k].tobytes()
    assert np.all(whole[4] == 0)


# ------------------------------------------------------------------------------------------------------------ jackknife
def test_skip_is_the_design_with_the_row_deleted(handle):
    D, y, _, _ = load_gv(50)
    row = np.array(golden("gv_cgp_recovered.json")["row"])
    val, beta, tau2, loo, st = handle.cgp_state_batch(D, y, np.repeat(row[None], 50, axis=0), skip=np.arange(50))
    assert np.all(st == 0)
    tally = Tally()
    for j in range(50):
        keep = np.arange(50) != j
        v1, b1, t1, _, s1 = handle.cgp_state_batch(D[keep], y[keep], row[None])
        out, _, s2 = handle.cgp_predict(D[keep], y[keep], row, D[j:j + 1])
        assert s1[0] == 0 and s2 == 0
        # only addresses depend on the full n; the sums run over the compacted points: the same bits (loo is summed in another
        # order than cgp_predict_kernel's Yp and stays under the band)
        assert val[j].tobytes() == v1[0].tobytes() and beta[j].tobytes() == b1[0].tobytes() and tau2[j].tobytes() == t1[0].tobytes(), j
        ref = cgp_ref.state(D, y, row, j)
        sc, c1 = cgp_ref.scales(ref, y), cgp_ref.cond1(ref)
        for k, a, b in (("val", val[j], v1[0]), ("beta", beta[j], b1[0]), ("tau2", tau2[j], t1[0]), ("loo", loo[j], out[0, 0])):
            tally.check(k, a, b, np.longdouble(b), 49, c1, sc[k], j)
            tally.check(k + " vs host", a, ref[k], np.longdouble(ref[k]), 49, c1, sc[k], j)
    tally.report("jackknife n 50")


# ----------------------------------------------------------------------------------------------------- failure contract
def test_duplicated_row_with_alpha_equal_theta_does_not_fault(handle):
    X, y = synthetic_design(30, 2, 9)
    X[17] = X[4]
    row = np.array([0.001, 3.0, 2.0, 3.0, 2.0, 0.5])
    val, beta, tau2, loo, st = handle.cgp_state_batch(X, y, np.repeat(row[None], 3, axis=0), skip=np.array([-1, 4, 20]))
    ref = [cgp_ref.state(X, y, row, s) for s in (-1, 4, 20)]
    print("status", st, "host", [r["status"] for r in ref], "val", val)
    for b in range(3):
        assert (st[b] > 0) == (ref[b]["status"] > 0)
        if st[b]:
            assert np.isnan(val[b]) and np.isnan(beta[b]) and np.isnan(tau2[b]) and np.isnan(loo[b])
        else:
            assert val[b] == pytest.approx(float(ref[b]["val"]), rel=1e-6)
    out, keep, s1 = handle.cgp_predict(X, y, row, X[:3])
    assert (s1 > 0) == (ref[0]["status"] > 0) and (keep is None) == (s1 > 0)


def test_failed_row_is_nan_and_its_neighbours_are_untouched(handle):
    """A row the host restatement fails on: lambda = 0 (below the fit's nugget_l, through the raw entry point) with theta so
    small that every entry of G is exactly 1 -- Q = G has a second pivot of exactly 0.  (Coincident design points, the other
    way to a singular Q, fail every row of the batch alike: L is 1 there too.)"""
    X, y = synthetic_design(30, 2, 9)
    good = np.array([0.3, 3.0, 2.0, 9.0, 8.0, 0.5])
    bad = np.array([0.0, 1e-17, 1e-17, 9.0, 8.0, 0.5])
    assert cgp_ref.state(X, y, bad)["status"] == 2 and cgp_ref.state(X, y, bad, 3)["status"] == 2
    assert cgp_ref.state(X, y, good)["status"] == 0
    rows = np.stack([good, bad, good * np.array([1, 1.1, 1, 1, 1, 1]), bad, good])
    val, beta, tau2, loo, st = handle.cgp_state_batch(X, y, rows, skip=np.array([-1, -1, 3, 3, 29]))
    assert st.tolist() == [0, 2, 0, 2, 0]
    for b in (1, 3):
        assert np.isnan(val[b]) and np.isnan(beta[b]) and np.isnan(tau2[b]) and np.isnan(loo[b])
    for b, sk in ((0, -1), (2, 3), (4, 29)):
        a = handle.cgp_state_batch(X, y, rows[b:b + 1], skip=np.array([sk]))
        assert all(a[k][0].tobytes() == (val, beta, tau2, loo)[k][b].tobytes() for k in range(4)) and np.isfinite(val[b])
        assert val[b] == pytest.approx(float(cgp_ref.state(X, y, rows[b], sk)["val"]), rel=1e-9)
    out, keep, s1 = handle.cgp_predict(X, y, bad, X[:5])
    assert s1 == 2 and keep is None and np.all(np.isnan(out))


def test_unsupported_and_bad_arguments_are_refused_before_any_launch():
    h = api.Handle(0)
    try:
        before = h.workspace_bytes()
        X, y = synthetic_design(129, 2, 1)
        for call in (lambda: h.cgp_state_batch(X, y, np.ones((1, 6))), lambda: h.cgp_predict(X, y, np.ones(6), X[:2])):
            with pytest.raises(api.CcgpError) as e:
                call()
            assert e.value.code == -4
        X, y = synthetic_design(128, 22, 1)        # the design no longer fits beside the working matrix
        with pytest.raises(api.CcgpError) as e:
            h.cgp_state_batch(X, y, np.ones((1, 46)))
        assert e.value.code == -4
        X, y = synthetic_design(10, 2, 1)
        with pytest.raises(api.CcgpError) as e:
            h.cgp_state_batch(X, y, np.ones((2, 6)), skip=np.array([0, 10]))
        assert e.value.code == -1
        assert h.workspace_bytes() == before       # nothing was allocated, so nothing was launched
        val, _, _, _, st = h.cgp_state_batch(*synthetic_design(128, 21, 1), np.concatenate([[0.01], np.full(21, 0.3), np.full(21, 4.0), [0.5]])[None])
        assert st[0] == 0 and np.isfinite(val[0])
    finally:
        h.close()


# -------------------------------------------------------------------------------------------------------- fit end to end
def test_fit_on_ground_vibrations_reaches_the_recorded_optimum(handle):
    fx = golden("gv_cgp_recovered.json")
    D, y, _, _ = load_gv(50)
    Dt, rec, yt = recorded_cgp()
    est = cgp.CGP(handle, D, y, rng=0)
    p = cgp.predict_CGP(handle, est, Dt, PI=True)
    rms = float(np.sqrt(np.mean((p["Yp"] - rec[:, 0]) ** 2)))
    rmspe = float(np.sqrt(np.mean((p["Yp"] - yt) ** 2)))
    cover = int(np.sum((yt >= p["Y_low"]) & (yt <= p["Y_up"])))
    rec_cover = int(np.sum((yt >= rec[:, 1]) & (yt <= rec[:, 2])))
    print("objval %.6f (fixture %.6f), rms to recorded %.4g, RMSPE %.4f, coverage %d / 150 (recorded %d), calls %d, evaluations %d"
          % (est["objval"], fx["objective"], rms, rmspe, cover, rec_cover, est["calls"], est["evaluations"]))
    assert rec_cover == 109
    assert est["objval"] <= fx["objective"] + 5e-3
    assert rms <= 0.05
    assert abs(rmspe - 2.8556) <= 0.02
    assert abs(cover - 109) <= 2
    assert est["calls"] < 400
    # rmscv: the restatement's jackknife at the returned parameters
    row = cgp.param_row(est)
    refs = [cgp_ref.state(D, y, row, j) for j in range(50)]
    loo = np.array([float(r["loo"]) for r in refs])
    tally = Tally()
    for j in range(50):
        tally.check("Yp_jackknife", est["Yp_jackknife"][j], loo[j], np.longdouble(loo[j]), 49, cgp_ref.cond1(refs[j]),
                    float(np.abs(y).max()), j)
    want = float(np.sqrt(np.sum((y - loo) ** 2) / 50))
    assert abs(est["rmscv"] - want) <= max(cgp_ref.band(49, max(cgp_ref.cond1(r) for r in refs), float(np.abs(y).max())), 0.0)
    tally.report("fit")


# ------------------------------------------------------------------------------------------------------------------ table
def test_results_table_gains_the_cgp_columns(handle, tmp_path):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    D, y, Dt, yt = load_qian()
    gp = CombinedGP("HX", handle=handle)
    draws = np.array([[0.3, 1.0, 4.0], [0.5, 2.0, 6.0], [0.7, 0.5, 3.0], [0.4, 1.5, 8.0]])
    names_in = ["x1", "x2", "x3", "x4"]
    plain = fit.compare_GP(gp, Dt, 0.05, yt, draws, D, 60.0, y, exact=True)
    with_cgp = fit.compare_GP(gp, Dt, 0.05, yt, draws, D, 60.0, y, exact=True, cgp=dict(num_starts=2, rng=1))
    assert "y_hat_CGP" not in plain and sorted(set(with_cgp) - set(plain)) == ["CGP", "LL_CGP", "UL_CGP", "y_hat_CGP"]
    for k in plain:
        assert np.array_equal(plain[k], with_cgp[k])
    pa, pb = os.path.join(tmp_path, "a.txt"), os.path.join(tmp_path, "b.txt")
    fit.write_results_table(pa, plain, Dt, names_in)
    names = fit.write_results_table(pb, with_cgp, Dt, names_in)
    _, a = read_table(pa)
    _, b = read_table(pb)
    col = {n: i for i, n in enumerate(names)}
    single = [col["y.hat.single"], col["LL.single"], col["UL.single"]]
    cg = [col["y.hat.CGP"], col["LL.CGP"], col["UL.CGP"]]
    assert np.all(np.isnan(a[:, single + cg])) and np.all(np.isnan(b[:, single]))
    assert np.all(np.isfinite(b[:, cg])) and np.all(b[:, cg[1]] <= b[:, cg[0]]) and np.all(b[:, cg[0]] <= b[:, cg[2]])
    rest = [i for i in range(len(names)) if i not in cg]
    assert np.array_equal(a[:, rest], b[:, rest], equal_nan=True)
    # today's table: the same bytes as a table whose comparator columns are filled with NA by hand
    from ccgp_amd.tables import write_table
    pc = os.path.join(tmp_path, "c.txt")
    write_table(pc, np.hstack([Dt, plain["y_hat"][:, None], plain["quant"][:, None], plain["LL"][:, None], plain["UL"][:, None],
                               np.full((Dt.shape[0], 6), np.nan), yt[:, None]]), names)
    with open(pa, "rb") as f1, open(pc, "rb") as f2:
        assert f1.read() == f2.read()
    rmspe = float(np.sqrt(np.mean((b[:, cg[0]] - yt) ** 2)))
    print("Qian: CGP RMSPE %.3f (sd of y.test %.3f)" % (rmspe, np.std(yt)))
    assert rmspe < 0.5 * np.std(yt)
