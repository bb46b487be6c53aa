"""ccgp_krige_predict_batch -- the single-GP comparator's prediction in its three variance forms (ORDINARY: predict.post;
PLUGIN: mlegp's se.fit^2; UNBIASED: the 1-D scripts' Q / (n - 1)) -- on every prediction route, and compare.GP's `.single`
columns on top of it.

Yardstick: tests/krige_ref.py (long double on top of oracle.ccgp_oracle.predict_factor / predict_parts, component-wise
bands with C = PREDICT_TOL_C = 128, no condition number and no floor; tests/test_krige_ref.py holds the bands' margin and
the forms themselves on the host).  Every entry of both tables, beta and Q must lie in its band.

Each exactness call has B = 5 rows: the case's draws with the weights scaled by 10^(-b / 2) -- R is normalised, so the model
is the same and sigma2_hat of ccgp_profile_batch moves by decades -- and sigma2_b = 1.3 10^(b - 2), y scaled per case: a
row that read another row's sigma2 or Q misses every band.

Largest |device - reference| / (band / C) per route and form on an MI355X (test_zz_report_headroom prints them; the limit
is C = 128):
    route                            ordinary  plugin  unbiased  Q       mean    beta
    kept factor                      0.271     0.274   0.259     0.0274  0.030   0.0079
    extra rows                       0.301     0.301   0.301     0.0058  0.023   0.0026
    blocked sweep, phase launches    0.179     0.179   0.179     0.0129  0.015   0.0049
    blocked sweep, scheduled launch  0.122     0.122   0.122     0.0058  0.011   0.0024
    1-D, Matern(5), n = 8            --        --      1.04      --      0.0014  --
No route left its band.
"""
import functools
import os

import numpy as np
import pytest
from scipy.stats import t as student_t

import exact_designs as ex
import krige_ref as kr
import test_gpu_failure_contract as fc
import test_gpu_predict_exact as px
import test_gpu_profile as tp
from conftest import DATA, golden, load_gv
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import _timed
from test_gpu_routes import assert_tier

pytestmark = pytest.mark.gpu

B = 5
SIGMA2 = 1.3 * 10.0 ** (np.arange(B) - 2.0)
C = kr.C
MAX_RATIO = {}
# the cases of tests/krige_ref.py, the extra-row scheme by option, and the sweep as one scheduled launch
EXACT_CASES = [c + (None,) for c in kr.CASES] + [("extra", 128, 2, 3, 63, "factor0"), ("sched",) + px.SCHED_CASE + ("sched",)]
ONE_PER_ROUTE = [("kept", 50, 4, 1, 257), ("extra", 105, 2, 2, 62), ("blocked", 129, 3, 2, 129)]


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def _ulp(v, k=4):
    return k * np.spacing(np.abs(v))


@functools.lru_cache(maxsize=None)
def _case(n, d, K, m):
    """(X, y, rows[B], Xt): make_case's design, draws and sites; weights scaled per row, y per case."""
    X, y, P, Xt = px.make_case(n, d, K, m, "plain" if (n, d) == (40, 1) else "full")
    rows = P[np.arange(B) % len(P)].copy()
    rows[:, :K] *= 10.0 ** (-0.5 * np.arange(B))[:, None]
    y = y * 10.0 ** ((n + m) % 5 - 2)
    for a in (X, y, rows, Xt):
        a.setflags(write=False)
    return X, y, rows, Xt


@functools.lru_cache(maxsize=None)
def _reference(n, d, K, m, b):
    X, y, rows, Xt = _case(n, d, K, m)
    ref = kr.reference(X, y, rows[b], K, Xt)
    assert orc.cond1(ref["factor"]["R"], ref["factor"]["Rinv"]) <= px.KAPPA_MAX
    return ref, kr.bands(ref)


class _route:
    """Run a call on the route a case names and assert, through the timing counters and the mirrored predicates, that it
    took it."""

    def __init__(self, handle, route, n, d, K, opt=None):
        self.a = (handle, route, n, d, K, opt)

    def __call__(self, fn):
        from ccgp_amd import api
        handle, route, n, d, K, opt = self.a
        option = {"factor0": (api.OPT_PREDICT_FACTOR, 0, 1), "sched": (api.OPT_SCHED, 1, 3)}.get(opt)
        if option:
            handle.set_option(option[0], option[1])
        try:
            out, t = _timed(handle, fn)
        finally:
            if option:
                handle.set_option(option[0], option[2])
        if route == "kept":
            assert px.kept_factor(n, d, K) and opt is None
            assert_tier(t, "r", n)
        elif route == "extra":
            assert px.predict_route(n, d, K) == "r" and (opt == "factor0" or not px.kept_factor(n, d, K))
            assert_tier(t, "r", n)
        elif route == "blocked":
            assert px.predict_route(n, d, K) == "b"
            assert_tier(t, "b", n)
            assert t["sweep"][1] == 0, t
        else:
            assert px.predict_route(n, d, K) == "b" and t["fused"][1] == 0 and t["sweep"][1] > 0, t
        return out


def _note(route, name, ratio):
    key = (route, name)
    MAX_RATIO[key] = max(MAX_RATIO.get(key, 0.0), float(ratio) * C)


# ----------------------------------------------------------------------------- 1. exact, every route x every form
@pytest.mark.parametrize("route,n,d,K,m,opt", EXACT_CASES, ids=["%s-%d-%d-%d-%d" % c[:5] for c in EXACT_CASES])
def test_exact_on_every_route_in_every_form(handle, route, n, d, K, m, opt):
    X, y, rows, Xt = _case(n, d, K, m)
    far = np.nonzero((Xt == 50.0).all(axis=1))[0]
    assert far.size == (1 if m > 1 else 0)                          # a lone site is the training point n - 1
    for form in kr.FORMS:
        name = kr.FORM_NAMES[form]
        s2_in = None if form == kr.UNBIASED else SIGMA2
        mean, var, beta, q, st = _route(handle, route, n, d, K, opt)(
            lambda: handle.krige_predict_batch(X, y, K, rows, s2_in, Xt, form))
        assert not st.any() and mean.shape == (B, m) and var.shape == (B, m)
        for b in range(B):
            ref, bnd = _reference(n, d, K, m, b)
            e_mean = np.abs(mean[b] - _f64(ref["mean"]))
            e_beta = abs(beta[b] - float(ref["beta"]))
            e_q = abs(q[b] - float(ref["Q"]))
            want = _f64(kr.variance(ref, form, SIGMA2[b]))
            vband = kr.variance_band(ref, bnd, form, SIGMA2[b])
            e_var = np.abs(var[b] - want)
            print("%s %s row %d: var %.3g mean %.3g beta %.3g Q %.3g (x band / C)" % (
                route, name, b, (e_var / vband).max() * C, (e_mean / bnd["mean"]).max() * C, e_beta / bnd["beta"] * C,
                e_q / bnd["Q"] * C))
            _note(route, name, (e_var / vband).max())
            _note(route, "mean", (e_mean / bnd["mean"]).max())
            _note(route, "beta", e_beta / bnd["beta"])
            _note(route, "Q", e_q / bnd["Q"])
            bad = np.nonzero(~(e_var <= vband))[0]
            assert bad.size == 0, (route, name, b, bad[:6], var[b][bad[:6]], want[bad[:6]], (e_var / vband)[bad[:6]])
            assert (e_mean <= bnd["mean"]).all(), (route, name, b, (e_mean / bnd["mean"]).max())
            assert e_beta <= bnd["beta"], (route, name, b, beta[b], float(ref["beta"]))
            assert e_q <= bnd["Q"], (route, name, b, q[b], float(ref["Q"]), bnd["Q"])
            # the far site: every correlation underflows, so the mean is beta and the variance shows the form's terms alone
            if far.size == 0:
                continue
            t = far[0]
            s11, Q = float(ref["s11"]), float(ref["Q"])
            assert float(_f64(ref["parts"]["r"])[t].max()) <= 1e-60
            assert abs(mean[b, t] - beta[b]) <= _ulp(beta[b]), (route, name, b, mean[b, t], beta[b])
            if form == kr.PLUGIN:
                assert var[b, t] == SIGMA2[b], (route, b, var[b, t], SIGMA2[b])          # no term for the estimated mean
            elif form == kr.ORDINARY:
                w = SIGMA2[b] * (1.0 + 1.0 / s11)
                assert abs(var[b, t] - w) <= _ulp(w) + SIGMA2[b] * bnd["s11"] / s11 ** 2, (route, b, var[b, t], w)
            else:
                w = Q / (n - 1) * (1.0 + 1.0 / s11)
                tol = _ulp(w) + Q / (n - 1) * bnd["s11"] / s11 ** 2 + (1.0 + 1.0 / s11) * bnd["Q"] / (n - 1)
                assert abs(var[b, t] - w) <= tol, (route, b, var[b, t], w, tol)


# ----------------------------------------------------------------------------- 2. the same path as ccgp_predict_batch
@pytest.mark.parametrize("route,n,d,K,m", ONE_PER_ROUTE, ids=[c[0] for c in ONE_PER_ROUTE])
def test_ordinary_form_returns_the_bits_of_predict_batch(handle, route, n, d, K, m):
    X, y, P, Xt = px.make_case(n, d, K, m)
    want = handle.predict_batch(X, y, K, P, Xt, 1.3)
    got = _route(handle, route, n, d, K)(
        lambda: handle.krige_predict_batch(X, y, K, P, np.full(len(P), 1.3), Xt, kr.ORDINARY))
    assert not got[4].any() and not want[3].any()
    assert tp._same((got[0], got[1], got[2]), want[:3])


# ----------------------------------------------------------------------------- 3. a row is its own
def _rows_alone(handle, X, y, K, rows, s2, Xt, batched, form, which):
    for b in which:
        one = handle.krige_predict_batch(X, y, K, rows[b:b + 1], None if form == kr.UNBIASED else s2[b:b + 1], Xt, form)
        assert one[4][0] == 0
        assert tp._same([a[b:b + 1] for a in batched[:4]], one[:4]), (kr.FORM_NAMES[form], b)


@pytest.mark.parametrize("form", kr.FORMS)
def test_a_row_is_its_own_across_the_draw_chunk_of_the_kept_factor(handle, form):
    """B = 70 crosses the 64 draws the factorising instance takes in its four-wave form and, on a small workspace, a chunk."""
    n, d, K, m = 9, 4, 3, 64
    X, y, rows5, Xt = _case(n, d, K, m)
    rows = np.concatenate([rows5 * np.concatenate([np.full(K, 1.0 + 0.25 * c), np.ones(K * d)]) for c in range(14)])
    s2 = 1.3 * 10.0 ** ((np.arange(70) % 7) - 3.0)
    got = _route(handle, "kept", n, d, K)(
        lambda: handle.krige_predict_batch(X, y, K, rows, None if form == kr.UNBIASED else s2, Xt, form))
    assert not got[4].any()
    _rows_alone(handle, X, y, K, rows, s2, Xt, got, form, range(70))


@pytest.mark.parametrize("form", kr.FORMS)
def test_a_row_is_its_own_across_the_site_chunk_of_the_extra_rows(handle, form):
    """m = 63 = one chunk of 62 sites and one site: Q and sigma2 reach both workgroups of a row."""
    n, d, K, m = 128, 9, 1, 63
    X, y, rows, Xt = _case(n, d, K, m)
    got = _route(handle, "extra", n, d, K)(
        lambda: handle.krige_predict_batch(X, y, K, rows, None if form == kr.UNBIASED else SIGMA2, Xt, form))
    assert not got[4].any()
    _rows_alone(handle, X, y, K, rows, SIGMA2, Xt, got, form, range(B))


@pytest.mark.parametrize("form", kr.FORMS)
def test_a_row_is_its_own_across_the_chunks_of_the_sweep(handle, form):
    """Under a workspace limit of 4 MB the five matrices of n = 129 with their 129 site rows (1.6 MB each) take at least
    three chunks: sigma2 and Q are indexed by the row of the call, not of the chunk."""
    n, d, K, m = 129, 3, 2, 129
    X, y, rows, Xt = _case(n, d, K, m)
    with fc._limit(handle, 4 << 20):
        got, t = _timed(handle, lambda: handle.krige_predict_batch(X, y, K, rows, None if form == kr.UNBIASED else SIGMA2, Xt, form))
    assert_tier(t, "b", n)
    assert t["solve"][1] >= 3, t
    assert not got[4].any()
    _rows_alone(handle, X, y, K, rows, SIGMA2, Xt, got, form, range(B))


# ----------------------------------------------------------------------------- 4. the forms against each other and the fit
@pytest.mark.parametrize("route,n,d,K,m", [c for c in kr.CASES if c[1:] in ((64, 2, 3, 65), (105, 2, 2, 62), (129, 3, 2, 129))],
                         ids=["kept", "extra", "blocked"])
def test_forms_agree_with_each_other_and_with_the_profiled_fit(handle, route, n, d, K, m):
    X, y, rows, Xt = _case(n, d, K, m)
    run = _route(handle, route, n, d, K)
    m_o, v_o, beta, q, st = run(lambda: handle.krige_predict_batch(X, y, K, rows, SIGMA2, Xt, kr.ORDINARY))
    _, v_p, _, q_p, _ = run(lambda: handle.krige_predict_batch(X, y, K, rows, SIGMA2, Xt, kr.PLUGIN))
    m_u, v_u, _, q_u, _ = run(lambda: handle.krige_predict_batch(X, y, K, rows, None, Xt, kr.UNBIASED))
    assert not st.any() and tp._same((q, m_o), (q_p, m_o)) and tp._same((q, m_o), (q_u, m_u))
    # Q is n sum w^2 sigma2_hat of the profiled likelihood: the same sum on the same route, then a division and two products
    _, s2_hat, beta_p, _, st_p = handle.profile_batch(X, y, K, rows, grad=False)
    assert not st_p.any() and tp._same((beta,), (beta_p,))
    sw = (rows[:, :K] ** 2).sum(axis=1)
    assert s2_hat.max() / s2_hat.min() > 1e3
    assert (np.abs(q - n * sw * s2_hat) <= _ulp(q, 8)).all(), (q, n * sw * s2_hat)
    # UNBIASED is ORDINARY at sigma2_b = Q_b / (n - 1)
    _, v_q, _, _, _ = run(lambda: handle.krige_predict_batch(X, y, K, rows, q / (n - 1), Xt, kr.ORDINARY))
    assert (np.abs(v_u - v_q) <= _ulp(v_q)).all()
    # ORDINARY - PLUGIN is the term for the estimated mean, sigma2 u^2 / s11 >= 0
    for b in range(B):
        ref, bnd = _reference(n, d, K, m, b)
        term = SIGMA2[b] * _f64(ref["unit"] - ref["plug_unit"])
        both = kr.variance_band(ref, bnd, kr.ORDINARY, SIGMA2[b]) + kr.variance_band(ref, bnd, kr.PLUGIN, SIGMA2[b])
        diff = v_o[b] - v_p[b]
        assert (np.abs(diff - term) <= both).all() and (diff >= -both).all(), (route, b)


# ----------------------------------------------------------------------------- 5. the failure contract
def _krige(h, D, K, Xt, form):
    def call(rows):
        s2 = None if form == kr.UNBIASED else np.full(len(rows), 1.3)
        mean, var, beta, q, st = h.krige_predict_batch(D.X, D.y, K, rows, s2, Xt, form)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    return call


@pytest.mark.parametrize("form", kr.FORMS)
@pytest.mark.parametrize("route,n,m,chunk", [("kept", 64, 65, 64), ("extra", 128, 63, 62), ("blocked", 129, 129, 128)])
def test_failed_rows_are_reported_as_predict_batch_reports_them(handle, route, n, m, chunk, form):
    """Exact 0/1 designs (tests/exact_designs.py): the status is the known pivot index, a failed row is NaN in mean, var, beta
    and q, its neighbours on both sides keep the bits of a call without it, and the return value counts the failed rows."""
    K = 2
    D = ex.ExactDesign(n, ex.predict_seps(n))
    rows, exp = D.draws(K, D.mixed())
    Xt, _ = D.sites(m, chunk)
    out, t = fc._contract(handle, _krige(handle, D, K, Xt, form), rows, exp)
    (fc._small if route != "blocked" else (lambda tt: fc._blocked(tt, n)))(t)
    assert (route == "kept") == fc.sites_supported(D.n, D.d, K)
    one = np.nonzero(exp)[0][:1]
    single, rc, _ = fc._call(handle, lambda: _krige(handle, D, K, Xt, form)(rows[one]))
    assert rc == 1 and single["status"][0] == exp[one[0]] and np.isnan(single["q"][0]) and np.isnan(single["var"]).all()


def test_argument_errors_leave_the_outputs_untouched(handle):
    from ccgp_amd import api
    X, y, rows, Xt = _case(9, 4, 3, 64)
    n, d, K, m = 9, 4, 3, 64
    Xf, Xtf, rf = (np.asfortranarray(a) for a in (X, Xt, rows))
    poison = -1.2345e77

    def raw(n_rows, s2, form):
        bufs = [np.full((B, m), poison, order="F"), np.full((B, m), poison, order="F"), np.full(B, poison), np.full(B, poison)]
        st = np.full(B, 77, dtype=np.int32)
        rc = api.lib().ccgp_krige_predict_batch(handle._h, api._p(Xf[:n_rows].copy(order="F")), n_rows, d, api._p(y[:n_rows].copy()), K,
                                                api._p(rf), B, api._p(s2), form, api._p(Xtf), m, api._p(bufs[0]), api._p(bufs[1]),
                                                api._p(bufs[2]), api._p(bufs[3]), api._ipt(st))
        assert all((b == poison).all() for b in bufs) and (st == 77).all(), "outputs were written"
        return rc

    ok = SIGMA2.copy()
    for form in (-1, 3, 7):
        assert raw(n, ok, form) == -1                               # CCGP_EINVAL
    assert raw(1, None, kr.UNBIASED) == -1                          # n - 1 = 0
    for form in (kr.ORDINARY, kr.PLUGIN):
        assert raw(n, None, form) == -1
        for v in (np.nan, np.inf, -np.inf, -1e-300):
            s2 = ok.copy()
            s2[3] = v
            assert raw(n, s2, form) == -1, (form, v)
    # and the same buffers are written by a good call: sigma2 = 0 is allowed
    mean, var, _, _, st = handle.krige_predict_batch(X, y, K, rows, np.zeros(B), Xt, kr.PLUGIN)
    assert not st.any() and (var == 0.0).all() and np.isfinite(mean).all()


# ----------------------------------------------------------------------------- 6. known answer, device only
def _recorded():
    from ccgp_amd.tables import read_table
    names, res = read_table(os.path.join(DATA, "gv", "results_50_1.txt"))
    return names, {k: res[:, i] for i, k in enumerate(names)}, res[:, :9]


def test_device_alone_reproduces_the_recorded_single_columns(handle, tmp_path):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table
    fx = golden("gv_mlegp_recovered.json")
    names, rec, Dt = _recorded()
    D, y, _, ytest = load_gv(50)
    gp = CombinedGP("GV", handle=handle)
    table = fit.compare_GP(gp, Dt, 0.05, ytest, [(0.8, 0.05, 2.0), (0.6, 0.1, 1.0)], D, fx["sigma2"], y, rng=0,
                           single=dict(theta=fx["theta"], sigma2=fx["sigma2"]))
    np.testing.assert_allclose(table["y_hat_single"], rec["y.hat.single"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(table["LL_single"], rec["LL.single"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(table["UL_single"], rec["UL.single"], rtol=0, atol=1e-7)
    path = str(tmp_path / "results.txt")
    written = fit.write_results_table(path, table, Dt, names[:9])
    assert written == names
    _, back = read_table(path)
    for k in ("y.hat.single", "LL.single", "UL.single"):
        col = back[:, names.index(k)]
        assert not np.isnan(col).any()
        np.testing.assert_allclose(col, rec[k], rtol=0, atol=1e-7)
    s = fit.comparison_summary(table)
    want_rmspe = float(np.sqrt(np.mean((rec["y.true"] - rec["y.hat.single"]) ** 2)))
    want_cover = float(np.mean((rec["y.true"] >= rec["LL.single"]) & (rec["y.true"] <= rec["UL.single"])))
    assert abs(s["rmspe_single"] - want_rmspe) <= 1e-7 and s["coverage_single"] == want_cover
    assert abs(want_rmspe - 2.687) < 1e-3 and abs(want_cover - 0.867) < 1e-3
    assert "rmspe_CGP" not in s and {"rmspe", "coverage", "mean_quantile"} <= set(s)


# ----------------------------------------------------------------------------- 7. end to end
def test_compare_gp_fits_and_predicts_all_three_models(handle, tmp_path):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    from ccgp_amd.tables import read_table
    fx = golden("gv_mlegp_recovered.json")
    names, _, Dt = _recorded()
    D, y, _, ytest = load_gv(50)
    gp = CombinedGP("GV", handle=handle)
    table = fit.compare_GP(gp, Dt, 0.05, ytest, [(0.8, 0.05, 2.0), (0.6, 0.1, 1.0)], D, fx["sigma2"], y, rng=0, exact=True,
                           cgp=True, single=True)
    for c in ("", "_single", "_CGP"):
        yh, lo, hi = table["y_hat" + c], table["LL" + c], table["UL" + c]
        assert np.isfinite(yh).all() and np.isfinite(lo).all() and np.isfinite(hi).all(), c
        assert (lo < yh).all() and (yh < hi).all(), c
    ll_mlegp = handle.profile_batch(D, y, 1, np.concatenate([[1.0], fx["theta"]])[None])[0][0]
    assert table["single"]["loglik"] >= ll_mlegp                    # mlegp stopped short of the MLE
    path = str(tmp_path / "results.txt")
    assert fit.write_results_table(path, table, Dt, names[:9]) == names and len(names) == 20
    assert not np.isnan(read_table(path)[1]).any()
    s = fit.comparison_summary(table)
    assert {"rmspe_single", "coverage_single", "rmspe_CGP", "coverage_CGP"} <= set(s)


# ----------------------------------------------------------------------------- 8. the 1-D scripts
@pytest.mark.parametrize("two_families", [False, True], ids=["D1", "D1F"])
def test_one_dimensional_single_gp(handle, two_families):
    """CombinedGP1D(nu = 5), n = 8: MLEs() on the device, then prediction.single (D1:548-567; the two-family script's copy,
    D1F:872-889, is the same Matern model).  y_hat_single and single_var against tests/krige_ref.py with the Matern entries
    of tests/family_exact.py; LL / UL through qt(1 - alpha / 2, 7)."""
    import family_exact as fx
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP1D, CombinedGP1DTwoFamilies
    from test_gpu_family_end_to_end import _rho
    n, nu, alpha = 8, 5.0, 0.1
    x = (np.arange(n) + np.array([0.3, 0.7, 0.2, 0.5, 0.8, 0.4, 0.6, 0.1])) / n
    y = np.sin(5.0 * x) + 0.5 * x
    sites = np.array([0.05, 0.31, x[3], x[5] + 1e-3, 0.77, 1.2])
    gp = (CombinedGP1DTwoFamilies if two_families else CombinedGP1D)(nu, handle=handle)
    draws = [(0.6, 0.3, 0.1), (0.4, 0.5, 0.2)]
    table = fit.compare_GP(gp, sites, alpha, np.sin(5.0 * sites) + 0.5 * sites, draws, x, 0.5, y, rng=0, single=True)
    theta = table["single"]["theta"]
    assert set(table["single"]) >= {"theta", "sigma2", "beta"} and theta > 0
    # the reference at the fitted theta: exact Matern entries, their own rho in place of the expanded exponent's
    gram, cross = fx.table(1, nu, (1.0,), (theta,), x, x), fx.table(1, nu, (1.0,), (theta,), sites, x)
    ld = np.longdouble
    f = orc.predict_factor(x[:, None], y, np.array([1.0, theta]), 1, 1, ld, Rc=[gram.longdouble()])
    aL = np.abs(_f64(f["L"]))
    gband = (gram.band + 2.0 * kr.EPS * np.abs(gram.hi)) * (1.0 - np.eye(n))
    cband = cross.band + 2.0 * kr.EPS * np.abs(cross.hi)
    rho_t = np.array([_rho(cband[t], cross.hi[t]) for t in range(len(sites))])
    ref = kr.reference(x[:, None], y, np.array([1.0, theta]), 1, sites[:, None], factor=f, rc=[cross.longdouble()],
                       rho=_rho(gband, aL @ aL.T), rho_t=rho_t)
    bnd = kr.bands(ref)
    assert orc.cond1(f["R"], f["Rinv"]) <= px.KAPPA_MAX
    e_mean = np.abs(table["y_hat_single"] - _f64(ref["mean"]))
    e_var = np.abs(table["single_var"] - _f64(kr.variance(ref, kr.UNBIASED)))
    vband = kr.variance_band(ref, bnd, kr.UNBIASED)
    print("1-D single GP theta %.6g: mean %.3g var %.3g (x band / C)" % (theta, (e_mean / bnd["mean"]).max() * C, (e_var / vband).max() * C))
    _note("1-D " + ("D1F" if two_families else "D1"), "unbiased", (e_var / vband).max())
    assert (e_mean <= bnd["mean"]).all() and (e_var <= vband).all(), (e_mean / bnd["mean"], e_var / vband)
    delta = student_t.ppf(1.0 - alpha / 2.0, n - 1) * np.sqrt(np.maximum(table["single_var"], 0.0))
    assert (np.abs(table["LL_single"] - (table["y_hat_single"] - delta)) <= _ulp(table["y_hat_single"]) + _ulp(delta)).all()
    assert (np.abs(table["UL_single"] - (table["y_hat_single"] + delta)) <= _ulp(table["y_hat_single"]) + _ulp(delta)).all()
    # prediction.single itself, at the same model, is what compare_GP wrote
    ps = fit.prediction_single(handle, x, sites, y, table["single"], alpha, nu=nu)
    assert tp._same([ps[k] for k in ("y_hat_single", "LL_single", "UL_single", "single_var")],
                    [table[k] for k in ("y_hat_single", "LL_single", "UL_single", "single_var")])


def test_zz_report_headroom():
    """Largest |device - reference| / (band / C) per route and quantity: C = 128 is the limit."""
    for route in sorted({k[0] for k in MAX_RATIO}):
        print("max ratio %-8s " % route + "  ".join("%s %.3g" % (k[1], v) for k, v in sorted(MAX_RATIO.items()) if k[0] == route))
