"""The yardstick of tests/test_gpu_krige.py, on the host (tests/krige_ref.py): its bands leave the margin asked of the
existing variance band, its PLUGIN form is the variance the reference recorded, and its UNBIASED form is the 1-D script's
arithmetic."""
import functools
import os

import numpy as np
from scipy.stats import t as student_t

import krige_ref as kr
from conftest import DATA, golden, load_gv
from ccgp_amd.tables import read_table
from oracle import ccgp_oracle as orc
from test_gpu_predict_exact import S, make_case

MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def _ratios(route, n, d, K, m):
    """largest |fp64 restatement - long double| / (band / C) per quantity over the case's draws"""
    X, y, P, Xt = make_case(n, d, K, m, "plain" if (n, d) == (40, 1) else "full")
    worst = dict(plugin=0.0, unbiased=0.0, ordinary=0.0, Q=0.0, mean=0.0)
    for s in range(S):
        ref = kr.reference(X, y, P[s], K, Xt)
        bnd = kr.bands(ref)
        dev = kr.device_restatement(X, y, P[s], K, Xt)
        got = {kr.ORDINARY: 1.3 * dev["unit"], kr.PLUGIN: 1.3 * dev["plug_unit"], kr.UNBIASED: dev["Q"] / (n - 1) * dev["unit"]}
        for form in kr.FORMS:
            err = np.abs(got[form] - np.asarray(kr.variance(ref, form, 1.3), dtype=np.float64))
            name = kr.FORM_NAMES[form]
            worst[name] = max(worst[name], float((err / kr.variance_band(ref, bnd, form, 1.3)).max()) * kr.C)
        worst["Q"] = max(worst["Q"], abs(dev["Q"] - float(ref["Q"])) / bnd["Q"] * kr.C)
        worst["mean"] = max(worst["mean"], float((np.abs(dev["mean"] - np.asarray(ref["mean"], dtype=np.float64)) / bnd["mean"]).max()) * kr.C)
    return worst


def test_bands_leave_the_margin_on_every_case():
    orc.require_extended_precision()
    top = {}
    for case in kr.CASES:
        w = _ratios(*case)
        print(case, " ".join("%s %.3g" % kv for kv in sorted(w.items())))
        for k, v in w.items():
            top[k] = max(top.get(k, 0.0), v)
            assert v <= kr.C / MARGIN, (case, k, v)
    print("largest |fp64 restatement - long double| / (band / C):", top)


def test_plugin_form_is_the_recorded_single_gp_interval():
    fx = golden("gv_mlegp_recovered.json")
    names, res = read_table(os.path.join(DATA, "gv", "results_50_1.txt"))
    rec = {n: res[:, i] for i, n in enumerate(names)}
    D, y, _, _ = load_gv(50)
    row = np.concatenate([[1.0], fx["theta"]])
    ref = kr.reference(D, y, row, 1, res[:, :9])
    mean = np.asarray(ref["mean"], dtype=np.float64)
    se = np.sqrt(np.asarray(kr.variance(ref, kr.PLUGIN, fx["sigma2"]), dtype=np.float64))
    qt = student_t.ppf(0.975, D.shape[0] - 1)
    np.testing.assert_allclose(mean, rec["y.hat.single"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(mean - qt * se, rec["LL.single"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(mean + qt * se, rec["UL.single"], rtol=0, atol=1e-7)


def test_unbiased_form_is_the_1d_scripts_arithmetic():
    """n = 8, nu = 5, a scale at which neighbouring points correlate at about 0.5: R is well conditioned and no variance
    cancels, so the literal fp64 arithmetic of D1:481-516 (solve, S, Q.sq) carries 1e-12 relative."""
    n, nu, theta, sigma2 = 8, 5.0, 0.1, 0.7
    x = (np.arange(n) + np.array([0.3, 0.7, 0.2, 0.5, 0.8, 0.4, 0.6, 0.1])) / n
    y = np.sin(5.0 * x) + 0.5 * x
    sites = np.array([0.05, 0.31, 0.52, 0.77, 1.2])
    R = orc.corr_matrix_matern(nu, x[:, None], theta)
    r = np.stack([orc.corr_vec_matern(t, x[:, None], theta, nu) for t in sites])
    assert np.linalg.cond(R) < 100.0
    var, want = kr.literal_d1_unbiased(R, r, y, sigma2)
    ld = np.longdouble
    ref = kr.reference(x[:, None], y, np.array([1.0, theta]), 1, sites[:, None], Rc=[R.astype(ld)], rc=[r.astype(ld)], rho=0.0,
                       rho_t=np.zeros(len(sites)))
    assert (want > 1e-2 * float(ref["Q"]) / (n - 1)).all()                      # nothing cancels
    np.testing.assert_allclose(np.asarray(kr.variance(ref, kr.UNBIASED), dtype=np.float64), want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.asarray(kr.variance(ref, kr.ORDINARY, sigma2), dtype=np.float64), var, rtol=1e-12, atol=0)
