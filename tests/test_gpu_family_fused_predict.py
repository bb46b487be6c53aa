"""Prediction and leave-one-out of the 1-D families on the register-resident evaluator (CCGP_OPT_FAMILY_FUSED_PREDICT: the FAM
instances of csrc/small_reg.hip that keep their factor or carry identity rows, site_corr_family_kernel, site_solve_kernel):
the Matern and Matern + spline kernels at d = 1, n <= 32, where the blocked sweep served these calls before.

Held, always with option 12 on and nu = 2.5 unless a case says otherwise; the tier is read from the timing counters (fused > 0
and diag == 0 on the new route, the reverse on the sweep):
  option        option 12 takes 0 and 1 only; option 11 alone leaves prediction and leave-one-out on the sweep;
  routes        n = 33, K = 4 and CCGP_OPT_PREDICT_FACTOR = 0 keep the sweep and the option-off bits (leave-one-out, whose
                domain neither K = 4 nor that option bounds, stays fused there); d = 2 and family 2 with K = 3 keep their
                refusal;
  prediction    mean, variance and beta inside oracle.predict_bands(parts, sigma2, PREDICT_TOL_C), built by
                tests/test_gpu_family_end_to_end.reference(...)["predict"] from the exact entries of tests/family_exact.py
                (r un-normalised under family 2): families 1 (K = 2) and 2 at n = 4 (the smallest make_case builds), 8 (one
                block), 17 (ragged two-block) and 32 (the largest), two draws, that file's three sites; Matern K = 1 at nu = 5,
                n = 8 and Matern K = 3 at n = 9, built the same way per component.  cond1 <= 1e8 asserted from the references;
  leave-one-out loo_ref.family_reference / loo_ref.bands in all three variance forms with a sigma2 per row, at (family, n) =
                (1, 8), (1, 17), (1, 32), (2, 8), (2, 17); family 2 on the normalised R only, as tests/test_gpu_loo.py says;
  structure     a site's column has the same bits at positions 0, 63, 69 of an m = 70 list and in a list of its own, and so
                have the leading columns at m = 64 and m = 65; a draw's row has the same bits alone (S = 2: the 16 x 16 wide
                form) and inside S = 70 (the 8 x 8 form), also under a workspace limit of 1 MB -- on a fresh handle, where that
                limit cuts the call into chunks of 64 and 6 draws; the same for loo_batch with B = 2 and B = 70;
  one path      krige_predict_batch(ORDINARY) has predict_batch's bits; predict_summary is the summary of predict_batch's own
                tables and loo_summary that of loo_batch's (tests/test_gpu_predict_summary.check); the _dev forms equal the
                host-pointer forms, and after ccgp_reserve they allocate nothing;
  failure       a duplicated design point gives the 1-based pivot index and NaN rows in both tables; a draw whose matrix is
                singular on its own (theta = 1e12: every entry exactly 1, pivot 2) fails alone and the other draws keep their
                bits; a NaN site gives NaN in its column alone; a NaN design coordinate poisons every draw;
  history       the same bits after ccgp_debug_fill_scratch(0x00 / 0xFF) and after a Gaussian call of another shape;
  python        CombinedGP1D(5, fused_predict=True): fit.compare_GP(exact=True, single=...) and fit.leave_one_out(single=...)
                return what the entry points return when called directly; a second object with fused_predict=False on the
                same handle keeps the sweep.

Nothing in a band comes from a device run.  Measured on an MI355X (test_zz_report_headroom): see DESIGN.md K19.
"""
import functools
import math

import numpy as np
import pytest

import family_exact as fx
import loo_ref as lr
import test_gpu_failure_contract as fc
import test_gpu_family_end_to_end as fe
import test_gpu_family_fused as ff
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import _timed

pytestmark = pytest.mark.gpu

EPS = fx.EPS
NU = fe.NU
SIGMA2 = fe.SIGMA2
KAPPA_MAX = 1e8
C = orc.PREDICT_TOL_C
MAX_RATIO = {}
PREDICT_CASES = [(fam, n) for fam in (1, 2) for n in (4, 8, 17, 32)]
EXTRA_CASES = [(5.0, 1, 8), (NU, 3, 9)]                       # (nu, K, n), Matern
LOO_CASES = [(1, 8), (1, 17), (1, 32), (2, 8), (2, 17)]
LEVELS = (0.025, 0.5, 0.975)


def same_bits(a, b):
    return ff.same_bits(a, b)


def _all_same(got, want):
    for g, w in zip(got, want):
        assert same_bits(g, w)


def _kernel_id(family):
    from ccgp_amd import api
    return api.KERNEL_MATERN if family == 1 else api.KERNEL_MATERN_SPLINE


class family_predict:
    """The handle under a 1-D family with option 12 at `on` (and option 11 at `loglik`); Gaussian and 0 afterwards."""

    def __init__(self, h, family, nu=NU, on=1, loglik=0):
        self.h, self.family, self.nu, self.on, self.loglik = h, family, nu, on, loglik

    def __enter__(self):
        from ccgp_amd import api
        self.h.set_kernel(_kernel_id(self.family), self.nu)
        self.h.set_option(api.OPT_FAMILY_FUSED, self.loglik)
        self.h.set_option(api.OPT_FAMILY_FUSED_PREDICT, self.on)
        return self.h

    def __exit__(self, *exc):
        from ccgp_amd import api
        self.h.set_option(api.OPT_FAMILY_FUSED_PREDICT, 0)
        self.h.set_option(api.OPT_FAMILY_FUSED, 0)
        self.h.set_kernel(api.KERNEL_GAUSS, 0.0)


def _fused(t):
    assert t["fused"][1] > 0 and t["diag"][1] == 0, t


def _sweep(t):
    assert t["fused"][1] == 0 and t["diag"][1] > 0, t


def _note(tag, ratio):
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float(ratio))


# ----------------------------------------------------------------------------- references beyond test_gpu_family_end_to_end's
@functools.lru_cache(maxsize=None)
def make_case_k(nu, K, n):
    """(x[n], y[n], rows[2, 2 K], sites[3]) of a Matern case with K components: tests/test_gpu_family_fused.design's jittered
    grid, weights in (0.3, 0.9), theta 2 - 3 spacings, and the three kinds of site of test_gpu_family_end_to_end.make_case."""
    rng = np.random.default_rng(9100 + 10 * n + K + int(10 * nu))
    x, y = ff.design(n, rng)
    h = 1.0 / n
    rows = np.column_stack([rng.uniform(0.3, 0.9, 2) for _ in range(K)] + [rng.uniform(2.0, 3.0, 2) * h for _ in range(K)])
    sites = np.array([x[n // 2], x[3] + 1e-3 * h, 0.5 * (x[n - 2] + x[n - 1])])
    for a in (x, y, rows, sites):
        a.setflags(write=False)
    return x, y, rows, sites


def _mix_k(row, K, tables):
    """test_gpu_family_end_to_end._mix for K components (normalised)."""
    w2 = row[:K] ** 2
    val = sum(w2[c] * tables[c].hi for c in range(K)) / w2.sum()
    return val, sum(w2[c] * tables[c].band for c in range(K)) / w2.sum() + 2.0 * EPS * np.abs(val)


@functools.lru_cache(maxsize=None)
def reference_k(nu, K, n, b):
    """(parts, bands, cond1) of one draw, as test_gpu_family_end_to_end.reference builds its "predict" entry."""
    x, y, rows, sites = make_case_k(nu, K, n)
    row, X = rows[b], x[:, None]
    gram = [fx.table(1, nu, (1.0,), (row[K + c],), x, x) for c in range(K)]
    cross = [fx.table(1, nu, (1.0,), (row[K + c],), sites, x) for c in range(K)]
    val, band = _mix_k(row, K, gram)
    off = band * (1.0 - np.eye(n))                                            # the device's diagonal is exactly 1
    f = orc.predict_factor(X, y, row, K, 1, np.longdouble, Rc=[T.longdouble() for T in gram])
    rval, rband = _mix_k(row, K, cross)
    aL = np.abs(np.asarray(f["L"], dtype=np.float64))
    rho_t = np.array([fe._rho(rband[t], rval[t]) for t in range(len(sites))])
    parts = orc.predict_parts(X, y, row, K, 1, SIGMA2, sites[:, None], np.longdouble, factor=f, rc=[T.longdouble() for T in cross],
                              raw_r=False, rho=fe._rho(off, aL @ aL.T), rho_t=rho_t)
    return parts, orc.predict_bands(parts, SIGMA2, C), orc.cond1(f["R"], f["Rinv"])


def _check_tables(tag, ref, mean, var, beta):
    """One draw's rows against (parts, bands, cond1): test_gpu_family_end_to_end.test_predict_tables_exact's assertions."""
    parts, band, kappa = ref
    assert kappa <= KAPPA_MAX, (tag, kappa)
    e_var = np.abs(var - np.asarray(parts["var"], dtype=np.float64)) / band["var"]
    e_mean = np.abs(mean - np.asarray(parts["mean"], dtype=np.float64)) / band["mean"]
    e_beta = abs(beta - float(parts["beta"])) / band["beta"]
    print("%s cond1 %.3g rho %.3g rho_t %s: var %.3g mean %.3g beta %.3g (x band / C)" % (
        tag, kappa, parts["rho"], np.array2string(np.asarray(parts["rho_t"]), precision=3), e_var.max() * C, e_mean.max() * C, e_beta * C))
    for name, e in (("var", e_var.max()), ("mean", e_mean.max()), ("beta", e_beta)):
        _note("predict/%s (of PREDICT_TOL_C = %g)" % (name, C), e * C)
    assert (e_var <= 1.0).all() and (e_mean <= 1.0).all() and e_beta <= 1.0, (tag, e_var, e_mean, e_beta)


# ----------------------------------------------------------------------------- 1. the option
def test_the_option_takes_zero_and_one(handle):
    from ccgp_amd import api
    assert api.OPT_FAMILY_FUSED_PREDICT == 12
    for bad in (2, -1):
        with pytest.raises(api.CcgpError) as e:
            handle.set_option(api.OPT_FAMILY_FUSED_PREDICT, bad)
        assert e.value.code == -1
    handle.set_option(api.OPT_FAMILY_FUSED_PREDICT, 1)
    handle.set_option(api.OPT_FAMILY_FUSED_PREDICT, 0)


def test_option_11_alone_keeps_prediction_and_loo_on_the_sweep(handle):
    x, y, rows, sites = fe.make_case(1, 8)
    X = x[:, None]
    with family_predict(handle, 1, on=0, loglik=0):
        want_p = handle.predict_batch(X, y, 2, rows, sites[:, None], SIGMA2)
        want_l = handle.loo_batch(X, y, 2, rows, [1.3, 0.13], lr.ORDINARY)
    with family_predict(handle, 1, on=0, loglik=1):
        got_p, tp = _timed(handle, lambda: handle.predict_batch(X, y, 2, rows, sites[:, None], SIGMA2))
        got_l, tl = _timed(handle, lambda: handle.loo_batch(X, y, 2, rows, [1.3, 0.13], lr.ORDINARY))
        _, tll = _timed(handle, lambda: handle.loglik_batch(X, y, 2, rows, 1.0))
    _sweep(tp)
    _sweep(tl)
    _fused(tll)                                                               # what option 11 moves, it still moves
    _all_same(got_p, want_p)
    _all_same(got_l, want_l)
    # and option 12 alone moves these two and not the likelihood
    with family_predict(handle, 1, on=1, loglik=0):
        _, tp = _timed(handle, lambda: handle.predict_batch(X, y, 2, rows, sites[:, None], SIGMA2))
        _, tl = _timed(handle, lambda: handle.loo_batch(X, y, 2, rows, [1.3, 0.13], lr.ORDINARY))
        _, tll = _timed(handle, lambda: handle.loglik_batch(X, y, 2, rows, 1.0))
    _fused(tp)
    _fused(tl)
    _sweep(tll)


# ----------------------------------------------------------------------------- 2. routes: the domain's edges keep the sweep
def _edge_inputs(n, K):
    rng = np.random.default_rng(3300 + n + K)
    x, y = ff.design(n, rng)
    rows = np.column_stack([rng.uniform(0.3, 0.9, 2) for _ in range(K)] + [rng.uniform(2.0, 3.0, 2) / n for _ in range(K)])
    return x[:, None], y, rows, np.array([[0.21], [x[n // 2]], [0.87]])


@pytest.mark.parametrize("n,K,factor", [(33, 2, 1), (8, 4, 1), (8, 2, 0)], ids=["n33", "K4", "predict-factor-0"])
def test_domain_edges_keep_the_sweep_and_its_bits(handle, n, K, factor):
    from ccgp_amd import api
    X, y, rows, Xt = _edge_inputs(n, K)
    s2 = [1.3, 0.13]

    def calls():
        return (handle.predict_batch(X, y, K, rows, Xt, SIGMA2), handle.krige_predict_batch(X, y, K, rows, None, Xt, api.VAR_UNBIASED),
                handle.predict_summary(X, y, K, rows, Xt, SIGMA2, LEVELS), handle.loo_batch(X, y, K, rows, s2, lr.PLUGIN))

    handle.set_option(api.OPT_PREDICT_FACTOR, factor)
    try:
        with family_predict(handle, 1, on=0):
            want = calls()
        with family_predict(handle, 1, on=1):
            got, t = _timed(handle, calls)
            loo_alone, tl = _timed(handle, lambda: handle.loo_batch(X, y, K, rows, s2, lr.PLUGIN))
    finally:
        handle.set_option(api.OPT_PREDICT_FACTOR, 1)
    for g, w in zip(got[:2], want[:2]):                                       # the three prediction entry points: the sweep's bits
        _all_same(g, w)
    for k in ("y_hat", "pred_var", "quant", "quantiles", "beta", "status"):
        assert same_bits(got[2][k], want[2][k]), k
    if n > 32:
        _sweep(t)
        _sweep(tl)
        _all_same(got[3], want[3])
        _all_same(loo_alone, want[3])
    else:
        # K = 4 and CCGP_OPT_PREDICT_FACTOR = 0 bound the prediction; leave-one-out has its own domain and stays inside it
        _fused(tl)
        assert t["diag"][1] > 0, t
        _all_same(loo_alone, got[3])


def test_shapes_a_family_refuses_stay_refused(handle):
    """d = 2 under either family and K = 3 under the two-family kernel: CCGP_EUNSUPPORTED with the option off and on."""
    from ccgp_amd import api
    rng = np.random.default_rng(5)
    X2, y = rng.random((8, 2)), rng.random(8)
    x1 = np.sort(rng.random(8))[:, None]
    for on in (0, 1):
        for family, X, K, P in ((1, X2, 2, [[0.6, 0.4, 0.3, 0.3, 0.2, 0.2]]), (2, x1, 3, [[0.5, 0.3, 0.2, 0.3, 0.3, 0.3]])):
            with family_predict(handle, family, on=on):
                for call in (lambda: handle.predict_batch(X, y, K, P, X[:2], SIGMA2), lambda: handle.loo_batch(X, y, K, P, [1.0], lr.ORDINARY)):
                    with pytest.raises(api.CcgpError) as e:
                        call()
                    assert e.value.code == -4, (on, family, e.value)          # CCGP_EUNSUPPORTED


# ----------------------------------------------------------------------------- 3. prediction, exact
@pytest.mark.parametrize("family,n", PREDICT_CASES)
def test_prediction_exact(handle, family, n):
    x, y, rows, sites = fe.make_case(family, n)
    with family_predict(handle, family):
        (mean, var, beta, st), t = _timed(handle, lambda: handle.predict_batch(x[:, None], y, 2, rows, sites[:, None], SIGMA2))
    _fused(t)
    assert not np.asarray(st).any() and mean.shape == (2, 3) and var.shape == (2, 3)
    for b in range(2):
        _check_tables("family %d n %d draw %d" % (family, n, b), fe.reference(family, n, b)["predict"], mean[b], var[b], beta[b])


@pytest.mark.parametrize("nu,K,n", EXTRA_CASES, ids=["K1-nu5-n8", "K3-n9"])
def test_prediction_exact_one_and_three_components(handle, nu, K, n):
    x, y, rows, sites = make_case_k(nu, K, n)
    with family_predict(handle, 1, nu=nu):
        (mean, var, beta, st), t = _timed(handle, lambda: handle.predict_batch(x[:, None], y, K, rows, sites[:, None], SIGMA2))
    _fused(t)
    assert not np.asarray(st).any() and mean.shape == (2, 3)
    for b in range(2):
        _check_tables("Matern nu %g K %d n %d draw %d" % (nu, K, n, b), reference_k(nu, K, n, b), mean[b], var[b], beta[b])


# ----------------------------------------------------------------------------- 4. leave-one-out, exact
@pytest.mark.parametrize("family,n", LOO_CASES)
def test_leave_one_out_exact_in_every_form(handle, family, n):
    import test_gpu_loo as tl
    x, y, rows = lr.family_case(family, n)
    s2 = np.array([1.3, 0.13])
    for form in lr.FORMS:
        with family_predict(handle, family):
            (mean, var, beta, q, st), t = _timed(handle, lambda: handle.loo_batch(x[:, None], y, 2, rows, None if form == lr.UNBIASED else s2, form))
        _fused(t)
        assert t["solve"][1] == 0, t
        assert not st.any() and mean.shape == (2, n) and var.shape == (2, n)
        for b in range(2):
            ref, bnd, _ = lr.family_reference(family, n, b)
            tl._check_row((family, n, b), "fused-family%d" % family, ref, bnd, form, s2[b], mean[b], var[b], beta[b], q[b])
    for (route, name), v in tl.MAX_RATIO.items():
        if str(route).startswith("fused-family"):
            _note("loo/%s (of PREDICT_TOL_C = %g)" % (name, C), v)


# ----------------------------------------------------------------------------- 5. structure
def _seventy_sites(sites):
    xt = np.linspace(0.013, 0.991, 70)
    xt[[0, 63, 69]] = sites
    return xt


@pytest.mark.parametrize("family,n", [(1, 17), (2, 8)])
def test_a_site_is_its_own(handle, family, n):
    x, y, rows, sites = fe.make_case(family, n)
    X, xt = x[:, None], _seventy_sites(sites)
    with family_predict(handle, family):
        alone = handle.predict_batch(X, y, 2, rows, sites[:, None], SIGMA2)
        full, t = _timed(handle, lambda: handle.predict_batch(X, y, 2, rows, xt[:, None], SIGMA2))
        m64 = handle.predict_batch(X, y, 2, rows, xt[:64, None], SIGMA2)
        m65 = handle.predict_batch(X, y, 2, rows, xt[:65, None], SIGMA2)
        rev = handle.predict_batch(X, y, 2, rows, xt[::-1, None].copy(), SIGMA2)
    _fused(t)
    assert not np.asarray(full[3]).any()
    for k in (0, 1):                                                          # mean, variance
        assert same_bits(full[k][:, [0, 63, 69]], alone[k])
        assert same_bits(m64[k], full[k][:, :64]) and same_bits(m65[k], full[k][:, :65])
        assert same_bits(rev[k][:, ::-1], full[k])
    for other in (alone, m64, m65, rev):
        assert same_bits(other[2], full[2])                                   # beta does not depend on the sites


def _seventy_rows(rows, rng):
    K = rows.shape[1] // 2
    P = np.column_stack([rng.uniform(0.3, 0.9, 70) for _ in range(K)] + [rng.uniform(0.7, 1.3, 70) * rows[0, K + c] for c in range(K)])
    P[[5, 69]] = rows
    return P


@pytest.mark.parametrize("family,n", [(1, 17), (2, 8)])
def test_a_draw_is_its_own(handle, family, n):
    from ccgp_amd import api
    x, y, rows, sites = fe.make_case(family, n)
    X, Xt = x[:, None], sites[:, None]
    P = _seventy_rows(rows, np.random.default_rng(70 + family))
    s2 = np.full(70, 0.7)
    s2[[5, 69]] = [1.3, 0.13]
    with family_predict(handle, family):
        two, t2 = _timed(handle, lambda: handle.predict_batch(X, y, 2, rows, Xt, SIGMA2))
        big, t70 = _timed(handle, lambda: handle.predict_batch(X, y, 2, P, Xt, SIGMA2))
        with fc._limit(handle, 1 << 20):
            cut, tc = _timed(handle, lambda: handle.predict_batch(X, y, 2, P, Xt, SIGMA2))
        loo2 = handle.loo_batch(X, y, 2, rows, s2[[5, 69]], lr.ORDINARY)
        loo70, tl = _timed(handle, lambda: handle.loo_batch(X, y, 2, P, s2, lr.ORDINARY))
    for t in (t2, t70, tc, tl):
        _fused(t)
    assert not np.asarray(big[3]).any() and not loo70[4].any()
    for g, w in zip(two, big):
        assert same_bits(g, w[[5, 69]])
    _all_same(cut, big)
    for g, w in zip(loo2, loo70):
        assert same_bits(g, w[[5, 69]])
    # The session's handle may hold a workspace from earlier calls, and the scratch is cut by what the handle holds.  A handle
    # that has never held more: under the limit the scratch is that of 64 draws (csrc/capi.hip kept_factor_ws_bytes: half
    # the limit, at least 64 draws), so at n = 17, where 64 draws need more than half a megabyte, the call runs as 64 + 6.
    npf = (n + 7) // 8 * 8
    per = 8 * ((8 + 3 * npf + n * (n - 1) // 2 + 7) // 8 * 8 + npf * 64)     # small_reg_sites_scratch at m <= 64
    if 64 * per <= (1 << 19):
        return
    h2 = api.Handle(0)
    try:
        h2.set_workspace_limit(1 << 20)
        with family_predict(h2, family):
            fresh, tf = _timed(h2, lambda: h2.predict_batch(X, y, 2, P, Xt, SIGMA2))
        assert 0 < h2.workspace_bytes()[0] < 70 * per, (per, h2.workspace_bytes())
    finally:
        h2.close()
    _fused(tf)
    _all_same(fresh, big)


# ----------------------------------------------------------------------------- 6. one path
@pytest.mark.parametrize("family", [1, 2])
def test_krige_ordinary_is_predict_batch(handle, family):
    from ccgp_amd import api
    x, y, rows, sites = fe.make_case(family, 8)
    X, Xt = x[:, None], sites[:, None]
    with family_predict(handle, family):
        mean, var, beta, st = handle.predict_batch(X, y, 2, rows, Xt, SIGMA2)
        k, t = _timed(handle, lambda: handle.krige_predict_batch(X, y, 2, rows, [SIGMA2, SIGMA2], Xt, api.VAR_ORDINARY))
        plug, tp = _timed(handle, lambda: handle.krige_predict_batch(X, y, 2, rows, [SIGMA2, SIGMA2], Xt, api.VAR_PLUGIN))
        unb, tu = _timed(handle, lambda: handle.krige_predict_batch(X, y, 2, rows, None, Xt, api.VAR_UNBIASED))
    for tt in (t, tp, tu):
        _fused(tt)
    assert same_bits(k[0], mean) and same_bits(k[1], var) and same_bits(k[2], beta) and not k[4].any() and not np.asarray(st).any()
    for other in (plug, unb):                                                 # the forms share mean, beta and Q
        assert same_bits(other[0], mean) and same_bits(other[2], beta) and same_bits(other[3], k[3])
    assert np.isfinite(plug[1]).all() and np.isfinite(unb[1]).all()
    if family == 1:
        # sigma2 (1 - r'R^-1 r) <= sigma2 (1 - r'R^-1 r + u^2 / s11), and the unbiased form is the ordinary one at Q / (n - 1)
        assert (plug[1] <= var).all()
        want = var * (k[3] / 7.0 / SIGMA2)[:, None]
        scale = np.maximum(np.abs(want), (k[3] / 7.0)[:, None])
        assert (np.abs(unb[1] - want) <= 64 * EPS * scale).all()


@pytest.mark.parametrize("family", [1, 2])
def test_the_summaries_are_the_summaries_of_the_tables(handle, family):
    import test_gpu_predict_summary as ps
    x, y, rows, sites = fe.make_case(family, 8)
    X = x[:, None]
    P = _seventy_rows(rows, np.random.default_rng(170 + family))[:12]
    xt = np.array([0.031, sites[1], 0.055, sites[2]])
    y_at = np.sin(9.0 * xt)
    with family_predict(handle, family):
        mean, var, beta, st = handle.predict_batch(X, y, 2, P, xt[:, None], SIGMA2)
        res, t = _timed(handle, lambda: handle.predict_summary(X, y, 2, P, xt[:, None], SIGMA2, LEVELS, y_at))
        lmean, lvar, lbeta, _, lst = handle.loo_batch(X, y, 2, P, np.full(12, SIGMA2), lr.ORDINARY)
        lres, tl = _timed(handle, lambda: handle.loo_summary(X, y, 2, P, SIGMA2, LEVELS))
    _fused(t)
    _fused(tl)
    assert not np.asarray(st).any() and not lst.any() and res["n_failed"] == 0 and lres["n_failed"] == 0
    assert same_bits(res["beta"], beta) and same_bits(lres["beta"], lbeta)
    ps.check(res, mean, var, st, LEVELS, y_at)
    ps.check(lres, lmean, lvar, lst, LEVELS, y)


def test_the_dev_forms_equal_the_host_forms_and_allocate_nothing_when_reserved(handle):
    import torch
    x, y, rows, sites = fe.make_case(1, 17)
    n, S, m = 17, 70, 70
    P, xt = _seventy_rows(rows, np.random.default_rng(270)), _seventy_sites(sites)
    y_at = np.sin(9.0 * xt)
    dev = torch.device("cuda:0")
    col = lambda a: torch.tensor(np.asarray(a, dtype=np.float64).ravel(order="F"), device=dev)  # noqa: E731
    dX, dy, dP, dXt, dyat = col(x), col(y), col(P), col(xt), col(y_at)
    d_mean, d_var = (torch.empty(S * m, dtype=torch.float64, device=dev) for _ in range(2))
    d_out = torch.empty(m * (4 + len(LEVELS)), dtype=torch.float64, device=dev)
    d_beta = torch.empty(S, dtype=torch.float64, device=dev)
    d_st = torch.empty(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with family_predict(handle, 1):
        host = handle.predict_batch(x[:, None], y, 2, P, xt[:, None], SIGMA2)
        hsum = handle.predict_summary(x[:, None], y, 2, P, xt[:, None], SIGMA2, LEVELS, y_at)
        handle.reserve(n, 1, 2, S, m)
        before = handle.workspace_bytes()
        handle.enable_timing(True)
        try:
            handle.predict_batch_dev(dX, n, 1, dy, 2, dP, S, dXt, m, SIGMA2, d_mean, d_var, d_beta, d_st)
            handle.predict_summary_dev(dX, n, 1, dy, 2, dP, S, dXt, m, SIGMA2, LEVELS, dyat, d_out, d_beta, d_st)
            handle.synchronize()
            t = handle.get_timing()
        finally:
            handle.enable_timing(False)
        assert handle.workspace_bytes() == before, (before, handle.workspace_bytes())
    _fused(t)
    assert not d_st.cpu().numpy().any()
    assert same_bits(d_mean.cpu().numpy().reshape((S, m), order="F"), host[0])
    assert same_bits(d_var.cpu().numpy().reshape((S, m), order="F"), host[1])
    assert same_bits(d_beta.cpu().numpy(), host[2])
    out = d_out.cpu().numpy().reshape((m, 4 + len(LEVELS)), order="F")
    for c, k in enumerate(("y_hat", "pred_var", "quant", "cdf_at")):
        assert same_bits(out[:, c], hsum[k]), k
    assert same_bits(out[:, 4:], hsum["quantiles"])


# ----------------------------------------------------------------------------- 6b. failure
def _three_rows(rows):
    """[good 0, singular on its own, good 1]: theta = 1e12 makes every entry of either family's matrix exactly 1 (the Matern
    switch below z^2 = 9e-20, the spline's 1 - 6 u^2 at u = 1e-12), so pivot 2 is exactly 0."""
    bad = rows[0].copy()
    bad[2:] = 1e12
    return np.stack([rows[0], bad, rows[1]])


@pytest.mark.parametrize("family", [1, 2])
def test_a_singular_draw_fails_alone_with_the_pivot_index(handle, family):
    x, y, rows, sites = fe.make_case(family, 8)
    X, Xt, P = x[:, None], sites[:, None], _three_rows(rows)
    with family_predict(handle, family):
        good = handle.predict_batch(X, y, 2, rows, Xt, SIGMA2)
        (mean, var, beta, st), t = _timed(handle, lambda: handle.predict_batch(X, y, 2, P, Xt, SIGMA2))
        lgood = handle.loo_batch(X, y, 2, rows, [1.3, 0.13], lr.ORDINARY)
        (lmean, lvar, lbeta, lq, lst), tl = _timed(handle, lambda: handle.loo_batch(X, y, 2, P, [1.3, 7.0, 0.13], lr.ORDINARY))
    _fused(t)
    _fused(tl)
    assert list(st) == [0, 2, 0] and list(lst) == [0, 2, 0]
    assert np.isnan(mean[1]).all() and np.isnan(var[1]).all() and np.isnan(beta[1])
    assert np.isnan(lmean[1]).all() and np.isnan(lvar[1]).all() and np.isnan(lbeta[1]) and np.isnan(lq[1])
    for g, w in zip((mean, var, beta), good):
        assert same_bits(g[[0, 2]], w)
    for g, w in zip((lmean, lvar, lbeta, lq), lgood):
        assert same_bits(g[[0, 2]], w)


@pytest.mark.parametrize("family", [1, 2])
def test_a_duplicated_design_point_gives_the_pivot_index(handle, family):
    x, y, rows, sites = fe.make_case(family, 17)
    xd = x.copy()
    xd[9] = xd[4]                                                              # rows 4 and 9 are equal: column 9's pivot is 0
    with family_predict(handle, family):
        (mean, var, beta, st), t = _timed(handle, lambda: handle.predict_batch(xd[:, None], y, 2, rows, sites[:, None], SIGMA2))
        (lmean, lvar, lbeta, lq, lst), tl = _timed(handle, lambda: handle.loo_batch(xd[:, None], y, 2, rows, [1.3, 0.13], lr.ORDINARY))
    _fused(t)
    _fused(tl)
    assert list(st) == [10, 10] and list(lst) == [10, 10]
    assert np.isnan(mean).all() and np.isnan(var).all() and np.isnan(beta).all()
    assert np.isnan(lmean).all() and np.isnan(lvar).all() and np.isnan(lbeta).all() and np.isnan(lq).all()


@pytest.mark.parametrize("family", [1, 2])
def test_nan_coordinates(handle, family):
    x, y, rows, sites = fe.make_case(family, 8)
    X = x[:, None]
    xt = np.array([sites[0], math.nan, sites[2], 0.02])
    xn = x.copy()
    xn[5] = math.nan
    with family_predict(handle, family):
        clean = handle.predict_batch(X, y, 2, rows, xt[[0, 2, 3], None], SIGMA2)
        (mean, var, beta, st), t = _timed(handle, lambda: handle.predict_batch(X, y, 2, rows, xt[:, None], SIGMA2))
        (pm, pv, pb, pst), tp = _timed(handle, lambda: handle.predict_batch(xn[:, None], y, 2, rows, sites[:, None], SIGMA2))
        (lm, lv, lb, lq, lst), tl = _timed(handle, lambda: handle.loo_batch(xn[:, None], y, 2, rows, [1.3, 0.13], lr.ORDINARY))
    for tt in (t, tp, tl):
        _fused(tt)
    # a NaN site: its column alone
    assert not np.asarray(st).any() and np.isnan(mean[:, 1]).all() and np.isnan(var[:, 1]).all()
    assert same_bits(mean[:, [0, 2, 3]], clean[0]) and same_bits(var[:, [0, 2, 3]], clean[1]) and same_bits(beta, clean[2])
    # a NaN design coordinate: every draw
    assert np.asarray(pst).all() and np.isnan(pm).all() and np.isnan(pv).all() and np.isnan(pb).all()
    assert lst.all() and np.isnan(lm).all() and np.isnan(lv).all() and np.isnan(lb).all()


# ----------------------------------------------------------------------------- 6c. history
@pytest.mark.parametrize("family", [1, 2])
def test_the_bits_do_not_depend_on_what_the_handle_ran_before(handle, family):
    x, y, rows, sites = fe.make_case(family, 17)
    X, xt = x[:, None], _seventy_sites(sites)

    def calls():
        return (handle.predict_batch(X, y, 2, rows, xt[:, None], SIGMA2), handle.loo_batch(X, y, 2, rows, [1.3, 0.13], lr.UNBIASED),
                handle.krige_predict_batch(X, y, 2, rows, None, xt[:5, None], 2))

    def flat(out):
        return [a for part in out for a in part]

    with family_predict(handle, family):
        want = flat(calls())
    rng = np.random.default_rng(11)
    Xg, yg = rng.random((50, 3)), rng.random(50)
    Pg = np.array([[0.6, 0.4, 1.0, 2.0, 3.0, 20.0, 30.0, 40.0]])
    try:
        for fill in (0x00, 0xFF):
            assert handle.debug_fill_scratch(fill) == 0
            with family_predict(handle, family):
                got, t = _timed(handle, calls)
            _fused(t)
            _all_same(flat(got), want)
    finally:
        handle.debug_fill_scratch(-1)
    handle.predict_batch(Xg, yg, 2, Pg, rng.random((130, 3)), 1.0)            # a Gaussian call of another shape
    handle.loo_batch(Xg, yg, 2, Pg, [1.0], lr.ORDINARY)
    with family_predict(handle, family):
        _all_same(flat(calls()), want)


# ----------------------------------------------------------------------------- 7. python
def _python_case():
    rng = np.random.default_rng(88)
    x, y = ff.design(8, rng)
    draws = np.column_stack([rng.uniform(0.3, 0.7, 64), rng.uniform(0.25, 0.4, 64), rng.uniform(0.25, 0.4, 64)])
    xt = np.linspace(0.03, 0.97, 11)
    return x, y, draws, xt, np.sin(9.0 * xt)


def test_python_surface_routes_through_the_option_and_does_not_leak(handle):
    from ccgp_amd import api, fit
    from ccgp_amd.rsurface import CombinedGP1D
    x, y, draws, xt, yt = _python_case()
    alpha, s2, theta = 0.05, 0.9, 0.31
    gp = CombinedGP1D(5, handle=handle, fused_predict=True)
    assert gp.fused_predict and not gp.fused and gp._with(2.5).fused_predict
    single = dict(theta=theta)
    cmp_, t = _timed(handle, lambda: fit.compare_GP(gp, xt, alpha, yt, draws, x, s2, y, exact=True, single=single))
    _fused(t)
    loo, tl = _timed(handle, lambda: fit.leave_one_out(gp, alpha, draws, x, s2, y, single=single))
    _fused(tl)
    tab, tt = _timed(handle, lambda: gp.prediction_table(xt, draws, x, s2, y))
    _fused(tt)
    # the entry points, called directly under the option
    P = gp.draws_to_params(x[:, None], draws)
    one = np.array([[1.0, theta]])
    with family_predict(handle, 1, nu=5.0):
        r = handle.predict_summary(x[:, None], y, 2, P, xt[:, None], s2, (alpha / 2, 1 - alpha / 2))
        pb = handle.predict_batch(x[:, None], y, 2, P, xt[:, None], s2)
        k = handle.krige_predict_batch(x[:, None], y, 1, one, None, xt[:, None], api.VAR_UNBIASED)
        lsum = handle.loo_summary(x[:, None], y, 2, P, s2, (alpha / 2, 1 - alpha / 2))
        lb = handle.loo_batch(x[:, None], y, 1, one, None, api.VAR_UNBIASED)
    assert same_bits(cmp_["y_hat"], r["y_hat"]) and same_bits(cmp_["quant"], r["quant"])
    assert same_bits(cmp_["LL"], r["quantiles"][:, 0]) and same_bits(cmp_["UL"], r["quantiles"][:, 1])
    assert same_bits(cmp_["y_hat_single"], k[0][0]) and same_bits(cmp_["single_var"], k[1][0])
    assert same_bits(tab["mean"], pb[0]) and same_bits(tab["var"], pb[1])
    assert same_bits(loo["y_hat"], lsum["y_hat"]) and same_bits(loo["pit"], lsum["cdf_at"])
    assert same_bits(loo["LL"], lsum["quantiles"][:, 0]) and same_bits(loo["UL"], lsum["quantiles"][:, 1])
    assert same_bits(loo["y_hat_single"], lb[0][0]) and same_bits(loo["single_var"], lb[1][0])
    ps_ = fit.prediction_single(handle, x, xt, y, dict(theta=theta), alpha, nu=5.0, fused_predict=True)
    assert same_bits(ps_["y_hat_single"], k[0][0]) and same_bits(ps_["single_var"], k[1][0])
    # a second object on the same handle, without the flag: the sweep -- the option did not leak
    plain = CombinedGP1D(5, handle=handle)
    assert not plain.fused_predict
    off, to = _timed(handle, lambda: fit.compare_GP(plain, xt, alpha, yt, draws, x, s2, y, exact=True, single=single))
    _sweep(to)
    _, tlo = _timed(handle, lambda: fit.leave_one_out(plain, alpha, draws, x, s2, y, single=single))
    _sweep(tlo)
    for key in ("y_hat", "LL", "UL", "y_hat_single", "single_var"):
        assert np.allclose(off[key], cmp_[key], rtol=1e-8, atol=1e-10), key   # two eliminations of the same matrices
    # fused=True alone keeps doing what it does: prediction on the sweep
    only11 = CombinedGP1D(5, handle=handle, fused=True)
    _, t11 = _timed(handle, lambda: only11.prediction(xt, alpha, draws, x, s2, y))
    _sweep(t11)


# ----------------------------------------------------------------------------- 8. headroom
def test_zz_report_headroom():
    for k in sorted(MAX_RATIO):
        print("max ratio %-44s %.3g" % (k, MAX_RATIO[k]))
