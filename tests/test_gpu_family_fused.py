"""The 1-D families on the register-resident evaluator (CCGP_OPT_FAMILY_FUSED, the FAM instances of csrc/small_reg.hip): the
Matern and Matern + spline kernels at d = 1, n <= 32, served by one launch where the blocked sweep served them before.

Held, always with the option on and nu = 2.5 unless a case says otherwise:
  option, routes  the option takes 0 and 1 only; n = 8 runs fused, n = 33 keeps the sweep; with the option off the chain and the
                  search entry points still refuse these families and touch no output (the one test here that passes without
                  the feature);
  exact           log-likelihood and beta in mean mode 0, the log-likelihood in mean mode 1, against the long-double references
                  of tests/test_gpu_family_end_to_end.py (exact entries of tests/family_exact.py, oracle.loglik_grad_parts /
                  marginal_parts) within that file's bands: GRAD_TOL_C eps cond1 (1 + rho) size and MARGINAL_TOL_C units, rho
                  from family_exact's component-wise bands, cond1 <= 1e8 / MARGINAL_COND_MAX asserted.  Families 1 (K = 2) and
                  2 at n = 8 (one block), 17 (the smallest ragged two-block shape of the 16 x 16 grid, three blocks of the 8 x 8)
                  and 32 (the largest), designs a jittered grid with theta 2 - 3 spacings; once on each grid (B = 2, and the same
                  two rows inside a call of 70: the same bits); and Matern K = 1 at nu = 5, n = 8.  Nothing in a band comes from
                  a device run;
  sets            every row of a sets call has the bits of the single-set fused call on its set (C = 3, n 8, 9, 16, 17,
                  B 1, 5, 70, `set_of` in mixed order, both mean modes, both families); cutting B changes no bit;
                  logpost_sets is logpost_batch per set;
  failure         a duplicated design point gives the 1-based pivot index and NaN in the rows of its set alone; a NaN
                  coordinate poisons its set's rows alone;
  chains, search  three chains / searches on two sets under CCGP_PRIOR_ISO (Matern K = 2 at n = 8, Matern + spline at n = 14):
                  final state and trace equal the host twin's (ccgp_chain_logpost_sets one evaluation at a time, ccgp_nm_feed)
                  bit for bit, all at once and cut into calls of 7 and of 1; the twin's chains accept and reject;
  drivers         fit.Metro_device_sets and fit.laplace_device_sets with CombinedGP1D(fused=True) stay on the device and return
                  the twin's bits; a second object with fused=False on the same handle keeps the sweep;
  history         the same bits after ccgp_debug_fill_scratch(0x00 / 0xFF) and after a Gaussian call of another shape.

The chains' seeds and step scale were chosen on the CPU with the oracle's logpost_1d / logpost_2f so that every chain has
accepted and rejected proposals; the test asserts it from the twin's trace.  The exact cases' condition numbers were checked on
the CPU from the references alone: cond1 <= 6.9e3 in mode 0 and <= 3e5 in mode 1, rho 258 ... 411.

Measured on an MI355X (test_zz_report_headroom): see DESIGN.md K18.
"""
import functools
import math

import numpy as np
import pytest

import family_exact as fx
from chain_cases import walk
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import _timed, check_loglik_beta

pytestmark = pytest.mark.gpu

EPS = fx.EPS
NU = 2.5
S2_TAU2 = (1.0, 25.0)              # tests/test_gpu_family_end_to_end.py
KAPPA_MAX = 1e8
MAX_RATIO = {}
EXACT = [(fam, n, NU, 2) for fam in (1, 2) for n in (8, 17, 32)] + [(1, 8, 5.0, 1)]
T_CHAIN = 12
EVALS = 25


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


class fused:
    """The handle under a 1-D family with the option at `on`; Gaussian and 0 afterwards, whatever happened inside."""

    def __init__(self, h, family, nu=NU, on=1):
        self.h, self.family, self.nu, self.on = h, family, nu, on

    def __enter__(self):
        from ccgp_amd import api
        self.h.set_kernel(api.KERNEL_MATERN if self.family == 1 else api.KERNEL_MATERN_SPLINE, self.nu)
        self.h.set_option(api.OPT_FAMILY_FUSED, self.on)
        return self.h

    def __exit__(self, *exc):
        from ccgp_amd import api
        self.h.set_option(api.OPT_FAMILY_FUSED, 0)
        self.h.set_kernel(api.KERNEL_GAUSS, 0.0)


# ----------------------------------------------------------------------------- inputs and references
def design(n, rng, shift=0.0):
    """A jittered grid on [0, 1] and a response with a trend, as tests/test_gpu_family_end_to_end.py builds them at n = 14."""
    x = (np.arange(n) + rng.uniform(0.2, 0.8, n)) / n
    return x, np.sin(9.0 * x + shift) + 0.3 * np.cos(31.0 * x) + 0.3 * x


@functools.lru_cache(maxsize=None)
def make_case(family, n, nu, K):
    """(x[n], y[n], rows[2, 2 K]) of one exact case: weights in (0.3, 0.9), theta 2 - 3 spacings."""
    rng = np.random.default_rng(7000 + 10 * n + family + int(10 * nu) + K)
    x, y = design(n, rng)
    h = 1.0 / n
    rows = np.column_stack([rng.uniform(0.3, 0.9, 2) if K == 2 else np.ones(2) for _ in range(K)] +
                           [rng.uniform(2.0, 3.0, 2) * h for _ in range(K)])
    for a in (x, y, rows):
        a.setflags(write=False)
    return x, y, rows


def component_tables(family, nu, row, K, x):
    """The component Tables of the Gram block (the spline alone is the pair with weights (0, 1))."""
    out = [fx.table(1, nu, (1.0,), (row[K],), x, x)]
    if K == 2:
        out.append(fx.table(1, nu, (1.0,), (row[3],), x, x) if family == 1 else
                   fx.table(2, nu, (0.0, 1.0), (row[2], row[3]), x, x, raw=True))
    return out


@functools.lru_cache(maxsize=None)
def reference(family, n, nu, K, b):
    """What one draw is held to, in long double from the exact entries: test_gpu_family_end_to_end.reference for K components."""
    x, y, rows = make_case(family, n, nu, K)
    row, X = rows[b], x[:, None]
    gram = component_tables(family, nu, row, K, x)
    Rc = [T.longdouble() for T in gram]
    w2 = row[:K] ** 2
    val = sum(w2[c] * gram[c].hi for c in range(K)) / w2.sum()
    band = sum(w2[c] * gram[c].band for c in range(K)) / w2.sum() + 2.0 * EPS * np.abs(val)
    off = band * (1.0 - np.eye(n))                                            # the device's diagonal is exactly 1
    keep = off > 0
    assert (val[keep] > 0).all()
    rho = float((off[keep] / (EPS * val[keep])).max())
    s2, tau2 = S2_TAU2
    p0 = orc.loglik_grad_parts(X, y, row, K, 1, s2, np.longdouble, Rc=Rc)
    k0 = orc.cond1(p0["Sigma"], p0["Sinv"])
    s_ll, s_beta = orc.loglik_beta_scales(p0, y)
    unit = EPS * k0 * (1.0 + rho)
    p1 = orc.marginal_parts(X, y, row, K, 1, s2, tau2, np.longdouble, Rc=Rc)
    return dict(rho=rho, mode0=(float(p0["loglik"]), float(p0["beta"]), unit * s_ll, unit * s_beta, k0),
                mode1=(float(p1["loglik"]), orc.marginal_unit(p1, X, row, K, 1, rho=rho), orc.cond1(p1["Sigma"], p1["Sinv"])))


def _note(tag, ratio):
    MAX_RATIO[tag] = max(MAX_RATIO.get(tag, 0.0), float(ratio))


# ----------------------------------------------------------------------------- option and routes
def test_the_option_takes_zero_and_one(handle):
    from ccgp_amd import api
    assert api.OPT_FAMILY_FUSED == 11
    for bad in (2, -1):
        with pytest.raises(api.CcgpError) as e:
            handle.set_option(api.OPT_FAMILY_FUSED, bad)
        assert e.value.code == -1
    handle.set_option(api.OPT_FAMILY_FUSED, 1)
    handle.set_option(api.OPT_FAMILY_FUSED, 0)


def test_routes(handle):
    x8, y8, rows8 = make_case(1, 8, NU, 2)
    rng = np.random.default_rng(33)
    x33, y33 = design(33, rng)
    rows33 = np.array([[0.6, 0.4, 2.5 / 33, 2.2 / 33]])
    with fused(handle, 1):
        (ll, _, st), t = _timed(handle, lambda: handle.loglik_batch(x8[:, None], y8, 2, rows8, 1.0))
        assert t["fused"][1] > 0 and t["diag"][1] == 0, t
        assert not st.any() and np.isfinite(ll).all()
        # beyond the instances: the blocked sweep, with the option on
        (ll33, _, st33), t = _timed(handle, lambda: handle.loglik_batch(x33[:, None], y33, 2, rows33, 1.0))
        assert t["fused"][1] == 0 and t["diag"][1] > 0, t
        assert not st33.any()
    with fused(handle, 1, on=0):
        (ll_off, _, st_off), t = _timed(handle, lambda: handle.loglik_batch(x8[:, None], y8, 2, rows8, 1.0))
        assert t["fused"][1] == 0 and t["diag"][1] > 0, t
        (ll33_off, _, _), _ = _timed(handle, lambda: handle.loglik_batch(x33[:, None], y33, 2, rows33, 1.0))
    np.testing.assert_array_equal(ll33, ll33_off)                            # n = 33: the option moves nothing
    assert np.allclose(ll, ll_off, rtol=1e-9, atol=0) and not st_off.any()   # n = 8: two eliminations of one matrix
    # the Gaussian family takes no notice of the option
    from ccgp_amd import api
    g = np.array([[0.6, 0.4, 3.0, 40.0]])
    want = handle.loglik_batch(x8[:, None], y8, 2, g, 1.0)
    handle.set_option(api.OPT_FAMILY_FUSED, 1)
    try:
        _same(handle.loglik_batch(x8[:, None], y8, 2, g, 1.0), want)
    finally:
        handle.set_option(api.OPT_FAMILY_FUSED, 0)


def _raw_search(h, n=8, d=1):
    """ccgp_laplace_search_sets through ctypes with every output pre-filled -> (rc, outputs untouched?)."""
    from ccgp_amd import api
    rng = np.random.default_rng(2)
    Xs, ys, s2 = rng.random((1, d, n)), rng.random((1, n)), np.ones(1)
    state = np.ascontiguousarray(api.nm_begin([-1.0, 0.0, 0.3])[None])
    keep = state.copy()
    me, evals = np.array([2], dtype=np.int32), np.full(1, -7, dtype=np.int32)
    v, s = np.full((1, 4), 5.0), np.full((1, 4), 9, dtype=np.int32)
    rc = api.lib().ccgp_laplace_search_sets(h._h, api._p(Xs), n, d, api._p(ys), api._p(s2), 1, api.PRIOR_ISO, None, 1,
                                            api._ipt(np.zeros(1, dtype=np.int32)), api._p(state), api._ipt(me), api._ipt(evals),
                                            api._p(v), api._ipt(s), 4)
    return rc, same_bits(state, keep) and (evals == -7).all() and (v == 5.0).all() and (s == 9).all()


def test_with_the_option_off_chains_and_searches_are_refused(handle):
    """Today's behaviour, which the option's default keeps: CCGP_EUNSUPPORTED and no output touched."""
    from ccgp_amd import api
    from test_gpu_chains import raw_call
    for family in (1, 2):
        handle.set_kernel(api.KERNEL_MATERN if family == 1 else api.KERNEL_MATERN_SPLINE, NU)
        try:
            rc, untouched = raw_call(handle, n=8, d=1)
            assert rc == -4 and untouched
            rc, untouched = _raw_search(handle)
            assert rc == -4 and untouched
        finally:
            handle.set_kernel(api.KERNEL_GAUSS, 0.0)


def test_with_the_option_on_beyond_n_32_they_are_still_refused(handle):
    from test_gpu_chains import raw_call
    with fused(handle, 1):
        rc, untouched = raw_call(handle, n=33, d=1)
        assert rc == -4 and untouched
        rc, untouched = _raw_search(handle, n=33)
        assert rc == -4 and untouched
        rc, untouched = raw_call(handle, n=32, d=1)
        assert rc >= 0 and not untouched
        rc, untouched = _raw_search(handle, n=32)
        assert rc >= 0 and not untouched


# ----------------------------------------------------------------------------- exact likelihoods
@pytest.mark.parametrize("family,n,nu,K", EXACT, ids=["family%d-n%d-nu%g-K%d" % c for c in EXACT])
def test_likelihoods_exact(handle, family, n, nu, K):
    x, y, rows = make_case(family, n, nu, K)
    s2, tau2 = S2_TAU2
    # the same two rows inside a call of 70 (the 8 x 8 grid): at positions 3 and 66 among rows with other thetas
    many = np.tile(rows, (35, 1)) * np.concatenate([np.ones((70, K)), 1.0 + 0.004 * np.arange(70)[:, None] * np.ones((1, K))], axis=1)
    many[3], many[66] = rows[0], rows[1]
    with fused(handle, family, nu):
        (ll0, beta0, st0), t0 = _timed(handle, lambda: handle.loglik_batch(x[:, None], y, K, rows, s2, 0, 0.0))
        (ll1, beta1, st1), t1 = _timed(handle, lambda: handle.loglik_batch(x[:, None], y, K, rows, s2, 1, tau2))
        big0 = handle.loglik_batch(x[:, None], y, K, many, s2, 0, 0.0)
        big1 = handle.loglik_batch(x[:, None], y, K, many, s2, 1, tau2)
    for t in (t0, t1):
        assert t["fused"][1] == 1 and t["diag"][1] == 0, t
    assert not st0.any() and not st1.any() and not big0[2].any() and not big1[2].any()
    # the two grids give the same bits
    for small, big in (((ll0, beta0), big0), ((ll1, beta1), big1)):
        assert same_bits(small[0], big[0][[3, 66]]) and same_bits(small[1], big[1][[3, 66]])
    tag = "family%d%s" % (family, "" if K == 2 else "/K1-nu5")
    for b in range(2):
        ref = reference(family, n, nu, K, b)
        ll_ref, beta_ref, unit_ll, unit_beta, kappa = ref["mode0"]
        assert kappa <= KAPPA_MAX, (family, n, b, kappa)
        r = check_loglik_beta(ll_ref, beta_ref, unit_ll, unit_beta, ll0[b], beta0[b], tag + "/mode0")
        _note("%s/mode0 (of GRAD_TOL_C = %g)" % (tag, orc.GRAD_TOL_C), max(r))
        ll_ref, unit, kappa1 = ref["mode1"]
        assert kappa1 <= orc.MARGINAL_COND_MAX, (family, n, b, kappa1)
        assert beta1[b] == 0.0
        ratio = abs(ll1[b] - ll_ref) / unit
        print("family %d n %d nu %g K %d draw %d rho %.3g: mode 0 %.3g, %.3g (cond1 %.3g); mode 1 %.3g units (cond1 %.3g)" % (
            family, n, nu, K, b, ref["rho"], r[0], r[1], kappa, ratio, kappa1))
        _note("%s/mode1 (of MARGINAL_TOL_C = %g)" % (tag, orc.MARGINAL_TOL_C), ratio)
        assert ratio <= orc.MARGINAL_TOL_C, (family, n, b, ll1[b], ll_ref, ratio)


# ----------------------------------------------------------------------------- sets
def sets_case(n, C, B, seed):
    """C designs with responses and variances, B rows (K = 2) and their sets in mixed order, every set used where B allows."""
    rng = np.random.default_rng(seed)
    pairs = [design(n, rng, shift=0.4 * c) for c in range(C)]
    Xs, ys = np.stack([p[0][:, None] for p in pairs]), np.stack([p[1] for p in pairs])
    s2 = 0.5 + rng.random(C)
    P = np.column_stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.3, 0.9, B), rng.uniform(2.0, 3.0, B) / n, rng.uniform(2.0, 3.0, B) / n])
    set_of = rng.integers(C, size=B)
    lead = list(range(C))[::-1][:B]
    set_of[:len(lead)] = lead
    return Xs, ys, s2, P, set_of.astype(np.int32)


def per_set(h, Xs, ys, s2, P, set_of, mode, tau2):
    """The reference: the rows of every set through the single-set call."""
    B = len(P)
    ll, beta, st = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    for c in np.unique(set_of):
        rows = np.flatnonzero(set_of == c)
        ll[rows], beta[rows], st[rows] = h.loglik_batch(Xs[c], ys[c], 2, P[rows], s2[c], mode, tau2)
    return ll, beta, st


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("n", [8, 9, 16, 17])
def test_sets_rows_have_the_bits_of_the_single_set_call(handle, n, B):
    Xs, ys, s2, P, set_of = sets_case(n, 3, B, 100 * n + B)
    for family in (1, 2):
        with fused(handle, family):
            for mode, tau2 in ((0, 0.0), (1, 0.5)):
                want = per_set(handle, Xs, ys, s2, P, set_of, mode, tau2)
                assert not want[2].any() and np.isfinite(want[0]).all()
                got, t = _timed(handle, lambda: handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of, mode, tau2))
                assert t["fused"][1] == 1 and t["diag"][1] == 0, t          # one launch for all sets
                _same(got, want)
                if B == 70:
                    # cut into chunks: a workspace limit of the smallest size, and the rows in two calls (both of them on the
                    # 16 x 16 grid, the whole call on the 8 x 8)
                    handle.set_workspace_limit(1 << 20)
                    try:
                        _same(handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of, mode, tau2), want)
                    finally:
                        handle.set_workspace_limit(200 << 30)
                    parts = [handle.loglik_batch_sets(Xs, ys, s2, 2, P[a:b], set_of[a:b], mode, tau2) for a, b in ((0, 33), (33, 70))]
                    _same([np.concatenate([p[k] for p in parts]) for k in range(3)], want)


@pytest.mark.parametrize("family", [1, 2])
def test_logpost_sets_is_logpost_batch_per_set(handle, family):
    from ccgp_amd import api
    n, C, B = 9, 3, 11
    Xs, ys, s2, _, set_of = sets_case(n, C, B, 900 + family)
    rng = np.random.default_rng(family)
    T = np.stack([np.log(rng.uniform(2.0, 3.0, B) / n), np.log(rng.uniform(2.0, 4.0, B) / n), rng.normal(0.0, 0.8, B)], axis=1)
    with fused(handle, family):
        got = handle.logpost_sets(Xs, ys, s2, api.PRIOR_ISO, T, set_of)
        assert not got[3].any() and np.isfinite(got[0]).all()
        for c in np.unique(set_of):
            rows = np.flatnonzero(set_of == c)
            want = handle.logpost_batch(Xs[c], ys[c], s2[c], api.PRIOR_ISO, T[rows])
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g[rows], w)
            # the value-only single call: the same evaluation through ccgp_logpost
            one = handle.logpost(Xs[c], ys[c], s2[c], api.PRIOR_ISO, T[rows[0]], want_Rinv=False)
            assert one["val"] == want[0][0] and one["beta"] == want[1][0]


# ----------------------------------------------------------------------------- failure contract
@pytest.mark.parametrize("family", [1, 2])
def test_a_duplicated_point_fails_its_own_rows_with_the_pivot_index(handle, family):
    n = 9
    Xs, ys, s2, P, set_of = sets_case(n, 3, 7, 1200 + family)
    Xs = Xs.copy()
    Xs[1, 7, 0] = Xs[1, 3, 0]                         # rows 3 and 7 of set 1 coincide: two equal rows of R, pivot 7 vanishes
    with fused(handle, family):
        ll, beta, st = handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of)
        one = handle.loglik_batch(Xs[1], ys[1], 2, P[set_of == 1], s2[1])
    hit = set_of == 1
    assert hit.any() and (~hit).any()
    assert (st[hit] == 8).all() and np.isnan(ll[hit]).all() and np.isnan(beta[hit]).all()
    assert not st[~hit].any() and np.isfinite(ll[~hit]).all() and np.isfinite(beta[~hit]).all()
    assert (one[2] == 8).all() and np.isnan(one[0]).all() and np.isnan(one[1]).all()


@pytest.mark.parametrize("family", [1, 2])
def test_a_nan_coordinate_poisons_its_own_set_alone(handle, family):
    n = 9
    Xs, ys, s2, P, set_of = sets_case(n, 3, 7, 1300 + family)
    clean = None
    Xn = Xs.copy()
    Xn[2, 4, 0] = math.nan
    with fused(handle, family):
        clean = handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of)
        ll, beta, st = handle.loglik_batch_sets(Xn, ys, s2, 2, P, set_of)
    hit = set_of == 2
    assert hit.any() and (~hit).any() and not clean[2].any()
    assert (st[hit] != 0).all() and np.isnan(ll[hit]).all() and np.isnan(beta[hit]).all()
    assert not st[~hit].any() and same_bits(ll[~hit], clean[0][~hit]) and same_bits(beta[~hit], clean[1][~hit])


# ----------------------------------------------------------------------------- chains and the search
SHAPES = [(1, 8), (2, 14)]                             # (family, n): Matern K = 2, Matern + spline
CHAIN_SEED = {(1, 8): 11, (2, 14): 12}
CHAIN_SCALE = 0.6


@functools.lru_cache(maxsize=None)
def chain_problem(family, n):
    """Two training sets of one shape and three chains on them (sets 1, 0, 1): chain_cases.make_case's dicts."""
    from ccgp_amd import api
    rng = np.random.default_rng(CHAIN_SEED[(family, n)])
    sets = []
    for c in range(2):
        x, y = design(n, rng, shift=0.7 * c)
        sets.append(dict(D=x[:, None], y=y, s2=float(np.var(y, ddof=1))))
    set_of = [1, 0, 1]
    theta0 = np.array([math.log(2.5 / n), math.log(4.0 / n), 0.3])
    cases = []
    for a, c in enumerate(set_of):
        cases.append(dict(sets[c], prior=api.PRIOR_ISO, pars=None, script="D1", theta0=theta0 + 0.1 * a,
                          steps=CHAIN_SCALE * rng.standard_normal((T_CHAIN, 3)), logu=np.log(rng.random(T_CHAIN))))
    return sets, set_of, cases


def twin_walk(h, case):
    def ev(theta):
        val, beta, _, st = h.chain_logpost_sets(case["D"][None], case["y"][None], [case["s2"]], case["prior"], theta[None], [0])
        return float(val[0]), float(beta[0]), int(st[0])
    return walk(case, ev)


@pytest.mark.parametrize("family,n", SHAPES)
def test_device_chains_equal_the_host_twin(handle, family, n):
    from test_gpu_chains import check_against_walk, device_run
    sets, set_of, cases = chain_problem(family, n)
    with fused(handle, family):
        walks = [twin_walk(handle, c) for c in cases]
        for tr in walks:
            acc = sum(tr["accept"])
            print("family %d n %d: accepted %d rejected %d" % (family, n, acc, T_CHAIN - acc))
            assert 1 <= acc <= T_CHAIN - 1 and not any(tr["status"])
        # all at once: one launch carries the three chains to their end
        r, t = _timed(handle, lambda: device_run(handle, cases, sets=sets, set_of=set_of))
        assert t["diag"][1] == 0 and t["fused"][1] >= 1, t
        for j, tr in enumerate(walks):
            check_against_walk(r, j, tr, used=T_CHAIN)
        assert r["failed"] == 0
        # cut into calls of 7 and of 1, the state of one call the start of the next
        for cut in (7, 1):
            state, t0 = None, 0
            vals, accs = [[] for _ in cases], [[] for _ in cases]
            while t0 < T_CHAIN:
                m = min(cut, T_CHAIN - t0)
                r = device_run(handle, cases, n_prop=[m] * 3, stop_acc=[m] * 3, state=state, t0=t0, sets=sets, set_of=set_of)
                assert (r["used"] == m).all()
                for j in range(3):
                    vals[j] += list(r["trace_val"][j, :m])
                    accs[j] += list(r["trace_accept"][j, :m])
                state = [(r["theta"][j], float(r["l"][j]), float(r["beta"][j])) for j in range(3)]
                t0 += m
            for j, tr in enumerate(walks):
                assert same_bits(vals[j], tr["val"]) and accs[j] == tr["accept"], (cut, j)
                assert same_bits(state[j][0], tr["theta"]) and same_bits(state[j][1], tr["l"]) and same_bits(state[j][2], tr["beta_fin"])


@pytest.mark.parametrize("family,n", SHAPES)
def test_device_searches_equal_the_host_twin(handle, family, n):
    from ccgp_amd import api
    from test_gpu_device_laplace import check, search, twin
    sets, set_of, cases = chain_problem(family, n)
    p = dict(Xs=np.stack([s["D"] for s in sets]), ys=np.stack([s["y"] for s in sets]), s2=[s["s2"] for s in sets],
             prior=api.PRIOR_ISO, pars=None)
    s0 = np.stack([api.nm_begin(c["theta0"]) for c in cases])
    with fused(handle, family):
        want, tr_v, tr_s = twin(handle, p, set_of, s0, max_evals=EVALS)
        assert all(len(v) == EVALS for v in tr_v) and np.isfinite(np.array(tr_v)).all()
        r, t = _timed(handle, lambda: search(handle, p, set_of, s0, EVALS))
        assert t["diag"][1] == 0 and t["fused"][1] == 1, t
        for j in range(3):
            check(r, j, want[j], tr_v[j], tr_s[j])
        assert r["failed"] == 0
        for cut in (7, 1):
            state, t0 = s0, 0
            while t0 < EVALS:
                m = min(cut, EVALS - t0)
                r = search(handle, p, set_of, state, m)
                for j in range(3):
                    check(r, j, None, tr_v[j], tr_s[j], t0, m)
                state, t0 = r["state"], t0 + m
            assert same_bits(state, want), cut


# ----------------------------------------------------------------------------- drivers
def test_drivers_stay_on_the_device(handle):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP1D
    gp = CombinedGP1D(NU, handle=handle, fused=True)
    x = np.linspace(0.0, 1.0, 8)[:, None]
    y = np.sin(5.0 * x[:, 0]) + 0.3 * x[:, 0]
    mode = np.array([-1.0, 0.0, 0.3])
    # the chains: tests/test_gpu_chains.py test_fallback_where_the_device_refuses' settings
    est = dict(mode=mode, var=0.02 * np.eye(3), converged=True, value=0.0)
    kw = dict(N=12, samp_size=8, batch_size=4, alpha=2.0)
    a = fit.Metro_device_sets(gp, None, D_trains=[x], sigma2s=[1.0], ys=[y], rngs=[1], laplace=[est], max_proposals=60, **kw)
    b = fit.Metro_device_sets(gp, None, D_trains=[x], sigma2s=[1.0], ys=[y], rngs=[1], laplace=[est], max_proposals=60,
                              on_device=False, **kw)
    assert a["chains"][0]["accepted"] >= 8 and same_bits(a["chains"][0]["sample"], b["chains"][0]["sample"])
    assert same_bits(a["chains"][0]["beta"], b["chains"][0]["beta"])
    assert a["chains"][0]["proposals"] == b["chains"][0]["proposals"]
    assert a["device_batches"] < b["device_batches"]
    # the search: laplace_sets over the twin evaluator, every key
    Xs, Y, s2 = np.stack([x, x]), np.stack([y, y + 0.2 * x[:, 0]]), [1.0, 1.3]

    def fn(rows, set_of):
        return gp.h.chain_logpost_sets(Xs, Y, s2, gp.cfg["prior"], rows, set_of)[0]

    starts = np.stack([mode, mode + 0.2])
    want = fit.laplace_sets(fn, starts)
    got = fit.laplace_device_sets(gp, Xs, Y, s2, starts)
    for g, w in zip(got, want):
        assert sorted(set(g) - set(w)) == ["calls", "fed"] and g["calls"] == -(-g["fed"] // 512) + 1
        for k in w:
            assert same_bits(g[k], w[k]), k
    # a second object without `fused` on the same handle: the blocked sweep, as before
    plain = CombinedGP1D(NU, handle=handle)
    rows = np.array([[0.6, 0.4, 0.4, 1.0]])
    (_, _, st), t = _timed(handle, lambda: plain.h.loglik_batch(x, y, 2, rows, 1.0))
    assert t["fused"][1] == 0 and t["diag"][1] > 0 and not st.any(), t
    (_, _, st), t = _timed(handle, lambda: gp.h.loglik_batch(x, y, 2, rows, 1.0))
    assert t["fused"][1] == 1 and t["diag"][1] == 0 and not st.any(), t
    from ccgp_amd import api
    with pytest.raises(api.CcgpError) as e:
        plain.h.metro_segments_sets(Xs, Y, s2, plain.cfg["prior"], [0], mode[None], [0.0], np.zeros((1, 4, 3)), np.zeros((1, 4)), [4], [4])
    assert e.value.code == -4
    # matern_MLEs(fused=True): every call of the search on the fused route, the optimum of the sweep's search.  The two
    # objectives differ by rounding (1e-12 of their value), which moves the minimiser of a smooth minimum by about its square
    # root, 1e-6 of theta; 1e-4 leaves two orders
    m0 = fit.matern_MLEs(handle, x, y, NU)
    m1, t = _timed(handle, lambda: fit.matern_MLEs(handle, x, y, NU, fused=True))
    assert t["fused"][1] > 0 and t["diag"][1] == 0, t
    for k in ("theta", "sigma2", "beta"):
        assert m1[k] == pytest.approx(m0[k], rel=1e-4, abs=1e-6), (k, m0, m1)
    (_, _, st), t = _timed(handle, lambda: handle.loglik_batch(x, y, 2, np.array([[0.6, 0.4, 3.0, 40.0]]), 1.0))
    assert not st.any()                                  # and the handle is Gaussian again, option off


# ----------------------------------------------------------------------------- history
def test_bits_do_not_depend_on_the_handles_history(handle):
    from test_gpu_chains import device_run
    Xs, ys, s2, P, set_of = sets_case(17, 3, 70, 1700)
    sets, chain_sets, cases = chain_problem(1, 8)
    rng = np.random.default_rng(64)
    Xg = rng.random((64, 3))

    def both():
        with fused(handle, 1):
            a = handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of)
            r = device_run(handle, cases, sets=sets, set_of=chain_sets)
        return a, r

    want_sets, want_chain = both()
    assert not want_sets[2].any()
    try:
        for fill in (0x00, 0xFF, None):
            if fill is None:   # an unrelated Gaussian call of another shape
                handle.loglik_batch(Xg, np.sin(3.0 * Xg).sum(axis=1), 2, np.tile([0.5, 0.5, 1.0, 2.0, 3.0, 30.0, 40.0, 50.0], (5, 1)), 1.0)
            else:
                handle.debug_fill_scratch(fill)
            got_sets, got_chain = both()
            _same(got_sets, want_sets)
            for k in ("theta", "l", "beta", "draws", "draw_val", "draw_beta", "trace_val", "trace_beta"):
                assert same_bits(got_chain[k], want_chain[k]), (fill, k)
            for k in ("used", "accepted", "trace_status", "trace_accept"):
                assert np.array_equal(got_chain[k], want_chain[k]), (fill, k)
    finally:
        handle.debug_fill_scratch(-1)


def test_zz_report_headroom():
    for k in sorted(MAX_RATIO):
        print("max ratio %-48s %.3g" % (k, MAX_RATIO[k]))
