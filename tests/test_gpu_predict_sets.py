"""The Combined GP's and the single GP's prediction over many training sets of one shape: ccgp_predict_batch_sets,
ccgp_krige_predict_batch_sets and ccgp_predict_summary_sets.

The contract is one of BITS: row b (for the summary: set c's block) has exactly the bits the single-set entry point returns
on that set alone, whatever C, B, the row's position, the order of `set`, the workspace limit or what the handle ran
before.  Every comparison is np.testing.assert_array_equal on float64 (NaN == NaN), never a tolerance; the reference is the
single-set entry point on the same handle.  `set` is drawn as tests/test_gpu_sets.py draws it: unsorted, uneven counts, one
set without rows when C >= 3.

Shapes (n, d, K, C, B, m).  Where the single-set call keeps its factor: the smallest everything; one partial batch of sites;
padding rows and exactly one full batch; a batch boundary; the Ground-Vibrations size-50 sets with their own test sites; the
largest order on the 8 x 8 grid; the first on the 16 x 16 grid with sites beyond one workgroup's four batches; the last
kept-factor order.  Where it does not: 105 and 128 (extra rows), K = 4, n = 129 (the blocked sweep), the option switched off,
and Matern nu = 5 with the fused prediction on and off.  Singular rows: every theta = 1e-4 at d <= 3 (tests/test_gpu_loo.py)."""
import numpy as np
import pytest

from conftest import load_gv
from test_gpu_sets import _sets_case
from ccgp_amd import api

pytestmark = pytest.mark.gpu
EINVAL = -1
KEPT = [(5, 1, 1, 2, 3, 1), (14, 2, 2, 3, 7, 7), (17, 2, 1, 3, 6, 64), (40, 3, 2, 2, 5, 65), (50, 9, 2, 9, 45, 150),
        (64, 4, 2, 2, 5, 14), (65, 3, 3, 2, 4, 257), (104, 2, 2, 2, 4, 5)]
OTHER = [(105, 2, 2, 2, 4, 5), (128, 3, 3, 2, 4, 3), (20, 2, 4, 2, 4, 5), (129, 2, 2, 2, 3, 3)]
SUMMARY_KEYS = ("y_hat", "pred_var", "quant", "cdf_at", "quantiles", "beta", "status")
PROBS = {0: (), 2: (0.025, 0.975), 8: (0.01, 0.05, 0.25, 0.5, 0.6, 0.75, 0.95, 0.99)}
_CASES = {}


def _ids(shapes):
    return ["n%d-d%d-K%d-C%d-B%d-m%d" % s for s in shapes]


def _case(n, d, K, C, B, m, seed=0):
    """_sets_case plus m test sites and held-out responses per set and a sigma2 per row; built once, shared, read-only."""
    key = (n, d, K, C, B, m, seed)
    if key not in _CASES:
        Xs, ys, s2, P, set_of = _sets_case(n, d, K, C, B, 500 + n + seed)
        rng = np.random.default_rng(7000 + n + seed)
        if (n, d) == (50, 9):
            gv = [load_gv(50, c + 1) for c in range(C)]
            Xt, yt = np.stack([g[2][:m] for g in gv]), np.stack([g[3][:m] for g in gv])
        else:
            Xt, yt = rng.random((C, m, d)), rng.standard_normal((C, m))
        row_s2 = 0.5 + rng.random(B)
        for a in (Xs, ys, s2, P, set_of, Xt, yt, row_s2):
            a.setflags(write=False)
        _CASES[key] = (Xs, ys, s2, P, set_of, Xt, yt, row_s2)
    return _CASES[key]


def _rows(set_of, C):
    return [np.flatnonzero(np.asarray(set_of) == c) for c in range(C)]


def _ref_predict(h, case, K, set_of=None, P=None):
    Xs, ys, s2, P0, set0, Xt = case[:6]
    P, set_of = (P0 if P is None else P), (set0 if set_of is None else set_of)
    B, m = len(P), Xt.shape[1]
    mean, var, beta, st = np.full((B, m), np.nan), np.full((B, m), np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    for c, rows in enumerate(_rows(set_of, len(Xs))):
        if rows.size:
            mean[rows], var[rows], beta[rows], st[rows] = h.predict_batch(Xs[c], ys[c], K, P[rows], Xt[c], s2[c])
    return mean, var, beta, st


def _ref_krige(h, case, K, form, set_of=None, P=None, row_s2=None):
    Xs, ys, _, P0, set0, Xt, _, s20 = case
    P, set_of, row_s2 = (P0 if P is None else P), (set0 if set_of is None else set_of), (s20 if row_s2 is None else row_s2)
    B, m = len(P), Xt.shape[1]
    out = [np.full((B, m), np.nan), np.full((B, m), np.nan), np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)]
    for c, rows in enumerate(_rows(set_of, len(Xs))):
        if rows.size:
            r = h.krige_predict_batch(Xs[c], ys[c], K, P[rows], None if form == api.VAR_UNBIASED else row_s2[rows], Xt[c], form)
            for o, v in zip(out, r):
                o[rows] = v
    return tuple(out)


def _ref_summary(h, case, K, probs, with_at, set_of=None, P=None):
    Xs, ys, s2, P0, set0, Xt, yt = case[:7]
    P, set_of = (P0 if P is None else P), (set0 if set_of is None else set_of)
    res = []
    for c, rows in enumerate(_rows(set_of, len(Xs))):
        res.append(h.predict_summary(Xs[c], ys[c], K, P[rows], Xt[c], s2[c], probs, yt[c] if with_at else None)
                   if rows.size else None)
    return res


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _same_summaries(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None:   # no row: NaN throughout
            assert all(np.all(np.isnan(g[k])) for k in SUMMARY_KEYS[:5]) and g["beta"].size == 0 and g["n_failed"] == 0
            continue
        assert g["n_failed"] == w["n_failed"]
        for k in SUMMARY_KEYS:
            np.testing.assert_array_equal(g[k], w[k], err_msg=k)


def _check_all(h, case, K, forms=(api.VAR_PLUGIN,), n_probs=(2,), at=(True,), expect_clean=True):
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = case
    want = _ref_predict(h, case, K)
    assert not expect_clean or (not want[3].any() and np.all(np.isfinite(want[0])))
    _same(h.predict_batch_sets(Xs, ys, s2, K, P, set_of, Xt), want)
    for form in forms:
        s2r = None if form == api.VAR_UNBIASED else row_s2
        _same(h.krige_predict_batch_sets(Xs, ys, K, P, set_of, s2r, Xt, form), _ref_krige(h, case, K, form))
    for npr in n_probs:
        for with_at in at:
            got = h.predict_summary_sets(Xs, ys, s2, K, P, set_of, Xt, PROBS[npr], yt if with_at else None)
            _same_summaries(got, _ref_summary(h, case, K, PROBS[npr], with_at))


# ----------------------------------------------------------------------------- 1. bits against the single-set calls
@pytest.mark.parametrize("n,d,K,C,B,m", KEPT, ids=_ids(KEPT))
def test_kept_factor_shapes(handle, n, d, K, C, B, m):
    _check_all(handle, _case(n, d, K, C, B, m), K)
    if K > 1 and (n, d) != (50, 9):   # the single GP has one component: the same design with K = 1 rows
        _check_all(handle, _case(n, d, 1, C, B, m, seed=1), 1, n_probs=())


def test_every_variance_form_and_every_summary_size(handle):
    _check_all(handle, _case(14, 2, 2, 3, 7, 7), 2, forms=(api.VAR_ORDINARY, api.VAR_PLUGIN, api.VAR_UNBIASED),
               n_probs=(0, 2, 8), at=(True, False))
    _check_all(handle, _case(14, 2, 1, 3, 7, 7, seed=1), 1, forms=(api.VAR_ORDINARY, api.VAR_PLUGIN, api.VAR_UNBIASED),
               n_probs=(0, 8), at=(True, False))


@pytest.mark.parametrize("n,d,K,C,B,m", OTHER, ids=_ids(OTHER))
def test_shapes_without_a_kept_factor(handle, n, d, K, C, B, m):
    _check_all(handle, _case(n, d, K, C, B, m), K, n_probs=(0, 2), at=(True, False))


def test_with_the_kept_factor_switched_off():
    h = api.Handle(0)
    try:
        h.set_option(api.OPT_PREDICT_FACTOR, 0)
        _check_all(h, _case(14, 2, 2, 3, 7, 7), 2, n_probs=(0, 2), at=(True, False))
    finally:
        h.close()


@pytest.mark.parametrize("fused", [0, 1], ids=["sweep", "fused_predict"])
def test_matern_family(fused):
    h = api.Handle(0)
    try:
        h.set_kernel(api.KERNEL_MATERN, 5.0)
        h.set_option(api.OPT_FAMILY_FUSED_PREDICT, fused)
        Xs, ys, s2, P, set_of, Xt, yt, row_s2 = _case(8, 1, 2, 3, 6, 9)
        P = np.concatenate([P[:, :2], np.random.default_rng(3).uniform(0.5, 3.0, (6, 2))], axis=1)   # theta on the 1-D scale
        case = (Xs, ys, s2, P, set_of, Xt, yt, row_s2)
        _check_all(h, case, 2, forms=(api.VAR_PLUGIN, api.VAR_UNBIASED), n_probs=(0, 2), at=(True, False))
    finally:
        h.close()


# ----------------------------------------------------------------------------- 1b. route
def test_a_kept_factor_shape_is_one_set_of_launches_and_another_goes_set_by_set(handle):
    """One timed section for all nine Ground-Vibrations sets where the single-set call keeps its factor; one per set with rows
    where it does not (n = 105: the extra-row instances), and with the option off."""
    from test_gpu_gradient_exact import _timed
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = _case(50, 9, 2, 9, 45, 150)
    for call in (lambda h: h.predict_batch_sets(Xs, ys, s2, 2, P, set_of, Xt),
                 lambda h: h.krige_predict_batch_sets(Xs, ys, 2, P, set_of, row_s2, Xt, api.VAR_PLUGIN),
                 lambda h: h.predict_summary_sets(Xs, ys, s2, 2, P, set_of, Xt, PROBS[2], yt)):
        _, t = _timed(handle, lambda: call(handle))
        assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t
        off = api.Handle(0)
        try:
            off.set_option(api.OPT_PREDICT_FACTOR, 0)
            _, t = _timed(off, lambda: call(off))
            assert t["fused"][1] == len(np.unique(set_of)) == 8, t
        finally:
            off.close()
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = _case(105, 2, 2, 2, 4, 5)
    _, t = _timed(handle, lambda: handle.predict_batch_sets(Xs, ys, s2, 2, P, set_of, Xt))
    assert t["fused"][1] == 2 and t["sweep"][1] == 0, t


# ----------------------------------------------------------------------------- 2. position and size
@pytest.mark.parametrize("n,d,K,C,B,m", [KEPT[1], KEPT[4], OTHER[3]], ids=_ids([KEPT[1], KEPT[4], OTHER[3]]))
def test_position_and_size_change_nothing(handle, n, d, K, C, B, m):
    case = _case(n, d, K, C, B, m)
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = case
    base = handle.predict_batch_sets(Xs, ys, s2, K, P, set_of, Xt)
    basek = handle.krige_predict_batch_sets(Xs, ys, K, P, set_of, row_s2, Xt, api.VAR_PLUGIN)
    bases = handle.predict_summary_sets(Xs, ys, s2, K, P, set_of, Xt, PROBS[2], yt)
    rng = np.random.default_rng(n)
    perm = rng.permutation(B)                    # rows permuted (a summary sums in the order of its rows: not compared here)
    _same(handle.predict_batch_sets(Xs, ys, s2, K, P[perm], set_of[perm], Xt), [o[perm] for o in base])
    _same(handle.krige_predict_batch_sets(Xs, ys, K, P[perm], set_of[perm], row_s2[perm], Xt, api.VAR_PLUGIN),
          [o[perm] for o in basek])
    sp = rng.permutation(C)                      # new set j is old set sp[j]
    inv = np.argsort(sp)[set_of]
    _same(handle.predict_batch_sets(Xs[sp], ys[sp], s2[sp], K, P, inv, Xt[sp]), base)
    _same(handle.krige_predict_batch_sets(Xs[sp], ys[sp], K, P, inv, row_s2, Xt[sp], api.VAR_PLUGIN), basek)
    _same_summaries(handle.predict_summary_sets(Xs[sp], ys[sp], s2[sp], K, P, inv, Xt[sp], PROBS[2], yt[sp]),
                    [bases[c] for c in sp])
    # more sets and more rows (on the new set) around the same rows
    Xs2, ys2, s22 = np.concatenate([Xs, Xs[:1] * 0.9]), np.concatenate([ys, ys[:1]]), np.concatenate([s2, [2.0]])
    Xt2, yt2 = np.concatenate([Xt, Xt[:1]]), np.concatenate([yt, yt[:1]])
    P2, set2 = np.concatenate([P[:2], P]), np.concatenate([[C, C], set_of]).astype(np.int32)
    _same([o[2:] for o in handle.predict_batch_sets(Xs2, ys2, s22, K, P2, set2, Xt2)], base)
    _same([o[2:] for o in handle.krige_predict_batch_sets(Xs2, ys2, K, P2, set2, np.concatenate([[1.0, 1.0], row_s2]), Xt2,
                                                          api.VAR_PLUGIN)], basek)
    _same_summaries(handle.predict_summary_sets(Xs2, ys2, s22, K, P2, set2, Xt2, PROBS[2], yt2)[:C], bases)
    # C = 1 is the single-set call; all rows on one set of two
    c = int(set_of[0])
    one = (Xs[c:c + 1], ys[c:c + 1], s2[c:c + 1], P, np.zeros(B, dtype=np.int32), Xt[c:c + 1], yt[c:c + 1], row_s2)
    _check_all(handle, one, K, expect_clean=False)
    two = (Xs[:2], ys[:2], s2[:2], P, np.ones(B, dtype=np.int32), Xt[:2], yt[:2], row_s2)
    _check_all(handle, two, K, expect_clean=False)


# ----------------------------------------------------------------------------- 3. workspace limits
@pytest.mark.parametrize("n,d,K,B,m", [(50, 3, 2, 150, 20), (14, 2, 2, 300, 70)], ids=["n50-chunks-of-64", "n14-several-chunks"])
def test_a_workspace_limit_changes_no_bit(n, d, K, B, m):
    """1 MiB: the kept-factor scratch holds 64 draws at a time, so a set's rows are served in several chunks."""
    case = _case(n, d, K, 3, B, m, seed=2)
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = case
    whole_h, cut_h = api.Handle(0), api.Handle(0)
    try:
        cut_h.set_workspace_limit(1 << 20)
        assert max(np.bincount(set_of)) > 64
        whole = whole_h.predict_batch_sets(Xs, ys, s2, K, P, set_of, Xt)
        _same(cut_h.predict_batch_sets(Xs, ys, s2, K, P, set_of, Xt), whole)
        _same(whole, _ref_predict(whole_h, case, K))
        _same(cut_h.krige_predict_batch_sets(Xs, ys, K, P, set_of, row_s2, Xt, api.VAR_PLUGIN),
              whole_h.krige_predict_batch_sets(Xs, ys, K, P, set_of, row_s2, Xt, api.VAR_PLUGIN))
        ws = whole_h.predict_summary_sets(Xs, ys, s2, K, P, set_of, Xt, PROBS[2], yt)
        _same_summaries(cut_h.predict_summary_sets(Xs, ys, s2, K, P, set_of, Xt, PROBS[2], yt), ws)
        _same_summaries(ws, _ref_summary(whole_h, case, K, PROBS[2], True))
        assert cut_h.workspace_bytes()[0] < whole_h.workspace_bytes()[0]
    finally:
        whole_h.close()
        cut_h.close()


# ----------------------------------------------------------------------------- 4. failure
def test_failing_rows_are_nan_and_left_out_of_their_sets_summary(handle):
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = _case(14, 2, 2, 3, 7, 7)
    P = np.concatenate([P, P[:4]])
    set_of = np.concatenate([set_of, [0, 2, 0, 2]]).astype(np.int32)
    row_s2 = np.concatenate([row_s2, row_s2[:4]])
    bad = [2, 8, 9]                              # singular rows in two of the three sets, beside good ones
    P[bad, 2:] = 1e-4
    case = (Xs, ys, s2, P, set_of, Xt, yt, row_s2)
    want = _ref_predict(handle, case, 2)
    assert sorted(np.flatnonzero(want[3])) == bad and len({int(set_of[b]) for b in bad}) == 2
    _check_all(handle, case, 2, forms=(api.VAR_PLUGIN, api.VAR_UNBIASED), n_probs=(0, 2), at=(True, False), expect_clean=False)
    got = handle.predict_batch_sets(Xs, ys, s2, 2, P, set_of, Xt)
    assert np.all(np.isnan(got[0][bad])) and np.all(np.isnan(got[1][bad])) and np.all(np.isnan(got[2][bad]))
    good = [b for b in range(len(P)) if b not in bad]
    assert np.all(np.isfinite(got[0][good])) and not got[3][good].any()
    # one set whose every row fails: NaN in its block only
    P2 = P.copy()
    P2[set_of == 0, 2:] = 1e-4
    case2 = (Xs, ys, s2, P2, set_of, Xt, yt, row_s2)
    res = handle.predict_summary_sets(Xs, ys, s2, 2, P2, set_of, Xt, PROBS[2], yt)
    _same_summaries(res, _ref_summary(handle, case2, 2, PROBS[2], True))
    assert np.all(np.isnan(res[0]["y_hat"])) and res[0]["n_failed"] == int(np.sum(set_of == 0))
    assert np.all(np.isfinite(res[2]["y_hat"])) and np.all(np.isnan(res[1]["y_hat"]))   # set 1 has no row at all


# ----------------------------------------------------------------------------- 5. refusals
def test_bad_arguments_are_refused_before_anything_is_copied_or_launched():
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = _case(14, 2, 2, 3, 7, 7)
    n, d, K, C, B, m = 14, 2, 2, 3, 7, 7
    a = dict(Xb=np.ascontiguousarray(np.transpose(Xs, (0, 2, 1))), yb=np.ascontiguousarray(ys), s2=np.ascontiguousarray(s2),
             P=np.asfortranarray(P), set=np.ascontiguousarray(set_of), Xtb=np.ascontiguousarray(np.transpose(Xt, (0, 2, 1))),
             rs2=np.ascontiguousarray(row_s2), probs=np.array([0.1, 0.9]), n=n, d=d, K=K, C=C, B=B, m=m, form=api.VAR_PLUGIN,
             n_probs=2)
    mean, var, beta, q = np.full((B, m), 7.0, order="F"), np.full((B, m), 7.0, order="F"), np.full(B, 7.0), np.full(B, 7.0)
    out, st = np.full((C, 6, m), 7.0), np.full(B, 7, dtype=np.int32)
    h = api.Handle(0)
    L, p, ip = api.lib(), api._p, api._ipt

    def predict(**kw):
        v = dict(a, mean=mean, var=var)
        v.update(kw)
        return L.ccgp_predict_batch_sets(h._h, p(v["Xb"]), v["n"], v["d"], p(v["yb"]), p(v["s2"]), v["C"], v["K"], p(v["P"]),
                                         ip(v["set"]), v["B"], p(v["Xtb"]), v["m"], p(v["mean"]), p(v["var"]), p(beta), ip(st))

    def krige(**kw):
        v = dict(a, mean=mean, var=var)
        v.update(kw)
        return L.ccgp_krige_predict_batch_sets(h._h, p(v["Xb"]), v["n"], v["d"], p(v["yb"]), v["C"], v["K"], p(v["P"]),
                                               ip(v["set"]), v["B"], p(v["rs2"]), v["form"], p(v["Xtb"]), v["m"], p(v["mean"]),
                                               p(v["var"]), p(beta), p(q), ip(st))

    def summary(**kw):
        v = dict(a, out=out)
        v.update(kw)
        return L.ccgp_predict_summary_sets(h._h, p(v["Xb"]), v["n"], v["d"], p(v["yb"]), p(v["s2"]), v["C"], v["K"], p(v["P"]),
                                           ip(v["set"]), v["B"], p(v["Xtb"]), v["m"], p(v["probs"]), v["n_probs"], None,
                                           p(v["out"]), p(beta), ip(st))

    try:
        before = h.workspace_bytes()
        high, low = a["set"].copy(), a["set"].copy()
        high[3], low[6] = C, -1
        common = dict(C0=dict(C=0), B0=dict(B=0), m0=dict(m=0), n0=dict(n=0), K0=dict(K=0), set_high=dict(set=high),
                      set_low=dict(set=low), no_Xs=dict(Xb=None), no_ys=dict(yb=None), no_params=dict(P=None),
                      no_set=dict(set=None), no_Xtests=dict(Xtb=None))
        for name, kw in common.items():
            assert predict(**kw) == EINVAL and krige(**kw) == EINVAL and summary(**kw) == EINVAL, name
        for name, kw in dict(no_sigma2=dict(s2=None), no_mean=dict(mean=None), no_var=dict(var=None)).items():
            assert predict(**kw) == EINVAL, name
        neg, inf = a["rs2"].copy(), a["rs2"].copy()
        neg[2], inf[5] = -1.0, np.inf
        for name, kw in dict(form=dict(form=3), no_s2=dict(rs2=None), neg=dict(rs2=neg), inf=dict(rs2=inf), no_mean=dict(mean=None),
                             unbiased_n1=dict(form=api.VAR_UNBIASED, n=1)).items():
            assert krige(**kw) == EINVAL, name
        for name, kw in dict(no_sigma2=dict(s2=None), no_out=dict(out=None), probs_hi=dict(probs=np.array([0.1, 1.0])),
                             probs_lo=dict(probs=np.array([0.0, 0.9])), nine=dict(n_probs=9), neg=dict(n_probs=-1),
                             no_probs=dict(probs=None)).items():
            assert summary(**kw) == EINVAL, name
        assert L.ccgp_predict_batch_sets(None, *([None, 1, 1, None, None, 1, 1, None, None, 1, None, 1] + [None] * 4)) == EINVAL
        assert np.all(mean == 7.0) and np.all(var == 7.0) and np.all(beta == 7.0) and np.all(q == 7.0)
        assert np.all(out == 7.0) and np.all(st == 7) and h.workspace_bytes() == before
        assert predict() == 0 and krige() == 0 and krige(form=api.VAR_UNBIASED, rs2=None) == 0 and summary() == 0
    finally:
        h.close()


# ----------------------------------------------------------------------------- 6. history
@pytest.mark.parametrize("n,d,K,C,B,m", [KEPT[1], OTHER[3]], ids=_ids([KEPT[1], OTHER[3]]))
def test_the_bits_do_not_depend_on_what_the_handle_ran_before(n, d, K, C, B, m):
    Xs, ys, s2, P, set_of, Xt, yt, row_s2 = _case(n, d, K, C, B, m)
    P = P.copy()
    P[B - 1, K:] = 1e-4 if n < 100 else P[B - 1, K:]      # a failed row among them where theta = 1e-4 is singular

    def run(h):
        return (h.predict_batch_sets(Xs, ys, s2, K, P, set_of, Xt),
                h.krige_predict_batch_sets(Xs, ys, K, P, set_of, row_s2, Xt, api.VAR_PLUGIN),
                h.predict_summary_sets(Xs, ys, s2, K, P, set_of, Xt, PROBS[2], yt))

    def same(got, want):
        _same(got[0], want[0])
        _same(got[1], want[1])
        _same_summaries(got[2], want[2])

    alone = api.Handle(0)
    try:
        want = run(alone)
    finally:
        alone.close()
    h = api.Handle(0)
    try:
        for fill in (0x00, 0x3F, 0xFF):
            assert h.debug_fill_scratch(fill) == 0
            same(run(h), want)
        big = _case(104, 2, 2, 2, 4, 5)
        h.predict_batch(big[0][0], big[1][0], 2, big[3], big[5][0], 1.0)
        h.loglik_batch(big[0][1], big[1][1], 2, big[3], 1.0)
        h.predict_summary(Xs[0], ys[0], K, P[:2], Xt[0], 1.0, PROBS[8])
        same(run(h), want)
    finally:
        h.close()


# ----------------------------------------------------------------------------- 7. surface
def _gv_problem(handle, count, m_of):
    """`count` Ground-Vibrations size-50 sets with fitted comparators and a few draws each; set i keeps m_of[i] test sites."""
    from ccgp_amd import cgp, fit
    gv = [load_gv(50, i + 1) for i in range(count)]
    sets = [(g[0], g[1], g[2][:m_of[i]], g[3][:m_of[i]]) for i, g in enumerate(gv)]
    rng = np.random.default_rng(11)
    draws = [np.column_stack([rng.uniform(0.2, 0.8, 12), rng.uniform(0.03, 0.15, 12), rng.uniform(0.8, 3.0, 12)]) for _ in sets]
    krige = fit.ordinary_kriging_fit_sets(handle, [s[0] for s in sets], [s[1] for s in sets], starts=3)
    cgps = cgp.CGP_sets(handle, [s[0] for s in sets], [s[1] for s in sets], num_starts=2, on_device=True)
    return sets, draws, krige, cgps


@pytest.mark.parametrize("m_of", [(150, 150, 150), (150, 40)], ids=["three-sets", "two-sets-of-different-m"])
def test_compare_GP_sets_equals_compare_GP_per_set(handle, m_of):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    sets, draws, krige, cgps = _gv_problem(handle, len(m_of), m_of)
    gp = CombinedGP("GV", handle=handle)
    s2 = [k["sigma2"] for k in krige]
    cg, sg = [dict(est=e) for e in cgps], [dict(est=e) for e in krige]
    counts = {}
    got = fit.compare_GP_sets(gp, [s[2] for s in sets], 0.05, [s[3] for s in sets], draws, [s[0] for s in sets], s2,
                              [s[1] for s in sets], cgp=cg, single=sg, counts=counts)
    assert counts["calls"] == 3 * len(set(m_of))
    for i, s in enumerate(sets):
        want = fit.compare_GP(gp, s[2], 0.05, s[3], draws[i], s[0], s2[i], s[1], exact=True, cgp=cg[i], single=sg[i])
        assert list(got[i]) == list(want) and len(want) == 13   # 5 Combined-GP keys, 4 per comparator
        for k, v in want.items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(got[i][k], v, err_msg=k)
            else:
                assert got[i][k] is v
    # prediction_sets against prediction, with the held-out responses
    pred = gp.prediction_sets([s[2][:40] for s in sets], 0.1, draws, [s[0] for s in sets], s2, [s[1] for s in sets],
                              [s[3][:40] for s in sets])
    for i, s in enumerate(sets):
        w = gp.prediction(s[2][:40], 0.1, draws[i], s[0], s2[i], s[1], s[3][:40])
        assert sorted(pred[i]) == sorted(w)
        for k in w:
            np.testing.assert_array_equal(pred[i][k], w[k], err_msg=k)


def test_study_with_the_prediction_in_lockstep_writes_the_same_files(handle, tmp_path):
    import os
    from conftest import synthetic_design
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    sets = []
    for c in range(3):
        X, y = synthetic_design(12, 2, 40 + c)
        Xt, yt = synthetic_design(6, 2, 70 + c)
        sets.append((X, y * (1.0 + 0.2 * c) + 0.3 * c * X[:, 0], Xt, yt * (1.0 + 0.2 * c) + 0.3 * c * Xt[:, 0]))
    gp = CombinedGP("GV", handle=handle)
    arms = {}
    for on in (False, True):
        arms[on] = fit.study(gp, sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], cgp=dict(num_starts=2, rng=5),
                             single=True, lockstep_predict=on, out_dir=str(tmp_path / str(on)))
    for i in range(3):
        for k, v in arms[False]["tables"][i].items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(arms[True]["tables"][i][k], v, err_msg=k)
        assert arms[True]["summaries"][i] == arms[False]["summaries"][i]
        with open(os.path.join(tmp_path, "True", "results_%d.txt" % (i + 1)), "rb") as a, \
                open(os.path.join(tmp_path, "False", "results_%d.txt" % (i + 1)), "rb") as b:
            assert a.read() == b.read()
    assert arms[True]["calls"]["predict"] == 3 < arms[False]["calls"]["predict"] == 9
