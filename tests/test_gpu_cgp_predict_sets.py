"""The CGP comparator's prediction over many training sets of one shape: ccgp_cgp_predict_sets and cgp.predict_CGP_sets.

The contract is one of BITS: block b of `out` and of the kept state has exactly the bits ccgp_cgp_predict returns for that
row on set set[b] alone with that set's test sites, whatever C, B, the row's position, the order of `set`, where the
workspace limit cuts the call or what the handle ran before.  Every comparison below is np.testing.assert_array_equal on
float64 (NaN == NaN), never a tolerance; the reference is the single-set entry point on the same handle.

Shapes (n, d, C, B, m): the smallest design with fewer sites than one workgroup's four waves; the Ground-Vibrations
size-50 sets with their own 150 test sites each; the largest order, where lane l owns points l and l + 64.  `set` is drawn
as tests/test_gpu_sets.py draws it: unsorted, uneven counts, one set without rows when C >= 3.  Rows come from
test_gpu_cgp.rows_in_the_box (lambda alternating between its bounds)."""
import numpy as np
import pytest

from conftest import load_gv, synthetic_design
from test_gpu_cgp import rows_in_the_box
from ccgp_amd import api, cgp

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4
KEEP_KEYS = ("s", "res2", "temp", "sf", "beta", "tau2")
SHAPES = [(6, 2, 2, 5, 3), (50, 4, 3, 6, 150), (128, 2, 2, 4, 5)]
IDS = ["n%d-d%d-C%d-B%d-m%d" % s for s in SHAPES]
_CASES = {}


def _case(n, d, C, B, m):
    """C standardised designs with responses and m test sites each, B rows in CGP's box for their own set, a set per row.
    Built once per shape and shared; nothing changes it."""
    key = (n, d, C, B, m)
    if key not in _CASES:
        rng = np.random.default_rng(1000 + n)
        if n == 50:   # the first d inputs of the Ground-Vibrations size-50 sets, each with its own test sites
            gv = [load_gv(50, c + 1) for c in range(C)]
            lo = [g[0][:, :d].min(axis=0) for g in gv]
            sc = [g[0][:, :d].max(axis=0) - l for g, l in zip(gv, lo)]
            Xs = np.stack([(g[0][:, :d] - l) / s for g, l, s in zip(gv, lo, sc)])
            ys = np.stack([g[1] for g in gv])
            Xt = np.stack([(g[2][:m, :d] - l) / s for g, l, s in zip(gv, lo, sc)])
        else:
            pairs = [synthetic_design(n, d, 7 * n + 10 * c) for c in range(C)]
            Xs = np.stack([cgp.standardise(p[0])[0] for p in pairs])
            ys = np.stack([p[1] * (1.0 + 0.1 * c) for c, p in enumerate(pairs)])
            Xt = rng.random((C, m, d))
        used = [c for c in range(C) if not (C >= 3 and c == 1)]
        weights = np.arange(1, len(used) + 1, dtype=float) ** 2
        set_of = rng.choice(used, size=B, p=weights / weights.sum())
        lead = used[::-1][:B]
        set_of[:len(lead)] = lead
        set_of = set_of.astype(np.int32)
        P = np.stack([rows_in_the_box(Xs[c], B, 31 * n + b)[b] for b, c in enumerate(set_of)])
        for a in (Xs, ys, Xt, set_of, P):
            a.setflags(write=False)
        _CASES[key] = (Xs, ys, Xt, P, set_of)
    return _CASES[key]


def _per_row(handle, Xs, ys, Xt, P, set_of):
    """The reference: every row through ccgp_cgp_predict on its set alone."""
    B, m = len(P), Xt.shape[1]
    out, keeps, st = np.empty((B, m, 6)), [], np.zeros(B, dtype=np.int32)
    for b, c in enumerate(set_of):
        o, k, s = handle.cgp_predict(Xs[c], ys[c], P[b], Xt[c])
        out[b], st[b] = o, s
        keeps.append(k)
    return out, keeps, st


def _same_keeps(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            for k in KEEP_KEYS:
                np.testing.assert_array_equal(g[k], w[k], err_msg=k)


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[2])
    _same_keeps(got[1], want[1])


# ----------------------------------------------------------------------------- 1. bits against the single-set call
@pytest.mark.parametrize("n,d,C,B,m", SHAPES, ids=IDS)
def test_rows_have_the_bits_of_the_single_set_call(handle, n, d, C, B, m):
    Xs, ys, Xt, P, set_of = _case(n, d, C, B, m)
    want = _per_row(handle, Xs, ys, Xt, P, set_of)
    assert not want[2].any() and np.all(np.isfinite(want[0]))
    _same(handle.cgp_predict_sets(Xs, ys, P, set_of, Xt), want)
    # the states alone
    got = handle.cgp_predict_sets(Xs, ys, P, set_of, Xt[:, :0])
    assert got[0].shape == (B, 0, 6)
    np.testing.assert_array_equal(got[2], want[2])
    _same_keeps(got[1], want[1])
    # C = 1 is the single-set call; all rows on one set of two
    one = handle.cgp_predict_sets(Xs[1:2], ys[1:2], P[:2], [0, 0], Xt[1:2])
    _same(one, _per_row(handle, Xs[1:2], ys[1:2], Xt[1:2], P[:2], [0, 0]))
    only = np.ones(B, dtype=np.int32)
    _same(handle.cgp_predict_sets(Xs[:2], ys[:2], P, only, Xt[:2]), _per_row(handle, Xs, ys, Xt, P, only))


# ----------------------------------------------------------------------------- 2. position
@pytest.mark.parametrize("n,d,C,B,m", SHAPES[:2], ids=IDS[:2])
def test_permuting_rows_or_sets_permutes_the_outputs_and_nothing_else(handle, n, d, C, B, m):
    Xs, ys, Xt, P, set_of = _case(n, d, C, B, m)
    base = handle.cgp_predict_sets(Xs, ys, P, set_of, Xt)
    rng = np.random.default_rng(n)
    perm = rng.permutation(B)
    got = handle.cgp_predict_sets(Xs, ys, P[perm], set_of[perm], Xt)
    _same(got, (base[0][perm], [base[1][i] for i in perm], base[2][perm]))
    sp = rng.permutation(C)                      # new set j is old set sp[j]
    _same(handle.cgp_predict_sets(Xs[sp], ys[sp], P, np.argsort(sp)[set_of], Xt[sp]), base)
    # more sets and more rows around the same rows change nothing either
    Xs2, ys2, Xt2 = np.concatenate([Xs, Xs[:1] * 0.9]), np.concatenate([ys, ys[:1]]), np.concatenate([Xt, Xt[:1]])
    P2, set2 = np.concatenate([P[:3], P]), np.concatenate([[C, 0, C], set_of]).astype(np.int32)
    got = handle.cgp_predict_sets(Xs2, ys2, P2, set2, Xt2)
    _same((got[0][3:], got[1][3:], got[2][3:]), base)


# ----------------------------------------------------------------------------- 3. cuts
def test_a_workspace_limit_that_cuts_inside_a_set_changes_no_bit():
    """A row of (50, 4, m = 150) takes n^2 + 7 n + 6 m + 2 d + 16 = 3774 doubles and two words, 30 200 bytes: 1 MiB, the
    smallest limit, holds 34 of the 40 rows.  Every set with rows has some on either side of that cut, and the second chunk
    goes up without the sets."""
    Xs, ys, Xt, P, set_of = _case(50, 4, 3, 6, 150)
    P40 = np.concatenate([P * (1.0 + 0.001 * r) for r in range(7)])[:40]
    set40 = np.concatenate([set_of] * 7)[:40]
    whole_h, cut_h = api.Handle(0), api.Handle(0)
    try:
        whole = whole_h.cgp_predict_sets(Xs, ys, P40, set40, Xt)
        cut_h.set_workspace_limit(1 << 20)
        cut = cut_h.cgp_predict_sets(Xs, ys, P40, set40, Xt)
        assert whole_h.workspace_bytes()[0] >= 40 * 30200 and cut_h.workspace_bytes()[0] < 36 * 30200
    finally:
        whole_h.close()
        cut_h.close()
    assert not whole[2].any()
    _same(cut, whole)
    assert set(set40[:34]) == set(set40[34:]) == {0, 2}


# ----------------------------------------------------------------------------- 4. failure
def test_a_failing_row_is_nan_with_its_status_and_its_neighbours_are_untouched(handle):
    """lambda = 0 with every entry of G exactly 1 (tests/test_gpu_cgp.py): the second pivot is exactly 0."""
    Xs, ys, Xt, P, set_of = _case(6, 2, 2, 5, 3)
    bad = np.array([0.0, 1e-17, 1e-17, 9.0, 8.0, 0.5])
    rows = np.stack([P[0], bad, P[2], bad, P[4]])
    sets = np.array([1, 0, 0, 1, 1], dtype=np.int32)
    want = _per_row(handle, Xs, ys, Xt, rows, sets)
    assert want[2].tolist() == [0, 2, 0, 2, 0]
    got = handle.cgp_predict_sets(Xs, ys, rows, sets, Xt)
    _same(got, want)
    for b in (1, 3):
        assert np.all(np.isnan(got[0][b])) and got[1][b] is None
    for b in (0, 2, 4):
        assert np.all(np.isfinite(got[0][b]))
    # the raw call: the failed rows' state blocks are NaN, the return value counts them
    n, d, m = 6, 2, 3
    Xb = np.ascontiguousarray(np.transpose(Xs, (0, 2, 1)))
    Xtb = np.ascontiguousarray(np.transpose(Xt, (0, 2, 1)))
    rf = np.asfortranarray(rows)
    out, state, st = np.empty((5, 6, m)), np.empty((5, 3 * n + 3)), np.zeros(5, dtype=np.int32)
    rc = api.lib().ccgp_cgp_predict_sets(handle._h, api._p(Xb), n, d, api._p(np.ascontiguousarray(ys)), 2, api._p(rf),
                                         api._ipt(sets), 5, api._p(Xtb), m, api._p(out), api._p(state), api._ipt(st))
    assert rc == 2 and st.tolist() == [0, 2, 0, 2, 0]
    assert np.all(np.isnan(state[[1, 3]])) and np.all(np.isfinite(state[[0, 2, 4]]))
    # every row failing
    got = handle.cgp_predict_sets(Xs, ys, np.stack([bad, bad]), [0, 1], Xt)
    assert got[2].tolist() == [2, 2] and np.all(np.isnan(got[0])) and got[1] == [None, None]


# ----------------------------------------------------------------------------- 5. refusals
def test_bad_arguments_are_refused_before_anything_is_copied_or_launched():
    Xs, ys, Xt, P, set_of = _case(6, 2, 2, 5, 3)
    n, d, C, B, m = 6, 2, 2, 5, 3
    Xb = np.ascontiguousarray(np.transpose(Xs, (0, 2, 1)))
    Xtb = np.ascontiguousarray(np.transpose(Xt, (0, 2, 1)))
    yb, rf, sets = np.ascontiguousarray(ys), np.asfortranarray(P), np.ascontiguousarray(set_of)
    h = api.Handle(0)
    try:
        before = h.workspace_bytes()
        out, state, st = np.full((B, 6, m), 7.0), np.full((B, 3 * n + 3), 7.0), np.full(B, 7, dtype=np.int32)

        def call(Xb=Xb, n=n, d=d, yb=yb, C=C, rf=rf, sets=sets, B=B, Xtb=Xtb, m=m, out=out):
            return api.lib().ccgp_cgp_predict_sets(h._h, api._p(Xb), n, d, api._p(yb), C, api._p(rf), api._ipt(sets), B,
                                                   api._p(Xtb), m, api._p(out), api._p(state), api._ipt(st))

        high, low = sets.copy(), sets.copy()
        high[2], low[4] = C, -1
        refusals = dict(C0=dict(C=0), Bneg=dict(B=-1), mneg=dict(m=-1), n0=dict(n=0), d0=dict(d=0), set_high=dict(sets=high),
                        set_low=dict(sets=low), no_Xs=dict(Xb=None), no_ys=dict(yb=None), no_params=dict(rf=None),
                        no_set=dict(sets=None), no_Xtests=dict(Xtb=None), no_out=dict(out=None))
        for name, kw in refusals.items():
            assert call(**kw) == EINVAL, name
        assert api.lib().ccgp_cgp_predict_sets(None, None, 1, 1, None, 1, None, None, 1, None, 1, None, None, None) == EINVAL
        # d too large for the carve, n beyond the kernel: refused as ccgp_cgp_predict refuses them
        X22, y22 = synthetic_design(128, 22, 1)
        with pytest.raises(api.CcgpError) as e:
            h.cgp_predict_sets(X22[None], y22[None], np.ones((1, 46)), [0], X22[None, :2])
        assert e.value.code == EUNSUPPORTED
        X129, y129 = synthetic_design(129, 2, 1)
        with pytest.raises(api.CcgpError) as e:
            h.cgp_predict_sets(X129[None], y129[None], np.ones((1, 6)), [0], X129[None, :2])
        assert e.value.code == EUNSUPPORTED
        assert np.all(out == 7.0) and np.all(state == 7.0) and np.all(st == 7)
        assert h.workspace_bytes() == before       # nothing was allocated, so nothing was launched
        assert call(B=0) == 0 and np.all(out == 7.0) and h.workspace_bytes() == before
        # the wrapper's own shape checks
        for bad in (lambda: h.cgp_predict_sets(Xs, ys, P, set_of, Xt[:1]), lambda: h.cgp_predict_sets(Xs, ys, P, set_of, Xt[0]),
                    lambda: h.cgp_predict_sets(Xs, ys, P[:, :5], set_of, Xt),
                    lambda: h.cgp_predict_sets(Xs, ys, P, set_of[:2], Xt)):
            with pytest.raises(ValueError):
                bad()
        # and the largest supported design goes through
        X21, y21 = synthetic_design(128, 21, 1)
        row = np.concatenate([[0.01], np.full(21, 0.3), np.full(21, 4.0), [0.5]])
        got = h.cgp_predict_sets(X21[None], y21[None], row[None], [0], X21[None, :3])
        want = h.cgp_predict(X21, y21, row, X21[:3])
        assert got[2][0] == 0 == want[2]
        np.testing.assert_array_equal(got[0][0], want[0])
    finally:
        h.close()


# ----------------------------------------------------------------------------- 6. history
@pytest.mark.parametrize("n,d,C,B,m", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_the_bits_do_not_depend_on_what_the_handle_ran_before(n, d, C, B, m):
    Xs, ys, Xt, P, set_of = _case(n, d, C, B, m)
    bad = np.array([0.0, 1e-17, 1e-17, 9.0, 8.0, 0.5])
    rows = np.concatenate([P, bad[None]])      # a failed row keeps nothing: its blocks must not show the fill
    sets = np.concatenate([set_of, [0]]).astype(np.int32)
    alone = api.Handle(0)
    try:
        want = alone.cgp_predict_sets(Xs, ys, rows, sets, Xt)
    finally:
        alone.close()
    h = api.Handle(0)
    try:
        for fill in (0x00, 0x3F, 0xFF):
            assert h.debug_fill_scratch(fill) == 0
            _same(h.cgp_predict_sets(Xs, ys, rows, sets, Xt), want)
        # after other calls on the handle, larger and smaller
        big = synthetic_design(100, 3, 3)
        h.cgp_state_batch(cgp.standardise(big[0])[0], big[1], rows_in_the_box(cgp.standardise(big[0])[0], 9, 1))
        h.loglik_batch(big[0], big[1], 1, np.array([[1.0, 2.0, 3.0, 4.0]]), 1.0)
        h.cgp_predict(Xs[0], ys[0], P[0], Xt[0])
        _same(h.cgp_predict_sets(Xs, ys, rows, sets, Xt), want)
    finally:
        h.close()


# ----------------------------------------------------------------------------- 7. route
def test_a_call_is_one_set_of_launches(handle):
    """One timed section -- the state launch of all rows and the site launch behind it -- and nothing on the blocked sweep."""
    from test_gpu_gradient_exact import _timed
    Xs, ys, Xt, P, set_of = _case(50, 4, 3, 6, 150)
    got, t = _timed(handle, lambda: handle.cgp_predict_sets(Xs, ys, P, set_of, Xt))
    assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t
    _same(got, _per_row(handle, Xs, ys, Xt, P, set_of))


# ----------------------------------------------------------------------------- 8. surface
def test_predict_CGP_sets_equals_predict_CGP(handle):
    Xs, ys, Xt, P, set_of = _case(50, 4, 3, 6, 150)
    ests = [dict(X=Xs[c], yobs=ys[c], **{"lambda": P[b, 0]}, theta=P[b, 1:5], alpha=P[b, 5:9], bandwidth=P[b, 9])
            for b, c in enumerate(set_of)]
    news = [Xt[c] for c in set_of]
    for PI in (False, True):
        got = cgp.predict_CGP_sets(handle, ests, news, PI=PI)
        assert len(got) == len(ests)
        for g, e, u in zip(got, ests, news):
            w = cgp.predict_CGP(handle, e, u, PI=PI)
            assert sorted(g) == sorted(w)
            for k in w:
                if w[k] is None:
                    assert g[k] is None
                else:
                    np.testing.assert_array_equal(g[k], w[k], err_msg=k)
    # ragged: other test sets and another design shape in one list; the results keep the models' order
    X6, y6, Xt6, P6, set6 = _case(6, 2, 2, 5, 3)
    e6 = dict(X=X6[0], yobs=y6[0], **{"lambda": P6[1, 0]}, theta=P6[1, 1:3], alpha=P6[1, 3:5], bandwidth=P6[1, 5])
    mixed_e, mixed_u = [ests[0], e6, ests[1], ests[2]], [news[0][:7], Xt6[0], news[1], news[2][:7]]
    got = cgp.predict_CGP_sets(handle, mixed_e, mixed_u, PI=True)
    for g, e, u in zip(got, mixed_e, mixed_u):
        w = cgp.predict_CGP(handle, e, u, PI=True)
        for k in w:
            np.testing.assert_array_equal(g[k], w[k], err_msg=k)
    bad = dict(ests[0], **{"lambda": 0.0}, theta=np.full(4, 1e-17))
    with pytest.raises(RuntimeError):
        cgp.predict_CGP_sets(handle, [ests[0], bad], news[:2])
