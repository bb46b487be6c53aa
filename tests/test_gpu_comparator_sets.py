"""The comparator fits over many training sets of one shape: ccgp_profile_batch_sets / ccgp_cgp_state_batch_sets and the
lockstep fits on top of them (fit.ordinary_kriging_fit_sets, cgp.CGP_sets, fit.study(lockstep_fits=True)).

The contract is one of BITS, as for ccgp_loglik_batch_sets (tests/test_gpu_sets.py): row b has exactly the bits the single-set
call returns for it on set set[b] alone, whatever C, B, the row's position, the order of `set`, where the workspace limit
cuts the call, or what the handle ran before.  Every comparison of outputs below is np.testing.assert_array_equal on float64
(NaN == NaN), never a tolerance; the reference is the single-set entry point on the same handle.

Shapes of the profiled gradient (n, d, K, C, B): the smallest design (NB = 1), an odd one, the first order with padding rows
(17 = 16 + 1), the Ground-Vibrations size-50 sets at eight starts x nine sets, n = 64, the first order above the 8 x 8 grid and
the largest order.  Singular rows: every theta = 1e-4 at d <= 3, which tests/test_gpu_loo.py establishes as singular under the
pivot rule.  CGP (n, d, C, B): the smallest design the jackknife can hold a row out of with room to spare, the
Ground-Vibrations order at d = 4 and the largest order; a failing evaluation is tests/test_gpu_cgp.py's (lambda = 0 and G = 1)."""
import numpy as np
import pytest

from conftest import load_gv, synthetic_design
from test_gpu_cgp import rows_in_the_box
from test_gpu_gradient_exact import _timed
from test_gpu_random_shapes import draws

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -4


# ----------------------------------------------------------------------------- cases
def _set_of(rng, C, B):
    """A set index per row: unsorted, uneven counts, and (C >= 3) set 1 with no rows -- as tests/test_gpu_sets.py draws it."""
    used = [c for c in range(C) if not (C >= 3 and c == 1)]
    weights = np.arange(1, len(used) + 1, dtype=float) ** 2
    set_of = rng.choice(used, size=B, p=weights / weights.sum())
    lead = used[::-1][:B]
    set_of[:len(lead)] = lead
    return set_of.astype(np.int32)


def _designs(n, d, C, seed):
    if (n, d) == (50, 9):
        gv = [load_gv(50, i + 1) for i in range(C)]
        return np.stack([g[0] for g in gv]), np.stack([g[1] for g in gv])
    pairs = [synthetic_design(n, d, seed + 10 * c) for c in range(C)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] * (1.0 + 0.1 * c) + 0.2 * c * p[0][:, 0] for c, p in enumerate(pairs)])


def _profile_case(n, d, K, C, B, seed):
    rng = np.random.default_rng(seed)
    Xs, ys = _designs(n, d, C, seed)
    if (n, d) == (50, 9):   # the single GP's anisotropic scales on these inputs, from smooth to rough
        P = np.concatenate([np.ones((B, 1)), np.exp(rng.uniform(np.log(0.03), np.log(3.0), (B, d)))], axis=1)
        assert K == 1
    else:
        P = draws(rng, n, d, K, B)
    return Xs, ys, P, _set_of(rng, C, B)


def _profile_per_set(handle, Xs, ys, K, P, set_of, grad):
    """The reference: the rows of every set through ccgp_profile_batch."""
    B = len(P)
    ll, s2, beta, st = np.full(B, np.nan), np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    g = np.full(P.shape, np.nan) if grad else None
    for c in np.unique(set_of):
        rows = np.flatnonzero(set_of == c)
        r = handle.profile_batch(Xs[c], ys[c], K, P[rows], grad=grad)
        ll[rows], s2[rows], beta[rows], st[rows] = r[0], r[1], r[2], r[4]
        if grad:
            g[rows] = r[3]
    return ll, s2, beta, g, st


def _cgp_case(n, d, C, B, seed):
    """Rows inside each row's own set's box, skip mixing -1 with held-out rows, row 0 and row n - 1 among them."""
    from ccgp_amd import cgp
    rng = np.random.default_rng(seed)
    Xs, ys = _designs(n, d, C, seed)
    Xs = np.stack([cgp.standardise(X)[0] for X in Xs])
    set_of = _set_of(rng, C, B)
    P = np.stack([rows_in_the_box(Xs[c], 2, seed + 7 * b)[b % 2] for b, c in enumerate(set_of)])
    skip = np.full(B, -1, dtype=np.int32)
    skip[1::2] = rng.integers(0, n, size=len(skip[1::2]))
    skip[1], skip[3] = 0, n - 1
    return Xs, ys, P, set_of, skip


def _cgp_per_set(handle, Xs, ys, P, set_of, skip):
    B = len(P)
    out = [np.full(B, np.nan) for _ in range(4)] + [np.zeros(B, dtype=np.int32)]
    for c in np.unique(set_of):
        rows = np.flatnonzero(set_of == c)
        r = handle.cgp_state_batch(Xs[c], ys[c], P[rows], skip=None if skip is None else skip[rows])
        for k in range(5):
            if r[k] is not None:
                out[k][rows] = r[k]
    if skip is None:
        out[3] = None
    return tuple(out)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            np.testing.assert_array_equal(g, w)


# one shape at least per instance of the gradient kernel, NB = (n + 15) / 16 = 1 .. 8: n = 40, 70 and 90 are NB = 3, 5 and 6
PROFILE_SHAPES = [(5, 1, 1, 2, 3), (14, 2, 2, 3, 7), (17, 2, 1, 3, 6), (40, 3, 1, 2, 5), (50, 9, 1, 9, 72), (64, 4, 2, 2, 5),
                  (70, 2, 2, 3, 6), (90, 4, 1, 2, 5), (105, 2, 2, 2, 5), (128, 3, 3, 2, 4)]
CGP_SHAPES = [(6, 2, 2, 5), (50, 4, 3, 40), (128, 2, 2, 4)]


# ----------------------------------------------------------------------------- 1. profile gradient bits
@pytest.mark.parametrize("n,d,K,C,B", PROFILE_SHAPES, ids=["n%d-d%d-K%d-C%d-B%d" % s for s in PROFILE_SHAPES])
def test_profile_rows_have_the_bits_of_the_single_set_call(handle, n, d, K, C, B):
    Xs, ys, P, set_of = _profile_case(n, d, K, C, B, 100 + n)
    want = _profile_per_set(handle, Xs, ys, K, P, set_of, True)
    assert not want[4].any() and np.isfinite(want[3]).all()
    _same(handle.profile_batch_sets(Xs, ys, K, P, set_of, grad=True), want)
    _same(handle.profile_batch_sets(Xs, ys, K, P, set_of, grad=False), _profile_per_set(handle, Xs, ys, K, P, set_of, False))
    if C == 2:   # a set with no rows: everything on set 1
        only = np.ones(B, dtype=np.int32)
        _same(handle.profile_batch_sets(Xs, ys, K, P, only), _profile_per_set(handle, Xs, ys, K, P, only, True))


# ----------------------------------------------------------------------------- 2. position
@pytest.mark.parametrize("n,d,K,C,B", [(14, 2, 2, 3, 7), (50, 9, 1, 9, 72)])
def test_permuting_rows_or_sets_permutes_the_outputs_and_nothing_else(handle, n, d, K, C, B):
    Xs, ys, P, set_of = _profile_case(n, d, K, C, B, 200 + n)
    base = handle.profile_batch_sets(Xs, ys, K, P, set_of)
    rng = np.random.default_rng(n)
    perm = rng.permutation(B)
    _same(handle.profile_batch_sets(Xs, ys, K, P[perm], set_of[perm]), [o[perm] for o in base])
    sp = rng.permutation(C)                      # new set j is old set sp[j]
    inv = np.argsort(sp)
    _same(handle.profile_batch_sets(Xs[sp], ys[sp], K, P, inv[set_of]), base)
    # more sets and more rows around the same rows change nothing either
    Xs2, ys2 = np.concatenate([Xs, Xs[:1] * 0.9]), np.concatenate([ys, ys[:1]])
    P2, set2 = np.concatenate([P[:3], P]), np.concatenate([[C, 0, C], set_of]).astype(np.int32)
    _same([o[3:] for o in handle.profile_batch_sets(Xs2, ys2, K, P2, set2)], base)
    # the same for the CGP call
    Xc, yc, Pc, setc, skip = _cgp_case(10, 2, 3, 9, 210 + n)
    basec = handle.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip)
    perm = rng.permutation(9)
    _same(handle.cgp_state_batch_sets(Xc, yc, Pc[perm], setc[perm], skip=skip[perm]), [o[perm] for o in basec])
    sp = rng.permutation(3)
    _same(handle.cgp_state_batch_sets(Xc[sp], yc[sp], Pc, np.argsort(sp)[setc], skip=skip), basec)
    Xc2, yc2 = np.concatenate([Xc, Xc[:1]]), np.concatenate([yc, yc[:1] + 1.0])
    got = handle.cgp_state_batch_sets(Xc2, yc2, np.concatenate([Pc[:2], Pc]), np.concatenate([[3, 3], setc]).astype(np.int32),
                                      skip=np.concatenate([[-1, 2], skip]).astype(np.int32))
    _same([o[2:] for o in got], basec)


# ----------------------------------------------------------------------------- 3. route
def test_the_gradient_form_is_one_launch(handle):
    Xs, ys, P, set_of = _profile_case(50, 9, 1, 9, 72, 300)
    got, t = _timed(handle, lambda: handle.profile_batch_sets(Xs, ys, 1, P, set_of))
    assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t
    _same(got, _profile_per_set(handle, Xs, ys, 1, P, set_of, True))
    # the value-only form goes set by set (eight sets have rows), each group one launch of the likelihood instance
    got, t = _timed(handle, lambda: handle.profile_batch_sets(Xs, ys, 1, P, set_of, grad=False))
    assert t["fused"][1] == len(np.unique(set_of)) and t["diag"][1] == 0, t
    # the CGP call: one launch
    Xc, yc, Pc, setc, skip = _cgp_case(50, 4, 3, 40, 303)
    got, t = _timed(handle, lambda: handle.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip))
    assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["sweep"][1] == 0, t


def test_beyond_the_instance_the_rows_go_through_the_sweep_set_by_set(handle):
    from ccgp_amd import api
    Xs, ys, P, set_of = _profile_case(129, 3, 2, 2, 3, 301)
    got, t = _timed(handle, lambda: handle.profile_batch_sets(Xs, ys, 2, P, set_of))
    assert t["fused"][1] == 0 and t["diag"][1] > 0 and t["update"][1] > 0, t
    want = _profile_per_set(handle, Xs, ys, 2, P, set_of, True)
    assert not want[4].any()
    _same(got, want)
    # the Matern family exists on the sweep only, value-only
    rng = np.random.default_rng(302)
    Xm = np.stack([np.sort(rng.random(8))[:, None] for _ in range(3)])
    ym = np.sin(6.0 * Xm[:, :, 0]) + 0.1 * np.arange(3)[:, None]
    Pm = np.stack([[0.6, 0.4, 2.0 + b, 9.0 + b] for b in range(5)])
    setm = np.array([2, 0, 2, 1, 0], dtype=np.int32)
    handle.set_kernel(api.KERNEL_MATERN, 2.5)
    try:
        gotm, tm = _timed(handle, lambda: handle.profile_batch_sets(Xm, ym, 2, Pm, setm, grad=False))
        wantm = _profile_per_set(handle, Xm, ym, 2, Pm, setm, False)
        with pytest.raises(api.CcgpError) as e:      # the gradient is the Gaussian family's, as in the single-set call
            handle.profile_batch_sets(Xm, ym, 2, Pm, setm, grad=True)
    finally:
        handle.set_kernel(api.KERNEL_GAUSS)
    assert e.value.code == EUNSUPPORTED
    assert tm["fused"][1] == 0 and tm["diag"][1] > 0, tm
    assert not wantm[4].any()
    _same(gotm, wantm)


# ----------------------------------------------------------------------------- 4. failure isolation, 7. arguments
def _raw_profile(handle, Xs, ys, K, P, set_of, C=None, B=None, null=(), grad=True):
    """ccgp_profile_batch_sets itself, outputs pre-filled with sentinels -> (return value, loglik, sigma2, beta, grad, status)."""
    from ccgp_amd import api
    Xb, yb, _, idx, C0, n, d = api.Handle._sets(Xs, ys, np.zeros(len(Xs)), set_of, len(set_of))
    Pf = np.asfortranarray(P)
    nB = len(P)
    ll, s2, beta = np.full(nB, 7.5), np.full(nB, 7.5), np.full(nB, 7.5)
    g = np.full(P.shape, 7.5, order="F")
    st = np.full(nB, 77, dtype=np.int32)
    args = dict(Xs=api._p(Xb), ys=api._p(yb), params=api._p(Pf), set=api._ipt(idx), loglik=api._p(ll), sigma2=api._p(s2))
    for name in null:
        args[name] = None
    rc = api.lib().ccgp_profile_batch_sets(handle._h, args["Xs"], n, d, args["ys"], C0 if C is None else C, K, args["params"],
                                           args["set"], nB if B is None else B, args["loglik"], args["sigma2"], api._p(beta),
                                           api._p(g) if grad else None, api._ipt(st))
    return rc, ll, s2, beta, g, st


def _raw_cgp(handle, Xs, ys, P, set_of, skip, C=None, B=None, null=()):
    from ccgp_amd import api
    Xb, yb, _, idx, C0, n, d = api.Handle._sets(Xs, ys, np.zeros(len(Xs)), set_of, len(set_of))
    Pf = np.asfortranarray(P)
    nB = len(P)
    out = [np.full(nB, 7.5) for _ in range(4)]
    st = np.full(nB, 77, dtype=np.int32)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
    args = dict(Xs=api._p(Xb), ys=api._p(yb), params=api._p(Pf), set=api._ipt(idx), val=api._p(out[0]))
    for name in null:
        args[name] = None
    rc = api.lib().ccgp_cgp_state_batch_sets(handle._h, args["Xs"], n, d, args["ys"], C0 if C is None else C, args["params"],
                                             args["set"], nB if B is None else B, api._ipt(sk), args["val"], api._p(out[1]),
                                             api._p(out[2]), api._p(out[3]), api._ipt(st))
    return (rc, *out, st)


@pytest.mark.parametrize("n,d,K,C", [(14, 2, 2, 3), (100, 3, 2, 3)])
def test_a_singular_profile_row_fails_alone(handle, n, d, K, C):
    Xs, ys, P, set_of = _profile_case(n, d, K, C, 5, 400 + n)
    clean = handle.profile_batch_sets(Xs, ys, K, P, set_of)
    bad = P.copy()
    bad[2, K:] = 1e-4
    c = set_of[2]
    want = handle.profile_batch(Xs[c], ys[c], K, bad[2:3], grad=True)
    assert want[4][0] != 0
    rc, ll, s2, beta, g, st = _raw_profile(handle, Xs, ys, K, bad, set_of)
    assert rc == 1
    assert st[2] == want[4][0] and np.isnan(ll[2]) and np.isnan(s2[2]) and np.isnan(beta[2]) and np.isnan(g[2]).all()
    keep = np.arange(5) != 2
    assert not st[keep].any()
    for got, ref in zip((ll, s2, beta, g), clean):
        np.testing.assert_array_equal(got[keep], ref[keep])


def test_a_failing_cgp_evaluation_fails_alone(handle):
    """tests/test_gpu_cgp.py's failing row (lambda = 0, theta so small that G = 1: a second pivot of exactly 0) among good rows of
    two sets, with and without a held-out row."""
    pairs = [synthetic_design(30, 2, 9 + c) for c in range(2)]
    Xs, ys = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    good = np.array([0.3, 3.0, 2.0, 9.0, 8.0, 0.5])
    bad = np.array([0.0, 1e-17, 1e-17, 9.0, 8.0, 0.5])
    rows = np.stack([good, bad, good * np.array([1, 1.1, 1, 1, 1, 1]), bad, good])
    set_of = np.array([1, 0, 0, 1, 1], dtype=np.int32)
    skip = np.array([-1, -1, 3, 3, 29], dtype=np.int32)
    rc, val, beta, tau2, loo, st = _raw_cgp(handle, Xs, ys, rows, set_of, skip)
    assert rc == 2 and st.tolist() == [0, 2, 0, 2, 0]
    for b in (1, 3):
        assert np.isnan(val[b]) and np.isnan(beta[b]) and np.isnan(tau2[b]) and np.isnan(loo[b])
    _same((val, beta, tau2, loo, st), _cgp_per_set(handle, Xs, ys, rows, set_of, skip))
    assert np.isfinite(val[[0, 2, 4]]).all()


def test_refusals_come_before_anything_is_copied_or_launched(handle):
    from ccgp_amd import api
    Xs, ys, P, set_of = _profile_case(14, 2, 2, 3, 7, 600)
    Xc, yc, Pc, setc, skip = _cgp_case(10, 2, 3, 7, 601)
    handle.profile_batch_sets(Xs, ys, 2, P, set_of)
    handle.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip)
    before = handle.workspace_bytes()
    low, high = set_of.copy(), set_of.copy()
    low[3], high[6] = -1, 3
    cases = [dict(C=0), dict(C=-2), dict(B=-1), dict(set_of=low), dict(set_of=high)]
    for kw in cases + [dict(null=(name,)) for name in ("Xs", "ys", "params", "set", "loglik", "sigma2")]:
        kw = dict(kw)
        so = kw.pop("set_of", set_of)
        rc, ll, s2, beta, g, st = _raw_profile(handle, Xs, ys, 2, P, so, **kw)
        assert rc == EINVAL, kw
        sentinel = [name for name in ("loglik", "sigma2") if name not in kw.get("null", ())]
        assert all((dict(loglik=ll, sigma2=s2)[k] == 7.5).all() for k in sentinel), kw
        assert (beta == 7.5).all() and (g == 7.5).all() and (st == 77).all(), kw
    sk_low, sk_high = skip.copy(), skip.copy()
    sk_low[2], sk_high[4] = -2, 10
    for kw in cases + [dict(skip=sk_low), dict(skip=sk_high)] + [dict(null=(name,)) for name in ("Xs", "ys", "params", "set", "val")]:
        kw = dict(kw)
        so, sk = kw.pop("set_of", setc), kw.pop("skip", skip)
        rc, val, beta, tau2, loo, st = _raw_cgp(handle, Xc, yc, Pc, so, sk, **kw)
        assert rc == EINVAL, kw
        assert ("val" in kw.get("null", ()) or (val == 7.5).all()) and (st == 77).all(), kw
        assert (beta == 7.5).all() and (tau2 == 7.5).all() and (loo == 7.5).all(), kw
    # the skip rule's last clause: a held-out row needs a design of at least two points (0 is a row of n = 1, and refused)
    rc = _raw_cgp(handle, np.zeros((2, 1, 2)), np.ones((2, 1)), np.ones((2, 6)), np.array([0, 1], dtype=np.int32),
                  np.array([0, -1], dtype=np.int32))
    assert rc[0] == EINVAL and all((o == 7.5).all() for o in rc[1:5]) and (rc[5] == 77).all()
    # the CGP call's shape limit is the single-set call's, before any launch
    X129 = np.stack([synthetic_design(129, 2, 1)[0]] * 2)
    rc = _raw_cgp(handle, X129, np.zeros((2, 129)), np.ones((2, 6)), np.array([0, 1], dtype=np.int32), None)
    assert rc[0] == EUNSUPPORTED and (rc[1] == 7.5).all() and (rc[5] == 77).all()
    assert handle.workspace_bytes() == before
    # B == 0 is CCGP_OK, as in the single-set calls
    rc = _raw_profile(handle, Xs, ys, 2, P, set_of, B=0)
    assert rc[0] == 0 and (rc[1] == 7.5).all() and (rc[4] == 7.5).all() and (rc[5] == 77).all()
    rc = _raw_cgp(handle, Xc, yc, Pc, setc, skip, B=0)
    assert rc[0] == 0 and (rc[1] == 7.5).all() and (rc[5] == 77).all()
    assert api.lib().ccgp_profile_batch_sets(None, None, 1, 1, None, 1, 1, None, None, 1, None, None, None, None, None) == EINVAL
    assert api.lib().ccgp_cgp_state_batch_sets(None, None, 1, 1, None, 1, None, None, 1, None, None, None, None, None, None) == EINVAL


# ----------------------------------------------------------------------------- 5. cuts
def test_the_workspace_limit_cuts_the_call_and_changes_no_bit(handle):
    """1 MiB, the smallest limit.  A profile row at K = 2, d = 2 costs 8 (2 P + 3) + 8 = 128 bytes: 8192 rows a chunk; a CGP row at
    d = 2 costs 8 (6 + 4) + 12 = 92 bytes: 11397 rows a chunk.  Both calls below are cut into four chunks, the last one short."""
    from ccgp_amd import api
    Xs, ys, P0, _ = _profile_case(14, 2, 2, 3, 64, 500)
    rng = np.random.default_rng(501)
    B = 3 * 8192 + 5
    P = P0[rng.integers(0, 64, B)] * (1.0 + 1e-3 * rng.random((B, 1)))
    set_of = _set_of(rng, 3, B)
    whole = handle.profile_batch_sets(Xs, ys, 2, P, set_of)
    Xc, yc, Pc0, _, _ = _cgp_case(6, 2, 2, 64, 502)
    Bc = 3 * 11397 + 3
    pick = rng.integers(0, 64, Bc)
    setc = _set_of(rng, 2, Bc)
    Pc = np.stack([rows_in_the_box(Xc[c], 64, 503 + c) for c in range(2)])[setc, pick]
    skip = np.where(rng.random(Bc) < 0.5, -1, rng.integers(0, 6, Bc)).astype(np.int32)
    wholec = handle.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip)
    h2 = api.Handle(0)
    try:
        h2.set_workspace_limit(1 << 20)
        cut, t = _timed(h2, lambda: h2.profile_batch_sets(Xs, ys, 2, P, set_of))
        assert t["fused"][1] == 4, t
        cutc, tc = _timed(h2, lambda: h2.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip))
        assert tc["fused"][1] == 4, tc
        assert h2.workspace_bytes()[0] <= (1 << 20) + (1 << 18) + 8192
    finally:
        h2.close()
    _same(cut, whole)
    _same(cutc, wholec)
    assert not whole[4].any()
    # and the rows are the single-set call's: the first 300 of each
    _same([o[:300] for o in whole], _profile_per_set(handle, Xs, ys, 2, P[:300], set_of[:300], True))
    _same([o[:300] for o in wholec], _cgp_per_set(handle, Xc, yc, Pc[:300], setc[:300], skip[:300]))


# ----------------------------------------------------------------------------- 6. CGP bits
@pytest.mark.parametrize("n,d,C,B", CGP_SHAPES, ids=["n%d-d%d-C%d-B%d" % s for s in CGP_SHAPES])
def test_cgp_rows_have_the_bits_of_the_single_set_call(handle, n, d, C, B):
    Xs, ys, P, set_of, skip = _cgp_case(n, d, C, B, 700 + n)
    want = _cgp_per_set(handle, Xs, ys, P, set_of, skip)
    assert not want[4].any() and np.isfinite(want[0]).all() and np.isfinite(want[3][skip >= 0]).all()
    _same(handle.cgp_state_batch_sets(Xs, ys, P, set_of, skip=skip), want)
    _same(handle.cgp_state_batch_sets(Xs, ys, P, set_of), _cgp_per_set(handle, Xs, ys, P, set_of, None))


# ----------------------------------------------------------------------------- 8. the handle's past
def test_bits_do_not_depend_on_what_the_buffers_held():
    """Both calls on a fresh handle whose every buffer starts as 0xFF bytes (NaN doubles, -1 ints) -- the handle is too small
    for the call, so the call itself regrows workspace, staging and pinned buffer under the fill --, and again after the
    grown buffers were filled once more."""
    from ccgp_amd import api
    Xs, ys, P, set_of = _profile_case(14, 2, 2, 3, 7, 114)
    Xc, yc, Pc, setc, skip = _cgp_case(6, 2, 2, 5, 706)
    ref = api.Handle(0)
    try:
        want = ref.profile_batch_sets(Xs, ys, 2, P, set_of)
        want_v = ref.profile_batch_sets(Xs, ys, 2, P, set_of, grad=False)
        wantc = ref.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip)
    finally:
        ref.close()
    h = api.Handle(0)
    try:
        h.debug_fill_scratch(0xFF)
        assert h.workspace_bytes() == (0, 0)
        _same(h.profile_batch_sets(Xs, ys, 2, P, set_of), want)
        _same(h.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip), wantc)
        _same(h.profile_batch_sets(Xs, ys, 2, P, set_of, grad=False), want_v)
        assert h.workspace_bytes()[0] > 0
        h.debug_fill_scratch(0xFF)
        _same(h.cgp_state_batch_sets(Xc, yc, Pc, setc, skip=skip), wantc)
        _same(h.profile_batch_sets(Xs, ys, 2, P, set_of), want)
    finally:
        h.close()


# ----------------------------------------------------------------------------- 9. fits on the device
def _same_dict(got, want, skip=()):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in skip:
            continue
        if isinstance(want[k], np.ndarray):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        else:
            assert got[k] == want[k], k


def _twelve(c):
    X, y = synthetic_design(12, 2, 40 + c)
    Xt, yt = synthetic_design(6, 2, 70 + c)
    return X, y * (1.0 + 0.2 * c) + 0.3 * c * X[:, 0], Xt, yt * (1.0 + 0.2 * c) + 0.3 * c * Xt[:, 0]


@pytest.mark.parametrize("which", ["synthetic", "gv"])
def test_kriging_fits_in_lockstep_are_the_per_set_fits(handle, which):
    from ccgp_amd import fit
    sets = [_twelve(c)[:2] for c in range(3)] if which == "synthetic" else [load_gv(50, i)[:2] for i in (1, 2, 3)]
    alone = [fit.ordinary_kriging_fit(handle, D, y) for D, y in sets]
    (got, t) = _timed(handle, lambda: fit.ordinary_kriging_fit_sets(handle, [s[0] for s in sets], [s[1] for s in sets]))
    for c in range(3):
        _same_dict(got[c], alone[c])
    counts = [a["calls"] for a in alone]
    print("%s: per-set calls %s (final one included), group launches %s" % (which, counts, t["fused"][1]))
    # gradient calls: the largest per-set count (one launch each); the final value-only call goes set by set: three launches
    assert t["fused"][1] == (max(counts) - 1) + 3 and t["diag"][1] == 0


def test_cgp_fits_in_lockstep_are_the_per_set_fits(handle):
    from ccgp_amd import cgp
    sets = [synthetic_design(10, 2, 90 + c) for c in range(2)]
    alone = [cgp.CGP(handle, X, y, rng=c + 1) for c, (X, y) in enumerate(sets)]
    got = cgp.CGP_sets(handle, [s[0] for s in sets], [s[1] for s in sets], rngs=[1, 2])
    for c in range(2):
        _same_dict(got[c], alone[c], skip=("calls", "evaluations", "refinement_calls", "seconds"))
        assert got[c]["evaluations"] == alone[c]["evaluations"]
    ref_calls = [a["refinement_calls"] for a in alone]
    assert got[0]["refinement_calls"] == max(ref_calls) and got[0]["calls"] == max(ref_calls) + 2 + 2 < sum(a["calls"] for a in alone)


def test_study_has_the_same_tables_with_fewer_device_calls(handle):
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    gp = CombinedGP("GV", handle=handle)
    sets = [_twelve(c) for c in range(3)]
    arms = {on: fit.study(gp, sets, 0.05, 300, 60, 20, 0.5, net_samp_size=40, rngs=[1, 2, 3], cgp=True, single=True,
                          lockstep_fits=on) for on in (False, True)}
    off, on = arms[False], arms[True]
    assert on["sigma2"] == off["sigma2"]
    for i in range(3):
        assert sorted(on["tables"][i]) == sorted(off["tables"][i])
        for k, v in off["tables"][i].items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(on["tables"][i][k], v, err_msg=k)
        _same_dict(on["tables"][i]["single"], off["tables"][i]["single"])
        _same_dict(on["tables"][i]["CGP"], off["tables"][i]["CGP"], skip=("calls", "evaluations", "refinement_calls", "seconds"))
        assert on["summaries"][i] == off["summaries"][i]
        np.testing.assert_array_equal(on["draws"][i], off["draws"][i])
        np.testing.assert_array_equal(on["chains"][i]["sample"], off["chains"][i]["sample"])
    assert on["pooled"] == off["pooled"]
    print("device calls per set: %s; in lockstep: %s" % (off["calls"], on["calls"]))
    assert on["calls"]["single"] == 0 < off["calls"]["single"] == off["calls"]["sigma2"]
    assert 0 < on["calls"]["sigma2"] < off["calls"]["sigma2"] and 0 < on["calls"]["cgp"] < off["calls"]["cgp"]
    assert sum(on["calls"].values()) < sum(off["calls"].values())
