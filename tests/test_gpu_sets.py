"""Many training sets of one shape in one call: ccgp_loglik_batch_sets / ccgp_logpost_sets, and the lockstep inference on
top of them (fit.Metro_sets, fit.study).

The contract is one of BITS: row b has exactly the bits the single-set call returns for it on set set[b] alone, whatever C,
B, the row's position or the order of `set`.  Every comparison below is `==` on float64 arrays (np.testing.
assert_array_equal with NaN == NaN), never a tolerance; the reference is the single-set entry point on the same device.

Shapes (n, d, K, C, B): the smallest design, an odd one, the Ground-Vibrations size-50 sets at the size of a speculative step
(9 chains x 7 candidates), n = 8 * 8 where the single-set call takes the FULL instance, 13 x 13 blocks on one wave, the
boundary of the 8 x 8 grid (104 | 105) and the largest order; the shapes above 64 rows per call cross to the
one-wave-per-matrix grid.  Singular rows: every theta = 1e-4 at d <= 3 and 1e-9 at d = 9, which tests/test_gpu_loo.py
establishes as singular under the pivot rule."""

import numpy as np
import pytest

from conftest import load_gv, synthetic_design
from test_gpu_gradient_exact import _timed
from test_gpu_random_shapes import draws

pytestmark = pytest.mark.gpu
EINVAL = -1


# ----------------------------------------------------------------------------- cases
def _sets_case(n, d, K, C, B, seed):
    """C designs with their responses and variances, B well-conditioned rows, and a set index per row: unsorted, uneven
    counts, and (C >= 3) set 1 with no rows."""
    rng = np.random.default_rng(seed)
    if (n, d) == (50, 9):
        gv = [load_gv(50, i + 1) for i in range(C)]
        Xs, ys = np.stack([g[0] for g in gv]), np.stack([g[1] for g in gv])
        P = np.empty((B, K + K * d))
        for b in range(B):   # the Combined GP's two isotropic components on these inputs: a smooth and a rough one
            p = rng.uniform(0.2, 0.8)
            P[b] = np.concatenate([[p, 1.0 - p], np.full(d, rng.uniform(0.03, 0.15)), np.full(d, rng.uniform(0.8, 3.0))])
    else:
        pairs = [synthetic_design(n, d, seed + 10 * c) for c in range(C)]
        Xs, ys = np.stack([p[0] for p in pairs]), np.stack([p[1] * (1.0 + 0.1 * c) for c, p in enumerate(pairs)])
        P = draws(rng, n, d, K, B)
    s2 = 0.5 + rng.random(C)
    used = [c for c in range(C) if not (C >= 3 and c == 1)]
    weights = np.arange(1, len(used) + 1, dtype=float) ** 2
    set_of = rng.choice(used, size=B, p=weights / weights.sum())
    lead = used[::-1][:B]                    # (where B allows) every used set has a row, in descending order to begin with
    set_of[:len(lead)] = lead
    return Xs, ys, s2, P, set_of.astype(np.int32)


def _per_set(handle, Xs, ys, s2, K, P, set_of, mode, tau2):
    """The reference: the rows of every set through the single-set call."""
    B = len(P)
    ll, beta, st = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, dtype=np.int32)
    for c in np.unique(set_of):
        rows = np.flatnonzero(set_of == c)
        ll[rows], beta[rows], st[rows] = handle.loglik_batch(Xs[c], ys[c], K, P[rows], s2[c], mode, tau2)
    return ll, beta, st


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


SHAPES = [(5, 1, 1, 2, 3), (14, 2, 2, 3, 7), (50, 9, 2, 9, 63), (64, 4, 2, 2, 5), (64, 4, 2, 2, 130), (100, 2, 2, 3, 5),
          (100, 2, 2, 3, 65), (104, 2, 2, 2, 5), (104, 2, 2, 2, 65), (105, 2, 2, 2, 5), (105, 2, 2, 2, 65), (128, 3, 3, 2, 4)]


# ----------------------------------------------------------------------------- 1. bits against the single-set call
@pytest.mark.parametrize("mode,tau2", [(0, 0.0), (1, 0.5)], ids=["profile_beta", "zero_plus_tau2"])
@pytest.mark.parametrize("n,d,K,C,B", SHAPES, ids=["n%d-d%d-K%d-C%d-B%d" % s for s in SHAPES])
def test_rows_have_the_bits_of_the_single_set_call(handle, n, d, K, C, B, mode, tau2):
    Xs, ys, s2, P, set_of = _sets_case(n, d, K, C, B, 100 + n)
    want = _per_set(handle, Xs, ys, s2, K, P, set_of, mode, tau2)
    assert not want[2].any()
    _same(handle.loglik_batch_sets(Xs, ys, s2, K, P, set_of, mode, tau2), want)
    if C == 2:   # a set with no rows: everything on set 1
        only = np.ones(B, dtype=np.int32)
        _same(handle.loglik_batch_sets(Xs, ys, s2, K, P, only, mode, tau2), _per_set(handle, Xs, ys, s2, K, P, only, mode, tau2))


# ----------------------------------------------------------------------------- 2. position
@pytest.mark.parametrize("n,d,K,C,B", [(14, 2, 2, 3, 7), (50, 9, 2, 9, 63), (100, 2, 2, 3, 65)])
def test_permuting_rows_or_sets_permutes_the_outputs_and_nothing_else(handle, n, d, K, C, B):
    Xs, ys, s2, P, set_of = _sets_case(n, d, K, C, B, 200 + n)
    base = handle.loglik_batch_sets(Xs, ys, s2, K, P, set_of)
    rng = np.random.default_rng(n)
    perm = rng.permutation(B)
    got = handle.loglik_batch_sets(Xs, ys, s2, K, P[perm], set_of[perm])
    _same(got, [o[perm] for o in base])
    sp = rng.permutation(C)                      # new set j is old set sp[j]
    inv = np.argsort(sp)
    _same(handle.loglik_batch_sets(Xs[sp], ys[sp], s2[sp], K, P, inv[set_of]), base)
    # more sets and more rows around the same rows change nothing either
    Xs2, ys2, s22 = np.concatenate([Xs, Xs[:1] * 0.9]), np.concatenate([ys, ys[:1]]), np.concatenate([s2, [2.0]])
    P2, set2 = np.concatenate([P[:3], P]), np.concatenate([[C, 0, C], set_of]).astype(np.int32)
    _same([o[3:] for o in handle.loglik_batch_sets(Xs2, ys2, s22, K, P2, set2)], base)


# ----------------------------------------------------------------------------- 3. route
def test_a_reg_shape_is_one_launch(handle):
    Xs, ys, s2, P, set_of = _sets_case(50, 9, 2, 9, 63, 300)
    got, t = _timed(handle, lambda: handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of))
    assert t["fused"][1] == 1 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t
    _same(got, _per_set(handle, Xs, ys, s2, 2, P, set_of, 0, 0.0))


def test_beyond_the_instance_the_rows_go_through_the_sweep_set_by_set(handle):
    from ccgp_amd import api
    Xs, ys, s2, P, set_of = _sets_case(129, 3, 2, 2, 3, 301)
    got, t = _timed(handle, lambda: handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of))
    assert t["fused"][1] == 0 and t["diag"][1] > 0 and t["update"][1] > 0, t
    _same(got, _per_set(handle, Xs, ys, s2, 2, P, set_of, 0, 0.0))
    # the Matern family exists on the sweep only
    rng = np.random.default_rng(302)
    Xm = np.stack([np.sort(rng.random(8))[:, None] for _ in range(3)])
    ym = np.sin(6.0 * Xm[:, :, 0]) + 0.1 * np.arange(3)[:, None]
    Pm = np.stack([[0.6, 0.4, 2.0 + b, 9.0 + b] for b in range(5)])
    setm = np.array([2, 0, 2, 1, 0], dtype=np.int32)
    handle.set_kernel(api.KERNEL_MATERN, 2.5)
    try:
        gotm, tm = _timed(handle, lambda: handle.loglik_batch_sets(Xm, ym, [1.0, 1.5, 0.7], 2, Pm, setm))
        wantm = _per_set(handle, Xm, ym, [1.0, 1.5, 0.7], 2, Pm, setm, 0, 0.0)
    finally:
        handle.set_kernel(api.KERNEL_GAUSS)
    assert tm["fused"][1] == 0 and tm["diag"][1] > 0, tm
    assert not wantm[2].any()
    _same(gotm, wantm)


# ----------------------------------------------------------------------------- 4. failure contract, 6. arguments
def _raw(handle, Xs, ys, s2, K, P, set_of, C=None, B=None, mode=0, null=()):
    """ccgp_loglik_batch_sets itself, outputs pre-filled with sentinels -> (return value, loglik, beta, status)."""
    from ccgp_amd import api
    Xb, yb, s2b, idx, C0, n, d = api.Handle._sets(Xs, ys, s2, set_of, len(set_of))
    Pf = np.asfortranarray(P)
    ll, beta, st = np.full(len(P), 7.5), np.full(len(P), 7.5), np.full(len(P), 77, dtype=np.int32)
    args = dict(Xs=api._p(Xb), ys=api._p(yb), sigma2=api._p(s2b), params=api._p(Pf), set=api._ipt(idx), out=api._p(ll))
    for name in null:
        args[name] = None
    rc = api.lib().ccgp_loglik_batch_sets(handle._h, args["Xs"], n, d, args["ys"], args["sigma2"], C0 if C is None else C, K,
                                          args["params"], args["set"], len(P) if B is None else B, mode, 0.0, args["out"],
                                          api._p(beta), api._ipt(st))
    return rc, ll, beta, st


@pytest.mark.parametrize("n,d,K,C,tiny", [(14, 2, 2, 3, 1e-4), (50, 9, 2, 9, 1e-9), (100, 3, 2, 3, 1e-4)])
def test_a_singular_row_fails_alone(handle, n, d, K, C, tiny):
    Xs, ys, s2, P, set_of = _sets_case(n, d, K, C, 5, 400 + n)
    clean = handle.loglik_batch_sets(Xs, ys, s2, K, P, set_of)
    bad = P.copy()
    bad[2, K:] = tiny
    c = set_of[2]
    _, _, want_st = handle.loglik_batch(Xs[c], ys[c], K, bad[2:3], s2[c])
    assert want_st[0] != 0
    rc, ll, beta, st = _raw(handle, Xs, ys, s2, K, bad, set_of)
    assert rc == 1
    assert st[2] == want_st[0] and np.isnan(ll[2]) and np.isnan(beta[2])
    keep = np.arange(5) != 2
    assert not st[keep].any()
    np.testing.assert_array_equal(ll[keep], clean[0][keep])
    np.testing.assert_array_equal(beta[keep], clean[1][keep])


def test_refusals_come_before_anything_is_copied_or_launched(handle):
    Xs, ys, s2, P, set_of = _sets_case(14, 2, 2, 3, 7, 600)
    handle.loglik_batch_sets(Xs, ys, s2, 2, P, set_of)
    before = handle.workspace_bytes()
    low, high = set_of.copy(), set_of.copy()
    low[3], high[6] = -1, 3
    cases = [dict(C=0), dict(B=0), dict(C=-2), dict(B=-1), dict(set_of=low), dict(set_of=high), dict(mode=5)]
    cases += [dict(null=(name,)) for name in ("Xs", "ys", "sigma2", "params", "set", "out")]
    for kw in cases:
        so = kw.pop("set_of", set_of)
        rc, ll, beta, st = _raw(handle, Xs, ys, s2, 2, P, so, **kw)
        assert rc == EINVAL, kw
        assert (ll == 7.5).all() and (beta == 7.5).all() and (st == 77).all(), kw
    assert handle.workspace_bytes() == before
    from ccgp_amd import api
    assert api.lib().ccgp_loglik_batch_sets(None, None, 1, 1, None, None, 1, 1, None, None, 1, 0, 0.0, None, None, None) == EINVAL


# ----------------------------------------------------------------------------- 5. ccgp_logpost_sets
@pytest.mark.parametrize("prior,n,d,q,pars", [("GV", 50, 9, 3, None), ("ISO", 14, 2, 3, None), ("INVGAMMA", 64, 4, 3, (7, 3, 3, 28)),
                                              ("ANI", 30, 2, 4, None)])
def test_logpost_sets_is_logpost_batch_per_set(handle, prior, n, d, q, pars):
    from ccgp_amd import api
    C, B = (9, 63) if n == 50 else (3, 11)
    Xs, ys, s2, _, set_of = _sets_case(n, d, 2, C, B, 500 + n)
    rng = np.random.default_rng(d)
    lo, hi = ((0.03, 0.15), (0.8, 3.0)) if n == 50 else ((0.5, 3.0), (2.0 * n, 4.0 * n))
    T = np.stack([np.log(rng.uniform(*lo, B)), np.log(rng.uniform(*hi, B)), rng.normal(0.0, 0.8, B)] +
                 ([rng.normal(0.0, 0.3, B)] if q == 4 else []), axis=1)
    pid = getattr(api, "PRIOR_" + prior)
    got = handle.logpost_sets(Xs, ys, s2, pid, T, set_of, pars)
    assert not got[3].any()
    for c in np.unique(set_of):
        rows = np.flatnonzero(set_of == c)
        want = handle.logpost_batch(Xs[c], ys[c], s2[c], pid, T[rows], pars)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g[rows], w)
    if prior == "INVGAMMA":
        with pytest.raises(api.CcgpError) as e:
            handle.logpost_sets(Xs, ys, s2, pid, T, set_of, None)
        assert e.value.code == EINVAL


# ----------------------------------------------------------------------------- 7. the chain, 8. the study
SMALL = dict(N=200, samp_size=60, batch_size=20)


@pytest.fixture(scope="module")
def gv_fits(handle):
    """GV size-50 sets 1 - 3: sigma2 = var(y), fit.laplace per set, and fit.Metro per set at speculate 0 (seeds 1 - 3) -- the
    reference of the chain and study tests, computed once."""
    from ccgp_amd import fit
    from ccgp_amd.rsurface import CombinedGP
    gp = CombinedGP("GV", handle=handle)
    sets = [load_gv(50, i) for i in (1, 2, 3)]
    s2 = [float(np.var(s[1], ddof=1)) for s in sets]
    ests, chains, after = [], [], []
    for i, (D, y, _, _) in enumerate(sets):
        ests.append(fit.laplace(lambda rows: fit.logpost_batch(gp, D, rows, y, s2[i])[0], np.array([1.0, 1.0, 0.0])))
        rng = np.random.default_rng(i + 1)
        chains.append(fit.Metro(gp, np.array([1.0, 1.0, 0.0]), SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, D, s2[i],
                                y, rng=rng))
        after.append(rng.random())
    return gp, sets, s2, ests, chains, after


@pytest.mark.parametrize("m", [0, 3])
def test_lockstep_chains_are_the_per_set_chains(handle, gv_fits, m):
    from ccgp_amd import fit
    gp, sets, s2, ests, chains, after = gv_fits
    rngs = [np.random.default_rng(i + 1) for i in range(3)]
    r = fit.Metro_sets(gp, None, SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, [s[0] for s in sets], s2,
                       [s[1] for s in sets], rngs=rngs, speculate=m, laplace=ests)
    per_chain = []
    for i in range(3):
        got, want = r["chains"][i], chains[i]
        np.testing.assert_array_equal(got["laplace"]["mode"], want["laplace"]["mode"])   # Metro's own laplace is fit.laplace
        np.testing.assert_array_equal(got["sample"], want["sample"])
        np.testing.assert_array_equal(got["beta"], want["beta"])
        assert (got["accepted"], got["proposals"], got["geweke_p"]) == (want["accepted"], want["proposals"], want["geweke_p"])
        assert rngs[i].random() == after[i]
        per_chain.append(got["device_batches"])
        if m == 0:
            assert got["device_batches"] == want["device_batches"]
    assert r["device_batches"] == max(per_chain) < sum(per_chain)


def test_study_is_the_per_set_loop(handle, gv_fits, tmp_path):
    from ccgp_amd import fit
    gp, sets, s2, ests, chains, _ = gv_fits
    two = sets[:2]
    r = fit.study(gp, two, 0.05, SMALL["N"], SMALL["samp_size"], SMALL["batch_size"], 0.5, net_samp_size=40, sigma2s=s2[:2],
                  rngs=[1, 2], laplace=ests[:2], single=dict(theta=np.full(9, 0.5), sigma2=1.0), out_dir=str(tmp_path))
    tables = []
    for i, (D, y, Dt, yt) in enumerate(two):
        d = fit.transformed_to_draws(chains[i]["sample"][20:60])
        t = fit.compare_GP(gp, Dt, 0.05, yt, d, D, s2[i], y, exact=True, single=dict(theta=np.full(9, 0.5), sigma2=1.0))
        tables.append(t)
        for k in ("y_hat", "quant", "LL", "UL", "y_true", "y_hat_single", "LL_single", "UL_single"):
            np.testing.assert_array_equal(r["tables"][i][k], t[k])
        assert r["summaries"][i] == fit.comparison_summary(t)
    stacked = {k: np.concatenate([t[k] for t in tables]) for k in ("y_hat", "quant", "LL", "UL", "y_true", "y_hat_single",
                                                                    "LL_single", "UL_single")}
    assert r["pooled"] == fit.comparison_summary(stacked)
    assert r["groups"] == {(50, 9): [0, 1]}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["results_1.txt", "results_2.txt"]
