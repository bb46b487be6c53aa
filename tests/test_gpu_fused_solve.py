"""The fused-solve route of the launch-per-phase blocked sweep (CCGP_OPT_FUSED_SOLVE; csrc/blocked.hip: chol_diag_solve_kernel,
chol_update_solve_kernel) against the update + trsm launches it replaces from block column 1 on.  A tile's panel solve
L_ij = T_ij W_j' runs in the workgroup that updated the tile, on T held in LDS, with the summation order of chol_trsm_kernel:
every result must agree BIT FOR BIT with option 0 -- likelihood, beta, status (also of evaluations that fail), kept factors --
and with the dataflow scheduler.  Option 2 takes the route whatever the number of matrices, so the shapes here stay small;
option 1 (default) takes it when the chunk fills whole steps of 256 workgroups.  Reference anchor: the batch is the grid loop
of choose.hyperpars, Heat Exchanger Emulator/Combined GP Heat Exchanger.R:584-595."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(2 * np.pi * X).sum(axis=1) + 0.1 * rng.normal(size=n)
    return X, y, rng


def draws(rng, B, K, d, rough=20.0):
    P = np.empty((B, K + K * d))
    for b in range(B):
        w = 0.15 + 0.55 * rng.dirichlet(np.ones(K))
        th = np.exp(rng.uniform(np.log(0.5), np.log(50.0), size=(K, d)))
        th[K - 1] = np.maximum(th[K - 1], rough)
        P[b] = np.concatenate([w, th.ravel()])
    return P


def rough_for(n, d):
    """Lower bound of the roughest component's theta: 20 as in the benchmark's draws; in two dimensions n uniform points lie
    1 / sqrt(n) apart, and a Gaussian correlation needs theta of the order n to keep such neighbours apart (positive
    definite to working precision -- checked on the host with the fp64 oracle when the shapes were chosen)."""
    return 20.0 if d > 2 else 4.0 * n


def with_route(handle, fused, fn, sched=0):
    """fn() with CCGP_OPT_FUSED_SOLVE = fused on the launch-per-phase sweep (or under scheduler mode `sched`)."""
    from ccgp_amd import api
    handle.set_option(api.OPT_FUSED_SOLVE, fused)
    handle.set_option(api.OPT_SCHED, sched)
    try:
        return fn()
    finally:
        handle.set_option(api.OPT_FUSED_SOLVE, 1)
        handle.set_option(api.OPT_SCHED, 3)


def same(a, b):
    """Element for element the same bits; NaN only where the other has NaN."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def launch_counts(handle, fn):
    handle.enable_timing(True)
    try:
        out = fn()
        t = handle.get_timing()
    finally:
        handle.enable_timing(False)
    return out, t["update"][1], t["trsm"][1]


# nt = 2 with almost only padding and B % 8 != 0; nt = 2 whole; padding inside the last tile row; nt = 3 (a row solved in one
# launch is the column panel of the next); more rows; k-loops of several blocks
SHAPES = [(129, 3), (256, 8), (300, 5), (384, 9), (640, 16), (1000, 8)]


@pytest.mark.parametrize("n,B", SHAPES)
@pytest.mark.parametrize("d,K", [(2, 1), (5, 3)])
def test_same_bits_as_the_trsm_launches(handle, n, B, d, K):
    X, y, rng = synth(n, d, 1000 * d + n)
    P = draws(rng, B, K, d, rough_for(n, d))
    for mode, tau2 in ((0, 0.0), (1, 4.0)):
        ref = with_route(handle, 0, lambda: handle.loglik_batch(X, y, K, P, 1.3, mode, tau2))
        assert np.isfinite(ref[0]).all() and (ref[2] == 0).all()
        (got, n_update, n_trsm) = launch_counts(
            handle, lambda: with_route(handle, 2, lambda: handle.loglik_batch(X, y, K, P, 1.3, mode, tau2)))
        nt = (n + 127) // 128
        assert (n_update, n_trsm) == (2 * (nt - 1), 1), "option 2 did not take the fused route"
        assert same(ref, got), (n, B, d, K, mode)


def test_default_takes_the_route_when_the_batch_fills_whole_steps(handle):
    n, d, K, B = 384, 3, 2, 256
    nt = 3
    X, y, rng = synth(n, d, 5)
    P = draws(rng, B, K, d, rough=80.0)
    ref = with_route(handle, 0, lambda: handle.loglik_batch(X, y, K, P, 1.0))
    assert np.isfinite(ref[0]).all()
    got, n_update, n_trsm = launch_counts(handle, lambda: handle.loglik_batch(X, y, K, P, 1.0))   # options at default
    assert n_trsm == 1 and n_update == 2 * (nt - 1)
    assert same(ref, got)
    # 255 matrices are not whole steps: the update + trsm launches, and per matrix the bits of the batch of 256
    got, n_update, n_trsm = launch_counts(handle, lambda: handle.loglik_batch(X, y, K, P[:255], 1.0))
    assert n_trsm == nt and n_update == nt - 1
    assert same([r[:255] for r in ref], got)


def test_a_failing_matrix_keeps_its_status_and_the_others_their_bits(handle):
    """tests/exact_designs.py: design row 199 is a copy of an earlier row except in a separator dimension, and draw 4 of 9
    alone gives that dimension theta = 0 -- for that draw the row is duplicated to the bit and pivot 200 is exactly 0.  The
    other draws keep the rows apart and have ordinary correlation lengths, so their matrices are full and positive definite."""
    import exact_designs as ex
    n, K, B, bad = 384, 2, 9, 4
    D = ex.ExactDesign(n, (200,))
    rng = np.random.default_rng(17)
    P = np.empty((B, K + K * D.d))
    for b in range(B):
        P[b] = np.concatenate([0.3 + rng.uniform(size=K), rng.uniform(0.5, 3.0, size=K * D.d)])
    P[bad] = D.row(K, zero=(0,))
    ref = with_route(handle, 0, lambda: handle.loglik_batch(D.X, D.y, K, P, 1.3))
    got = with_route(handle, 2, lambda: handle.loglik_batch(D.X, D.y, K, P, 1.3))
    ok = np.arange(B) != bad
    for ll, beta, st in (ref, got):
        assert st[bad] == 200 and np.isnan(ll[bad]) and np.isnan(beta[bad])
        assert (st[ok] == 0).all() and np.isfinite(ll[ok]).all() and np.isfinite(beta[ok]).all()
    assert same(ref, got)
    # the neighbours are untouched: the same call without the failing draw
    alone = with_route(handle, 2, lambda: handle.loglik_batch(D.X, D.y, K, P[ok], 1.3))
    assert same([r[ok] for r in got], alone)


def test_other_jobs_stay_correct_under_option_2(handle):
    """Prediction tables and the gradient carry extra tile rows and keep the update + trsm launches; a kept factor set has
    none and is built on the fused route: the factor it leaves in memory serves predictions with the bits of option 0."""
    n, d, K, m = 300, 3, 2, 70
    X, y, rng = synth(n, d, 21)
    P = draws(rng, 6, K, d, rough=80.0)
    Xt = rng.uniform(size=(m, d))
    ref_p = with_route(handle, 0, lambda: handle.predict_batch(X, y, K, P, Xt, 1.5))
    ref_g = with_route(handle, 0, lambda: handle.loglik_grad_batch(X, y, K, P, 1.0))
    assert np.isfinite(ref_p[0]).all() and np.isfinite(ref_g[2]).all()
    got_p, _, n_trsm = launch_counts(handle, lambda: with_route(handle, 2, lambda: handle.predict_batch(X, y, K, P, Xt, 1.5)))
    assert same(ref_p, got_p)
    assert same(ref_g, with_route(handle, 2, lambda: handle.loglik_grad_batch(X, y, K, P, 1.0)))

    def kept():
        with handle.factor_batch(X, y, K, P, 1.5) as fs:
            return [fs.loglik.copy(), fs.beta.copy(), fs.status.copy()] + list(fs.predict(Xt))
    ref_k = with_route(handle, 0, kept)
    got_k = with_route(handle, 2, kept)
    assert same(ref_k, got_k)
    assert same(ref_p[:2], got_k[3:5])


def test_same_bits_as_the_scheduler(handle):
    n, d, K, B = 2048, 4, 2, 32
    X, y, rng = synth(n, d, 31)
    P = draws(rng, B, K, d)
    sched = with_route(handle, 0, lambda: handle.loglik_batch(X, y, K, P, 1.0), sched=2)
    fused = with_route(handle, 2, lambda: handle.loglik_batch(X, y, K, P, 1.0))
    assert np.isfinite(sched[0]).all()
    assert same(sched, fused)


def test_two_calls_give_identical_bits(handle):
    n, d, K, B = 640, 3, 2, 16
    X, y, rng = synth(n, d, 41)
    P = draws(rng, B, K, d, rough=80.0)
    a = with_route(handle, 2, lambda: handle.loglik_batch(X, y, K, P, 1.0))
    b = with_route(handle, 2, lambda: handle.loglik_batch(X, y, K, P, 1.0))
    assert np.isfinite(a[0]).all()
    assert same(a, b)


def test_the_headline_matrices(handle):
    """The first 8 draws of the benchmark's config 4 (n = 4096): option 2 against option 0 bit for bit, and against the CPU
    potrf digest at the benchmark's own tolerances."""
    import bench
    X, y, P, K = bench.cfg4_inputs(512)
    P = P[:8]
    with open(os.path.join(ROOT, "tests", "golden", "cfg4_loglik_512.json")) as fh:
        ref = json.load(fh)
    old = with_route(handle, 0, lambda: handle.loglik_batch(X, y, K, P, 1.0))
    new = with_route(handle, 2, lambda: handle.loglik_batch(X, y, K, P, 1.0))
    assert (new[2] == 0).all()
    assert same(old, new)
    assert np.allclose(new[0], np.array(ref["loglik"])[:8], rtol=1e-9, atol=0.0)
    assert np.allclose(new[1], np.array(ref["beta"])[:8], rtol=1e-7, atol=1e-10)
