"""ccgp_mixed_logdet_grad_designs -- d log det R_mixed / d X of candidate designs (small_reg_kernel, INV = 3) -- and the
design search built on it (CombinedGP.Entropy_optim / Batch_Entropy_optim, Batch Sequential ME Design.R:886-948) on the
device: against a numpy fp64 reference and mpmath, batch independence, failures, limits, the stored first-batch design
of the reference, and the R shim routine.  (tests/test_gpu_design_exact.py holds the same values component-wise to a
long-double reference, on every instance of the kernel.)"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from design_ref import (BSQ_PRIOR, design_distance, initial_me_design, logdet_grad_general, mixed_R_general,
                        numpy_evaluator, params_row, projected_gradient)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
EINVAL, EUNSUPPORTED = -1, -4   # include/ccgp.h


def _case(rng, n, d, K):
    """A random design with a parameter row that keeps R well enough conditioned to factorise: theta scaled so that
    neighbouring points (spacing ~ 2 n^(-1/d)) correlate at exp(-1) .. exp(-4)."""
    X = rng.uniform(-1.0, 1.0, (n, d))
    w = rng.uniform(0.2, 1.0, K)
    th = rng.uniform(1.0, 4.0, (K, d)) * (n ** (1.0 / d) / 2.0) ** 2 / d
    return X, np.concatenate([w, th.ravel()])


def _band(X, K, row, n_fixed, C=64.0):
    """|error| bound per gradient entry: C eps cond_1(R) gen times the sum of the absolute values of the terms.  gen: the
    kernel forms the exponent in the reference's corr.vec order, theta'x_i^2 + theta'x_j^2 - 2 x_i'Theta x_j (HX:373),
    whose absolute error is eps theta'(x_i^2 + x_j^2) <= 2 eps sum_k theta_k on the box -- an error of R's entries of that
    relative size, which R^-1 amplifies by cond(R)."""
    R, Rq, wh, th = mixed_R_general(X, K, row)
    A = np.linalg.inv(R)
    diff = X[:, None, :] - X[None, :, :]
    S = np.einsum("q,qk,qij->ijk", wh, th, Rq)
    scale = 4.0 * np.einsum("ij,ijk,ijk->ik", np.abs(A), np.abs(diff), S)[n_fixed:]
    cond = np.linalg.norm(R, 1) * np.linalg.norm(A, 1)
    gen = 1.0 + 2.0 * th.sum(axis=1).max()
    return C * EPS * cond * gen * (scale + 1e-300), cond, gen


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("d", [1, 2, 4, 9])
def test_gradient_matches_numpy(handle, K, d):
    rng = np.random.default_rng(100 * K + d)
    for n in (5, 14, 21, 64, 100, 128):
        X, row = _case(rng, n, d, K)
        designs = np.stack([X] + [_case(rng, n, d, K)[0] for _ in range(2)])
        ld_ref, _ = handle.mixed_logdet_designs(designs, K, row)
        for nf in sorted({0, max(n - 7, 0), n - 1}):
            ld, g, st = handle.mixed_logdet_grad_designs(designs, K, row, nf)
            assert g.shape == (3, n - nf, d)
            for b in range(3):
                want_ld, want_g = logdet_grad_general(designs[b], K, row, nf)
                band, cond, gen = _band(designs[b], K, row, nf)
                assert st[b] == 0, (n, d, K, nf, b, cond)
                assert abs(ld[b] - ld_ref[b]) <= 1e-12 * max(1.0, abs(ld_ref[b])), (n, d, K, nf, b)
                assert abs(ld[b] - want_ld) <= 1e-10 * max(1.0, abs(want_ld)) + 8 * EPS * cond * gen * n, (n, d, K, nf, b)
                err = np.abs(g[b] - want_g)
                bad = err > band
                assert not bad.any(), (n, d, K, nf, b, cond, np.argwhere(bad)[:3], err[bad][:3], band[bad][:3], want_g[bad][:3])


def test_gradient_matches_mpmath_at_50_digits(handle):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    rng = np.random.default_rng(7)
    for n, d, K, nf in ((5, 2, 2, 0), (14, 2, 2, 7), (21, 4, 3, 14)):
        X, row = _case(rng, n, d, K)
        _, g, st = handle.mixed_logdet_grad_designs(X[None], K, row, nf)
        assert st[0] == 0
        w2 = [mp.mpf(float(v)) ** 2 for v in row[:K]]
        th = [[mp.mpf(float(row[K + q * d + k])) for k in range(d)] for q in range(K)]
        sw = sum(w2)
        Xm = [[mp.mpf(float(X[i, k])) for k in range(d)] for i in range(n)]
        Rq = [mp.matrix(n, n) for _ in range(K)]
        R = mp.matrix(n, n)
        for q in range(K):
            for i in range(n):
                for j in range(n):
                    Rq[q][i, j] = mp.exp(-sum(th[q][k] * (Xm[i][k] - Xm[j][k]) ** 2 for k in range(d)))
                    R[i, j] += w2[q] * Rq[q][i, j] / sw
        A = R ** -1
        band, cond, _ = _band(X, K, row, nf)
        for i in range(nf, n):
            for k in range(d):
                v = -4 * sum(A[i, j] * (Xm[i][k] - Xm[j][k]) * sum(w2[q] / sw * th[q][k] * Rq[q][i, j] for q in range(K))
                             for j in range(n) if j != i)
                assert abs(g[0, i - nf, k] - float(v)) <= band[i - nf, k], (n, i, k, g[0, i - nf, k], float(v))


def test_batch_independence_and_a_failing_design(handle):
    rng = np.random.default_rng(3)
    designs = rng.uniform(-1.0, 1.0, (64, 14, 2))
    designs[10, 3] = designs[10, 2]                 # two coincident rows: singular R
    row = params_row(*BSQ_PRIOR, 2)
    ld, g, st = handle.mixed_logdet_grad_designs(designs, 2, row, 0)
    assert st[10] != 0 and np.isnan(ld[10]) and np.isnan(g[10]).all()
    assert (np.delete(st, 10) == 0).all() and np.isfinite(np.delete(g, 10, axis=0)).all()
    for b in (0, 9, 11, 63):
        ld1, g1, st1 = handle.mixed_logdet_grad_designs(designs[b:b + 1], 2, row, 0)
        assert st1[0] == 0 and np.array_equal(ld1[0], ld[b]) and np.array_equal(g1[0], g[b])
    ld5, g5, _ = handle.mixed_logdet_grad_designs(designs, 2, row, 5)
    assert np.array_equal(ld5, ld, equal_nan=True) and np.array_equal(g5[:11], g[:11, 5:], equal_nan=True)


def test_limits_and_arguments(handle):
    from ccgp_amd import api
    row = params_row(*BSQ_PRIOR, 2)
    X = np.random.default_rng(0).uniform(-1.0, 1.0, (1, 129, 2))
    with pytest.raises(api.CcgpError) as e:
        handle.mixed_logdet_grad_designs(X, 2, row, 0)
    assert e.value.code == EUNSUPPORTED
    with pytest.raises(api.CcgpError) as e:
        handle.mixed_logdet_grad_designs(X[:, :14], 2, row, 14)
    assert e.value.code == EINVAL
    handle.set_kernel(api.KERNEL_MATERN, 2.5)
    try:
        with pytest.raises(api.CcgpError) as e:
            handle.mixed_logdet_grad_designs(X[:, :14, :1], 2, params_row(*BSQ_PRIOR, 1), 0)
        assert e.value.code == EUNSUPPORTED
    finally:
        handle.set_kernel(api.KERNEL_GAUSS)


def test_stored_initial_design_is_a_kuhn_tucker_point_on_the_device(handle):
    D0 = initial_me_design()
    _, g, st = handle.mixed_logdet_grad_designs(D0[None], 2, params_row(*BSQ_PRIOR, 2), 0)
    assert st[0] == 0 and projected_gradient(D0, -g[0]) <= 1e-4


def test_entropy_optim_reproduces_the_stored_initial_design(handle):
    from ccgp_amd.rsurface import CombinedGP
    D0 = initial_me_design()
    gp = CombinedGP("BSQ", handle=handle)
    r = gp.Entropy_optim(14, 2, *BSQ_PRIOR, 20, rng=0)
    ld0 = handle.mixed_logdet_designs(D0[None], 2, params_row(*BSQ_PRIOR, 2))[0][0]
    assert r["logdet"] >= ld0 - 1e-7 and design_distance(r["Design"], D0) <= 1e-3
    assert r["log_entropy"] == np.exp(r["logdet"]) and r["Design"].shape == (14, 2)
    assert r["designs"].shape == (20, 14, 2) and r["device_calls"] < int(r["iterations"].sum())


def test_batch_entropy_optim_agrees_with_numpy_from_the_same_starts(handle):
    from ccgp_amd import design
    from ccgp_amd.rsurface import CombinedGP
    D0 = initial_me_design()
    starts = design.make_starts(25, 7, 2, 0)
    want = design.minimize_starts(numpy_evaluator(*BSQ_PRIOR, D_old=D0), starts)
    r = CombinedGP("BSQ", handle=handle).Batch_Entropy_optim(D0, 7, 2, *BSQ_PRIOR, 25, starts=starts)
    best = -want["f"].min()
    assert abs(r["logdet"] - best) <= 1e-9 * abs(best), (r["logdet"], best)
    assert r["Design"].min() >= -1.0 and r["Design"].max() <= 1.0


def test_r_shim_routine_matches_the_handle(handle):
    sys.path.insert(0, os.path.join(ROOT, "tests", "r_mock"))
    import rmock
    os.environ.pop("CCGP_DEVICES", None)
    R = rmock.MockR()
    try:
        R.reset()
        rng = np.random.default_rng(5)
        designs = rng.uniform(-1.0, 1.0, (5, 21, 2))
        designs[2, 20] = designs[2, 19]
        row = params_row(*BSQ_PRIOR, 2)
        Xs = np.stack([np.asfortranarray(Dd).ravel(order="F") for Dd in designs], axis=1)
        got = R.dot_call("ccgp_R_mixed_logdet_grad_designs", R.real(Xs), R.integer(21), R.integer(2), R.integer(2),
                         R.real(row), R.integer(14))
        ld, g, st = handle.mixed_logdet_grad_designs(designs, 2, row, 14)
        assert st[2] != 0 and R.is_na(got["logdet"][2]).all() and R.is_na(got["grad"][:, 2]).all()
        ok = [0, 1, 3, 4]
        assert np.array_equal(got["logdet"][ok], ld[ok])
        assert got["grad"].shape == (7 * 2, 5)
        for b in ok:
            assert np.array_equal(got["grad"][:, b], g[b].ravel(order="F"))
        R.assert_clean()
    finally:
        R.unload()
