"""The reference of the sigma2-profiled likelihood (tests/profile_ref.py) held to what defines it, and the lockstep
ordinary-kriging fit run on the host evaluator.  No device here.

1. Envelope theorem: the reference gradient -- the mode-0 closed form at (beta_hat, sigma2_hat) -- against central
   differences of l_p itself, everything in long double.  Step h = 1e-6 relative: truncation ~h^2 = 1e-12 relative to the
   third derivative's size, rounding ~1.1e-19 |l_p| / h = 1e-11 absolute on |l_p| ~ 1e2; the components are held to 1e-6
   of their cancellation-free size, which a missing d sigma2_hat / d row term (of the size of the component) cannot pass.
2. Scale invariance: l_p(c w, theta) = l_p(w, theta) (sigma2_hat absorbs c^2), so sum_q w_q d l_p / d w_q = 0, to a few
   long-double roundings of the terms' size sum_q |w_q| scale_q.
3. Known answer: at the theta recovered from the reference's results table (tests/golden/gv_mlegp_recovered.json) sigma2_hat
   is the recorded mlegp sig2 to 1e-10 relative -- mlegp's sig2 IS Q / n.
4. The fit: fit.ordinary_kriging_fit on profile_ref.NumpyHandle reproduces the basins the device tests rely on."""
import numpy as np
import pytest

from conftest import golden, load_gv, load_qian, synthetic_design
from ccgp_amd import fit
from oracle import ccgp_oracle as orc
from profile_ref import NumpyHandle, profile_exact, profile_loglik

N, D_, K_ = 17, 3, 2


def _case():
    X, y = synthetic_design(N, D_, seed=1717)
    y = y + 0.3 * X[:, 0]
    row, _ = orc.conditioned_row(X, K_, D_, np.random.default_rng(17), 1e8)
    return X, y, row


def test_envelope_theorem_against_central_differences():
    orc.require_extended_precision()
    X, y, row = _case()
    ref = profile_exact(X, y, row, K_, D_)
    ld = np.longdouble
    for j in range(row.size):
        h = 1e-6 * abs(row[j])
        up, dn = row.copy(), row.copy()
        up[j] += h
        dn[j] -= h
        fd = (profile_loglik(X, y, up, K_, D_) - profile_loglik(X, y, dn, K_, D_)) / ld(up[j] - dn[j])
        err = abs(float(fd - ref["grad"][j]))
        print("component %d: closed form %.12g, central difference %.12g, |diff| / scale %.3g" % (
            j, float(ref["grad"][j]), float(fd), err / float(ref["scale"][j])))
        assert err <= 1e-6 * float(ref["scale"][j]), (j, float(fd), float(ref["grad"][j]))


def test_profiled_likelihood_does_not_depend_on_the_weights_scale():
    orc.require_extended_precision()
    X, y, row = _case()
    ref = profile_exact(X, y, row, K_, D_)
    w = row[:K_]
    s = float((np.asarray(w, dtype=np.longdouble) * ref["grad"][:K_]).sum())
    size = float((np.abs(w) * ref["scale"][:K_].astype(np.float64)).sum())
    print("sum_q w_q dl_p/dw_q = %.3g against a term size of %.3g" % (s, size))
    assert abs(s) <= 64 * float(np.finfo(np.longdouble).eps) * N * size
    # and the value itself: doubling every weight changes sigma2_hat by 1/4 and nothing else
    row2 = row.copy()
    row2[:K_] *= 2.0
    ref2 = profile_exact(X, y, row2, K_, D_)
    assert abs(float(ref2["loglik"] - ref["loglik"])) <= 1e-15 * abs(float(ref["loglik"]))
    assert abs(float(4 * ref2["sigma2"] - ref["sigma2"])) <= 1e-15 * float(ref["sigma2"])


def test_sigma2_at_the_recovered_mlegp_theta_is_the_recorded_sig2():
    fx = golden("gv_mlegp_recovered.json")
    D, y, _, _ = load_gv(50)
    row = np.concatenate([[1.0], fx["theta"]])
    for dtype in (np.float64, np.longdouble):
        s2 = float(profile_exact(D, y, row, 1, D.shape[1], dtype)["sigma2"])
        print("%s sigma2_hat %.15g, recorded %.15g, relative difference %.3g" % (
            np.dtype(dtype).name, s2, fx["sigma2"], abs(s2 - fx["sigma2"]) / fx["sigma2"]))
        assert abs(s2 - fx["sigma2"]) <= 1e-10 * fx["sigma2"]


@pytest.fixture(scope="module")
def host_fits():
    """The two fits of the issue's table, once for the module: Qian with 8 starts, GV train_50_1 with 8 starts."""
    out = {}
    for name, (D, y) in dict(qian=load_qian()[:2], gv=load_gv(50)[:2]).items():
        h = NumpyHandle()
        out[name] = (fit.ordinary_kriging_fit(h, D, y, starts=8, rng=0), h, D, y)
    return out


def test_lockstep_fit_on_qian_finds_both_basins(host_fits):
    r, h, D, y = host_fits["qian"]
    f = np.sort(r["f"][np.isfinite(r["f"])])
    print("Qian: %d evaluator calls (+1 final), %d points, best log-likelihood %.4f, sigma2 %.3f, per start %s" % (
        r["calls"] - 1, r["evaluations"], r["loglik"], r["sigma2"], np.round(-r["f"], 4).tolist()))
    assert h.calls == r["calls"] and h.points == r["evaluations"]
    # two basins: the best, and one more than a unit of log-likelihood below it
    best = f[0]
    assert (f - best > 1.0).any() and (f - best < 1e-3).any()
    assert 57.5 <= r["sigma2"] <= 66.75
    assert abs(r["loglik"] + best) <= 1e-9 * abs(best)


def test_lockstep_fit_on_ground_vibrations_beats_the_mlegp_theta(host_fits):
    r, h, D, y = host_fits["gv"]
    fx = golden("gv_mlegp_recovered.json")
    ll_mlegp = float(profile_exact(D, y, np.concatenate([[1.0], fx["theta"]]), 1, D.shape[1], np.float64)["loglik"])
    print("GV train_50_1: %d evaluator calls (+1 final), %d points, best log-likelihood %.4f (mlegp theta: %.4f), sigma2 %.4f" % (
        r["calls"] - 1, r["evaluations"], r["loglik"], ll_mlegp, r["sigma2"]))
    assert r["loglik"] > ll_mlegp + 1.0
    assert 2 * r["calls"] < r["evaluations"]


def test_fit_uses_the_start_points_of_ordinary_kriging_sigma2():
    """Same generator, same order: start 0 is 1 / span^2, start s > 0 the s-th uniform(0.2, 5) draw of default_rng(rng) over
    span^2; extra starts follow as given."""
    D, _, _, _ = load_qian()
    d = D.shape[1]
    span = np.maximum(D.max(axis=0) - D.min(axis=0), 1e-12)
    gen = np.random.default_rng(0)
    want = [np.log((1.0 if s == 0 else gen.uniform(0.2, 5.0, size=d)) / span ** 2) for s in range(8)]
    extra = 0.5 * np.arange(1.0, d + 1.0)[None]
    got = fit.kriging_starts(D, 8, 0, extra)
    assert got.shape == (9, d)
    assert np.array_equal(got[:8], np.stack(want)) and np.array_equal(got[8], np.log(extra[0]))
