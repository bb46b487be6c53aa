"""The predict.post tables (HX:655-673: per draw and test site a predictive mean and variance) against an exact reference, at
EVERY (draw, site), on every piece of device code that computes them:

  kept factor   site_corr_kernel<K> + site_solve_kernel<NPF> (n <= 104, K <= 3, default options): one lane per site
  extra rows    the sites ride through the elimination as extra rows, in chunks of 30 (n <= 64) or 62 sites
  blocked       the sweep over materialised matrices with its predict tail, as phase launches or as one scheduled launch
  literal       ccgp_predict_post on the caller's R.Inv (predict_factors_kernel)
  factor set    ccgp_factor_batch + ccgp_predict_from_factorset

The reference is oracle.ccgp_oracle.predict_parts in long double (direct squared differences, hand-written Cholesky; held to
a 50-digit evaluation within band / 64 by tests/test_oracle.py).  Every entry must satisfy

    |mean - mean_ref| <= band_mean,   |var - var_ref| <= band_var,   |beta - beta_ref| <= band_beta

with the first-order bands of oracle.ccgp_oracle.predict_bands: for a bilinear form p'R^-1 q
    Q(p, q) = eta (|R^-1 p|' W |R^-1 q| + |R^-1 p|' |q| + |p|' |R^-1 q|),   eta = C eps (1 + rho),   W = |L| |L|',
    band_var  = sigma2 (Q(r, r) + 2 |u| Q(1, r) / s11 + u^2 Q(1, 1) / s11^2 + eps (1 + ww + u^2 / s11)),   u = 1 - z1w,
    band_beta = (Q(1, y - beta 1) + 2 |beta| Q(1, 1)) / s11 + eps sum_i |o_i y_i| / s11,
    band_mean = Q(r, y - beta 1) + (1 + |z1w|) band_beta + eps (|beta| + |r|' |g|).
rho is the size of the terms of the expanded exponent (oracle.expanded_form_magnitude; for a site's r the larger of the
design's and the site's own 2 sum_k theta_ck x_tk^2), as in tests/test_gpu_gradient_exact.py.  There is NO condition number
and NO floor: the variance cancels to zero at and near training points, where R^-1 r is a unit vector and the band is a few
eta sigma2 -- tests/test_oracle.py asserts band_var <= 1e-9 sigma2 at every site of the tables below that lies on a training
point or within 1e-6 of one, 100 times below the floor the tables were held to before.  A variance that comes back slightly
negative inside that band is correct behaviour (R's own arithmetic does the same).

The constant: C = oracle.ccgp_oracle.PREDICT_TOL_C = 128, the gradient band's.  Its yardstick is a plain fp64 restatement of
the device's own formula (oracle.predict_device_restatement: expanded exponents, L'DL'^T, forward substitutions, the three
dot products): over every case below its largest |fp64 - long double| / (band / C) is 0.55 (variance; mean 0.074, beta 0.022),
so C is 230 times that, where at least 8 times is asked for -- the margin for what the device does differently (FMA
contraction, another summation order, the 2-ulp polynomial exp, the reciprocal diagonal).  The same test of
tests/test_oracle.py asserts the factor of 8, and another that the band rejects six planted mistakes by a factor of 1e3.

Sites of a case (site_set): the training points 0, 7, 8 and n - 1, each of them moved by 1e-6 and by 1e-3 in one coordinate,
random interior sites up to m, one site at x = 50 * 1 -- where every correlation is below 1e-60 and, at all but the smallest
designs, underflows to zero: there mean == beta and var == sigma2 (1 + 1 / s11) to 4 ulp of the device's own beta and the
reference's s11 (whose own band is allowed for) -- and the training point n - 1 last: the last lane, the lone site of the last
chunk, the last row of an NPF instance.  S = 3 draws (oracle.conditioned_row, cond1 <= 1e8); at K = 3 the last draw's third
component has weight 1e-6.

Largest |device - reference| / (band / C) per route on an MI355X (test_zz_report_headroom prints them; C = 128 is the limit):
    route                             var     mean    beta
    kept factor                       0.39    0.067   0.032
    extra rows                        0.30    0.023   0.0087
    blocked sweep, phase launches     0.21    0.024   0.0049
    blocked sweep, scheduled launch   0.12    0.011   0.0024
    factor set                        0.12    0.011   0.0035
    literal (its own band)            22.9    0.074   --
No route left its band; no kernel was changed for this module.
"""
import numpy as np
import pytest

import route_witnesses
from oracle import ccgp_oracle as orc
from test_gpu_gradient_exact import EPS, KAPPA_MAX, LDS_LIMIT, _design, _timed, small_lds_bytes
from test_gpu_routes import assert_tier

S = 3
SIGMA2 = 1.3
C = orc.PREDICT_TOL_C
NEAR = 1e-6
MAX_RATIO = {}                        # route -> [var, mean, beta]: largest |dev - ref| / (band / C) seen


# ----------------------------------------------------------------------------- mirrors of the C++ route predicates
def _lds_fits(total, per_cu=1):
    """csrc/small_layout.h lds_fits (totals in doubles)."""
    return 8 * total <= 160 * 1024 // per_cu - 64


def _reg_lds_doubles(G, NB, NE, n, d, K):
    """csrc/small_layout.h RegCarve(G, NB, NE, inv = false, per_design = false, n, d, K).total, default build (no exp table)."""
    NP, XR, MPW = G * NB, G * NE, 256 // (G * G)
    per_mat = K * NP + K * d + K + 2 * (NP + XR) + NP + 2 * NP + 8 + (K * XR + 3 * XR * G if NE > 1 else 0)
    return d * n + MPW * per_mat + (d * XR if NE > 1 else 0)


def predict_route(n, d, K):
    """small_route(Op::Predict, gauss, n, d, K): 'r' = the register-resident evaluator, 'b' = the blocked sweep."""
    if n > 128 or small_lds_bytes(n, d, 1) > LDS_LIMIT:
        return "b"
    G = 8 if n <= 64 else 16
    return "r" if _lds_fits(_reg_lds_doubles(G, (n + G - 1) // G, 4, n, d, K)) else "b"


def kept_factor(n, d, K):
    """small_reg_sites_supported: the kept-factor scheme serves this shape (CCGP_OPT_PREDICT_FACTOR = 1, the default)."""
    if predict_route(n, d, K) != "r" or n > 104 or K > 3:
        return False
    npf = (n + 7) // 8 * 8
    solve = 8 + 3 * npf + 32 * (npf // 8) ** 2 + 8
    corr = (K * d + 7) // 8 * 8 + 8 + K * npf + K * d * npf + 4 * d * 64
    return _lds_fits(_reg_lds_doubles(8, (n + 7) // 8, 1, n, d, K)) and _lds_fits(solve, 2) and _lds_fits(corr, 2)


def extra_row_chunk(n):
    """sites per chunk of the extra-row scheme: G kPredictNE - 2"""
    return 30 if n <= 64 else 62


# ----------------------------------------------------------------------------- the case tables: (n, d, K, m[, ...])
# every value of NPF = 8 ceil(n / 8) (8 ... 104), the AHEAD switch between NPF = 56 and 64, both thread grids (n <= 64 and
# above); m: one lane, a full wave, the second wave, the second workgroup of four waves
KEPT_CASES = [(1, 2, 1, 1), (2, 4, 2, 64), (7, 9, 3, 65), (8, 2, 2, 257), (9, 4, 3, 64), (16, 9, 1, 65), (17, 2, 3, 257),
              (31, 4, 2, 1), (33, 9, 1, 64), (48, 2, 3, 65), (50, 4, 1, 257), (63, 9, 2, 64), (64, 2, 3, 65), (65, 4, 2, 257),
              (73, 9, 3, 1), (88, 2, 1, 64), (96, 4, 3, 65), (97, 9, 2, 257), (104, 9, 3, 257)]
# d = 1 with theta ~ n^2: rho ~ 1e4, the rho term of the band at work; interior and far sites only
HIGH_RHO_CASE = (40, 1, 2, 65)
# (n, d, K, m, CCGP_OPT_PREDICT_FACTOR): n > 104, K > 3, or the option; a full chunk, and a full chunk and one site
EXTRA_CASES = [(105, 2, 2, 62, 1), (105, 4, 3, 63, 1), (128, 9, 1, 62, 1), (128, 2, 3, 63, 1), (50, 4, 4, 30, 1),
               (50, 2, 4, 31, 1), (64, 4, 2, 30, 0), (64, 9, 2, 31, 0)]
# (n, d, K, m): one site, one full tile row of sites, a tile row and one site
BLOCKED_SHAPES = {129: (3, 2), 257: (2, 3), 385: (4, 1)}
BLOCKED_CASES = [(n, d, K, m) for n, (d, K) in BLOCKED_SHAPES.items() for m in (1, 128, 129)]
WITNESS_CASE = tuple(c[2:] for c in route_witnesses.WITNESSES[0] if c[:2] == ("predict", "b"))[0] + (3,)   # (108, 63, 1, 3)
SCHED_CASE = (257, 2, 3, 129)
FACTORSET_CASES = [(64, 2, 3, 65), (257, 2, 3, 129)]
LITERAL_CASES = [(14, 3, 2, 5), (100, 3, 2, 5)]


def all_table_cases():
    """(route, n, d, K, m, kind) of every case that goes through check_table, for the host tests of tests/test_oracle.py."""
    out = [("kept", n, d, K, m, "full") for n, d, K, m in KEPT_CASES]
    out.append(("kept",) + HIGH_RHO_CASE + ("plain",))
    out += [("extra", n, d, K, m, "full") for n, d, K, m, _ in EXTRA_CASES]
    out += [("blocked", n, d, K, m, "full") for n, d, K, m in BLOCKED_CASES]
    out.append(("blocked",) + WITNESS_CASE + ("plain",))
    return out


# ----------------------------------------------------------------------------- designs, draws, sites
def site_set(X, m, seed, kind="full"):
    """The m test sites of a case.  kind 'plain': random interior sites and the far site only (no cancellation).  'full':
    the training points 0, 7, 8, n - 1 (clipped to the design), each moved by 1e-6 and by 1e-3 in one coordinate, interior
    sites up to m, the far site, and the training point n - 1 last.  Where m is too small for all of them: the training
    point n - 1, a 1e-6 neighbour, a 1e-3 neighbour and an interior site, as many as fit, then the far site."""
    n, d = X.shape
    rng = np.random.default_rng(seed)
    far = np.full((1, d), 50.0)
    if kind == "plain":
        return np.vstack([rng.random((m - 1, d)), far])
    tp = sorted({0, min(7, n - 1), min(8, n - 1), n - 1})
    step = np.stack([np.eye(d)[i % d] for i in range(len(tp))])
    T, T6, T3 = X[tp], X[tp] + 1e-6 * step, X[tp] + 1e-3 * step
    full = 3 * len(tp) + 1
    if m >= full:
        return np.vstack([T[:-1], T6, T3, rng.random((m - full, d)), far, T[-1:]])
    short = np.vstack([T[-1:], T6[:1], T3[min(1, len(tp) - 1)][None], rng.random((1, d)), T[:1]])
    return short[:1] if m == 1 else np.vstack([short[:m - 1], far])


def near_training(X, Xt):
    """mask of the sites on a training point or within 1e-6 (in the largest coordinate difference) of one"""
    return np.array([np.abs(X - x).max(axis=1).min() <= 1.5 * NEAR for x in Xt])


def make_case(n, d, K, m, kind="full"):
    """(X, y, P[S, K + K d], Xt[m, d]) of a shape: one design and one set of draws per (n, d, K), whatever m."""
    X, y = _design(n, d, seed=9000 + 31 * n + d)
    rng = np.random.default_rng(7 * n + 64 * d + K)
    P = np.stack([orc.conditioned_row(X, K, d, rng, KAPPA_MAX)[0] for _ in range(S)])
    if K == 3:
        # the last draw: the rough component second, and a third component whose weight all but vanishes
        th = P[-1, K:].reshape(K, d).copy()
        P[-1, K:] = th[[0, 2, 1]].ravel()
        P[-1, 2] = 1e-6
    return X, y, P, site_set(X, m, seed=n + m, kind=kind)


_FACTORS = {}


def reference(X, y, row, K, Xt, sigma2):
    """(parts, bands, cond1(R)) of one draw in long double; the factorisation is shared between the site sets of a design."""
    key = hash((X.tobytes(), y.tobytes(), row.tobytes()))
    if key not in _FACTORS:
        f = orc.predict_factor(X, y, row, K, X.shape[1], np.longdouble)
        f["cond1"] = orc.cond1(f["R"], f["Rinv"])
        _FACTORS[key] = f
    f = _FACTORS[key]
    parts = orc.predict_parts(X, y, row, K, X.shape[1], sigma2, Xt, np.longdouble, factor=f)
    return parts, orc.predict_bands(parts, sigma2, C), f["cond1"]


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def check_table(X, y, K, P, Xt, sigma2, got, tag):
    """got = (mean[S, m], var[S, m], beta[S], status[S]) from the device: status 0 and every entry within its band; at a far
    site (every coordinate 50) mean == beta and var == sigma2 (1 + 1 / s11) to 4 ulp beside s11's own band."""
    mean, var, beta, st = got
    assert not np.asarray(st).any(), (tag, st)
    assert mean.shape == (len(P), len(Xt)) and var.shape == mean.shape
    far = np.nonzero((Xt == 50.0).all(axis=1))[0]
    worst = MAX_RATIO.setdefault(tag, [0.0, 0.0, 0.0])
    for s in range(len(P)):
        parts, band, kappa = reference(X, y, P[s], K, Xt, sigma2)
        assert kappa <= KAPPA_MAX, (tag, s, kappa)
        e_var = np.abs(var[s] - _f64(parts["var"]))
        e_mean = np.abs(mean[s] - _f64(parts["mean"]))
        e_beta = abs(beta[s] - float(parts["beta"]))
        worst[0] = max(worst[0], float((e_var / band["var"]).max()) * C)
        worst[1] = max(worst[1], float((e_mean / band["mean"]).max()) * C)
        worst[2] = max(worst[2], e_beta / band["beta"] * C)
        print("%s draw %d cond1 %.3g rho %.3g: var %.3g mean %.3g beta %.3g (x band / C)" % (
            tag, s, kappa, parts["rho"], (e_var / band["var"]).max() * C, (e_mean / band["mean"]).max() * C,
            e_beta / band["beta"] * C))
        for name, err, bnd, dev in (("var", e_var, band["var"], var[s]), ("mean", e_mean, band["mean"], mean[s])):
            bad = np.nonzero(~(err <= bnd))[0]
            assert bad.size == 0, (
                "%s draw %d: %s of sites %s is %s, off by %s bands (cond1 %.3g); reference there: %s ww %s z1w %s zyw %s s11 %.17g"
                % (tag, s, name, bad[:6], dev[bad[:6]], (err / bnd)[bad[:6]], kappa, _f64(parts[name])[bad[:6]],
                   _f64(parts["ww"])[bad[:6]], _f64(parts["z1w"])[bad[:6]], _f64(parts["zyw"])[bad[:6]], float(parts["s11"])))
        assert e_beta <= band["beta"], (tag, s, beta[s], float(parts["beta"]), band["beta"], kappa)
        for t in far:
            assert float(_f64(parts["r"])[t].max()) <= 1e-60
            assert abs(mean[s, t] - beta[s]) <= 4 * np.spacing(abs(beta[s])), (tag, s, t, mean[s, t], beta[s])
            s11 = float(parts["s11"])
            want = sigma2 * (1.0 + 1.0 / s11)
            assert abs(var[s, t] - want) <= 4 * np.spacing(want) + sigma2 * band["s11"] / s11 ** 2, (tag, s, t, var[s, t], want)


# ----------------------------------------------------------------------------- kept factor
@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K,m,kind", [c + ("full",) for c in KEPT_CASES] + [HIGH_RHO_CASE + ("plain",)])
def test_kept_factor_tables_exact(handle, n, d, K, m, kind):
    assert kept_factor(n, d, K)
    X, y, P, Xt = make_case(n, d, K, m, kind)
    got, t = _timed(handle, lambda: handle.predict_batch(X, y, K, P, Xt, SIGMA2))
    assert_tier(t, "r", n)
    check_table(X, y, K, P, Xt, SIGMA2, got, "kept")


# ----------------------------------------------------------------------------- extra rows
@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K,m,opt", EXTRA_CASES)
def test_extra_row_tables_exact(handle, n, d, K, m, opt):
    from ccgp_amd import api
    assert predict_route(n, d, K) == "r" and (opt == 0 or not kept_factor(n, d, K))
    X, y, P, Xt = make_case(n, d, K, m)
    handle.set_option(api.OPT_PREDICT_FACTOR, opt)
    try:
        got, t = _timed(handle, lambda: handle.predict_batch(X, y, K, P, Xt, SIGMA2))
    finally:
        handle.set_option(api.OPT_PREDICT_FACTOR, 1)
    assert_tier(t, "r", n)
    check_table(X, y, K, P, Xt, SIGMA2, got, "extra")


# ----------------------------------------------------------------------------- blocked sweep
@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K,m", BLOCKED_CASES)
def test_blocked_tables_exact(handle, n, d, K, m):
    assert predict_route(n, d, K) == "b"
    X, y, P, Xt = make_case(n, d, K, m)
    got, t = _timed(handle, lambda: handle.predict_batch(X, y, K, P, Xt, SIGMA2))
    assert_tier(t, "b", n)
    assert t["sweep"][1] == 0, t
    check_table(X, y, K, P, Xt, SIGMA2, got, "blocked")


@pytest.mark.gpu
def test_blocked_tables_exact_below_129(handle):
    """The n <= 128 shape whose prediction takes the sweep (tests/route_witnesses.py): d = 63, so interior and far sites."""
    n, d, K, m = WITNESS_CASE
    assert predict_route(n, d, K) == "b" and n <= 128
    X, y, P, Xt = make_case(n, d, K, m, "plain")
    got, t = _timed(handle, lambda: handle.predict_batch(X, y, K, P, Xt, SIGMA2))
    assert_tier(t, "b", n)
    check_table(X, y, K, P, Xt, SIGMA2, got, "blocked")


@pytest.mark.gpu
def test_scheduled_sweep_tables_exact(handle):
    """CCGP_OPT_SCHED = 1: the sweep and its extra tile rows as ONE scheduled launch (tests/test_gpu_sched.py runs this size)."""
    from ccgp_amd import api
    n, d, K, m = SCHED_CASE
    X, y, P, Xt = make_case(n, d, K, m)
    handle.set_option(api.OPT_SCHED, 1)
    try:
        got, t = _timed(handle, lambda: handle.predict_batch(X, y, K, P, Xt, SIGMA2))
    finally:
        handle.set_option(api.OPT_SCHED, 3)
    assert t["fused"][1] == 0 and t["sweep"][1] > 0, t
    check_table(X, y, K, P, Xt, SIGMA2, got, "sched")


# ----------------------------------------------------------------------------- factor set
@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K,m", FACTORSET_CASES)
def test_factor_set_tables_exact(handle, n, d, K, m):
    """tests/test_gpu_factorset.py holds the factor set bit-equal to predict_batch; this ties it to the reference directly."""
    X, y, P, Xt = make_case(n, d, K, m)

    def run():
        with handle.factor_batch(X, y, K, P, SIGMA2) as fs:
            mean, var = fs.predict(Xt)
            return mean, var, fs.beta, fs.status
    got, t = _timed(handle, run)
    assert_tier(t, predict_route(n, d, K), n)
    check_table(X, y, K, P, Xt, SIGMA2, got, "factorset")


# ----------------------------------------------------------------------------- literal predict.post
def literal_reference(X, row, K, sigma2, Xt, R_inv, beta, mf, v1, v2):
    """HX:667-670 on the caller's R.Inv and factors, in long double with r from direct squared differences:
    (mean, var, band_mean, band_var).  The band is the rounding of the sums alone: eta = C eps (1 + rho) times each sum's terms
    in absolute value (r's entries come out of the expanded exponent, and a sum of n products errs by at most n / 4 + 10 eps
    of that in the kernel's order), plus 4 eps of the last operations' operands."""
    ld = np.longdouble
    d = X.shape[1]
    w, Th = orc.unpack_params(row, K, d)
    r = sum(ld(w[c]) ** 2 * orc.cross_corr(Xt, X, Th[c], ld) for c in range(K)) / (np.asarray(w, dtype=ld) ** 2).sum()
    Ri, mfl, v1l = np.asarray(R_inv, dtype=ld), np.asarray(mf, dtype=ld), np.asarray(v1, dtype=ld)
    q = ((r @ Ri) * r).sum(axis=1)
    u = ld(1) - r @ v1l
    var = ld(sigma2) * (ld(1) - q + u * u / ld(v2))
    mean = ld(beta) + r @ mfl
    rho_t = 2.0 * ((Xt ** 2) @ np.asarray(Th).T).max(axis=1)
    eta = C * EPS * (1.0 + np.maximum(orc.expanded_form_magnitude(X, row, K, d), rho_t))
    ar = np.abs(_f64(r))
    bq = eta * ((ar @ np.abs(R_inv)) * ar).sum(axis=1)
    uf, qf = _f64(u), _f64(q)
    band_var = sigma2 * (bq + 2 * np.abs(uf) * eta * (ar @ np.abs(v1)) / v2 + 4 * EPS * (1 + np.abs(qf) + uf * uf / v2))
    band_mean = eta * (ar @ np.abs(mf)) + 4 * EPS * (abs(beta) + ar @ np.abs(mf))
    return _f64(mean), _f64(var), band_mean, band_var


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K,m", LITERAL_CASES)
def test_literal_predict_post_exact(handle, n, d, K, m):
    """ccgp_predict_post with the fp64 solve(R) of the oracle as R.Inv: only predict_factors_kernel (and the cross-correlation
    kernel in front of it) differs from the reference, which runs the same arithmetic on the same R.Inv."""
    X, y, P, Xt = make_case(n, d, K, m)
    worst = MAX_RATIO.setdefault("literal", [0.0, 0.0, 0.0])
    for s in range(S):
        w, Th = orc.unpack_params(P[s], K, d)
        R_inv = orc.solve_inverse(orc.mixed_corr_matrix_general(X, w, Th))
        beta = orc.beta_mle(R_inv, y)
        mf, v1, v2 = orc.factors(R_inv, beta, y)
        mean, var = handle.predict_post(Xt, X, K, P[s], beta, mf, v1, v2, R_inv, SIGMA2)
        want_mean, want_var, band_mean, band_var = literal_reference(X, P[s], K, SIGMA2, Xt, R_inv, beta, mf, v1, v2)
        worst[0] = max(worst[0], float((np.abs(var - want_var) / band_var).max()) * C)
        worst[1] = max(worst[1], float((np.abs(mean - want_mean) / band_mean).max()) * C)
        assert (np.abs(var - want_var) <= band_var).all(), (n, s, var, want_var, band_var)
        assert (np.abs(mean - want_mean) <= band_mean).all(), (n, s, mean, want_mean, band_mean)


# ----------------------------------------------------------------------------- the case tables themselves (host)
def test_case_table_reaches_every_site_solve_instance():
    """Host check of the lists above: the 13 instances of site_solve_kernel<NPF> and K = 1, 2, 3 of site_corr_kernel<K> occur
    among the kept-factor cases, the sizes the issue names are there, every case is on the route its test asserts, and each
    route's site counts straddle its chunk size."""
    kept = KEPT_CASES + [HIGH_RHO_CASE]
    assert {(n + 7) // 8 * 8 for n, _, _, _ in kept} >= set(range(8, 105, 8))
    assert {n for n, _, _, _ in KEPT_CASES} >= {1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 96, 97, 104}
    assert {K for _, _, K, _ in kept} == {1, 2, 3} and {d for _, d, _, _ in KEPT_CASES} == {2, 4, 9}
    assert {m for _, _, _, m in KEPT_CASES} == {1, 64, 65, 257}                 # 64 lanes a wave, 4 waves a workgroup
    assert all(kept_factor(n, d, K) for n, d, K, _ in kept)
    assert {n for n, _, _, _ in kept if n <= 64} and {n for n, _, _, _ in kept if n > 64}       # both thread grids
    # the mirror of small_route(Predict) against the witness of the check program: the first shape that takes the sweep
    wn, wd, wK = WITNESS_CASE[:3]
    assert predict_route(wn, wd, wK) == "b" and wn <= 128
    assert all(predict_route(n, d, K) == "r" for n in range(1, wn + 1) for d in range(1, 65) for K in range(1, 9)
               if (n, d, K) < (wn, wd, wK))
    for n, d, K, m, opt in EXTRA_CASES:
        assert predict_route(n, d, K) == "r" and (opt == 0 or not kept_factor(n, d, K)), (n, d, K)
    assert {(n, K) for n, _, K, _, opt in EXTRA_CASES if opt} >= {(50, 4)} and {n for n, _, _, _, opt in EXTRA_CASES if opt} >= {105, 128}
    assert (64, 2, 0) in {(n, K, opt) for n, _, K, _, opt in EXTRA_CASES}
    for chunk in (30, 62):
        ms = {m for n, _, _, m, _ in EXTRA_CASES if extra_row_chunk(n) == chunk}
        assert chunk in ms and chunk + 1 in ms, (chunk, ms)
    assert {m for _, _, _, m, _ in EXTRA_CASES} == {30, 31, 62, 63}
    assert {n for n, _, _, _ in BLOCKED_CASES} == {129, 257, 385}
    for n in BLOCKED_SHAPES:                                                    # 128 sites make one extra tile row
        assert {m for nn, _, _, m in BLOCKED_CASES if nn == n} == {1, 128, 129}
    assert all(predict_route(n, d, K) == "b" for n, d, K, _ in BLOCKED_CASES + [SCHED_CASE])
    assert WITNESS_CASE == (108, 63, 1, 3) and SCHED_CASE in BLOCKED_CASES
    assert {n for n, _, _, _ in FACTORSET_CASES} == {64, 257} and {n for n, _, _, _ in LITERAL_CASES} == {14, 100}
    # the site sets: training points, both neighbours, the far site, and the training point n - 1 last
    for n, d, K, m in [(104, 9, 3, 257), (8, 2, 2, 257), (2, 4, 2, 64), (105, 2, 2, 62), (64, 4, 2, 31)]:
        X = _design(n, d, seed=9000 + 31 * n + d)[0]
        Xt = site_set(X, m, seed=n + m)
        assert Xt.shape == (m, d) and (Xt[-1] == X[n - 1]).all() and (Xt[-2] == 50.0).all()
        dist = np.array([np.abs(X - x).max(axis=1).min() for x in Xt])
        k = len({0, min(7, n - 1), min(8, n - 1), n - 1})
        assert (dist == 0).sum() == k and (np.abs(dist - 1e-6) < 1e-12).sum() == k and (np.abs(dist - 1e-3) < 1e-12).sum() == k
        assert near_training(X, Xt).sum() == 2 * k


@pytest.mark.gpu
def test_zz_report_headroom():
    """Largest |device - reference| / (band / C) per route, for var, mean and beta: C = 128 is the limit."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-10s var %.3g  mean %.3g  beta %.3g" % ((k,) + tuple(MAX_RATIO[k])))
