"""tests/design_exact.py on the host: the long-double reference against mpmath, the case list against its routes and its
condition cap, the two fp64 LAPACK figures behind C_LD and C_G, and proof that the bands bite.  No GPU.

The planted mistakes (design_exact.fp64_restatement(mistake=...)) must each miss a band by at least 4 C on at least one
listed case.  One of them cannot, by construction: `diag_one`, the diagonal forced to exactly 1 where the expanded form gives
exp(-rounding).  The band grants every entry of R, the diagonal included, a relative error eps (1 + rho_aa), and rho_aa = 4
u_a is exactly the size of the terms whose rounding the expanded diagonal carries (|u_a + u_a - 2 u_a| <= eps rho_aa / 2): a
kernel that forces the diagonal moves each R_aa by less than half of what the band grants it.  It is asserted to stay INSIDE
the band (at most C units) on every case, so that the statement is checked and not merely made."""
import time

import numpy as np
import pytest

import design_exact as dx
import route_witnesses
from oracle import ccgp_oracle as orc
from test_gpu_failure_contract import _reg_lds_doubles8
from test_gpu_gradient_exact import KAPPA_MAX
from test_gpu_gradient_exact import small_reg_inverse_supported as inverse_supported_other
from test_gpu_predict_exact import _reg_lds_doubles

T_START = time.perf_counter()


# ----------------------------------------------------------------------------- routes
def test_carve_restatement_agrees_with_the_others_and_with_the_witnesses():
    for n in (1, 8, 9, 49, 64, 65, 100, 104, 105, 128):
        for d in (1, 2, 9, 33, 64):
            for K in (1, 3, 8):
                assert dx.reg_carve_total(8, (n + 7) // 8, 1, False, False, n, d, K) == _reg_lds_doubles8(n, d, K)
                assert dx.small_reg_inverse_supported(n, d, K) == inverse_supported_other(n, d, K)
                for G in (8, 16):
                    for NE in (1, 4):
                        NB = (n + G - 1) // G
                        assert dx.reg_carve_total(G, NB, NE, False, False, n, d, K) == _reg_lds_doubles(G, NB, NE, n, d, K)
    W = {(op, r): s for op, r, *s in route_witnesses.WITNESSES[0]}
    n, d, K = W[("design_grad", "u")]            # the smallest refused shape: n, then d, then K
    assert dx.design_grad_route(n, d, K) == "u" and dx.design_grad_route(n, d, K - 1) == "r"
    assert dx.design_grad_route(n, d - 1, 8) == "r" and dx.design_grad_route(n - 1, 64, 8) == "r"
    assert dx.design_grad_route(129, 1, 1) == "u" and dx.design_grad_route(128, 9, 3) == "r" and dx.design_grad_route(128, 9, 4) == "u"
    n, d, K = W[("logdet_designs", "b")]
    assert dx.logdet_route(n, d, K) == "b" and dx.logdet_route(n, d, K - 1) == "r"
    assert dx.logdet_route(n, d - 1, 8) == "r" and dx.logdet_route(n - 1, 64, 8) == "r"
    assert (n, d, K) == dx.LOGDET[12]


def test_case_list_reaches_what_it_is_aimed_at():
    for c in dx.grad_cases():
        assert dx.design_grad_route(c.n, c.d, c.K) == "r", c
    # every NB of dispatch_inv<3> at its first, last and one-past size
    ns = [n for n, _, _ in dx.INSTANCES]
    assert ns == [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128]
    for NB in range(1, 9):
        group = [(n, d, K) for n, d, K in dx.INSTANCES if (n + 15) // 16 == NB]
        assert any(d % 2 for _, d, _ in group) and any(K == 8 for _, _, K in group), NB
    # the dimension loop: one, two and three chunks (and more) with full and clamped last chunks; the second trip of pass 2
    assert {(d + 7) // 8 for _, d, _ in dx.CHUNKS} >= {1, 2, 3, 4, 5}
    assert {d for n, d, _ in dx.CHUNKS if n == 49} == {8, 9, 16, 17, 24, 25}
    assert len(dx.SECOND_TRIP) == 5 and all(n * ((d + 7) // 8) > 256 for n, d, _ in dx.SECOND_TRIP)
    assert any(K == 8 for _, _, K in dx.SECOND_TRIP)
    # n_fixed at 1, at odd and even rows, at a multiple of 16, at n < NP and n == NP
    assert [n for n, _, _ in dx.FIXED] == [33, 48]
    for n, _, _ in dx.FIXED:
        assert set(dx.fixed_values(n)) >= {0, 1, 2, 15, 16, 17, n - 2, n - 1}
    # every instance of the per-design log det
    assert [dx.logdet_instance(*s) for s in dx.LOGDET] == ["reg8"] * 6 + ["wave"] * 4 + ["reg16"] * 2 + ["blocked"] * 4
    assert [(s[0] + 7) // 8 for s in dx.LOGDET[6:10]] == [9, 9, 10, 13]
    # the batch positions: all four sub-matrix slots and a last workgroup that is not full
    assert max(dx.POSITION_B) % 4 != 0 and max(dx.POSITION_B) > 4
    assert [dx.logdet_instance(*s) for s in dx.POSITION] == ["reg8", "reg8", "reg8", "wave"]
    for c in dx.grad_cases():
        if c.cls == "dyadic":
            X, row = dx.case_inputs(c)
            th = row[c.K:]
            assert c.d <= 4 and (X * 64 == np.round(X * 64)).all() and np.abs(X).max() <= 1.0
            assert (np.log2(th) == np.round(np.log2(th))).all()
            assert all(len({tuple(p) for p in D}) == c.n for D in X)
        if c.cls == "position":
            X, _ = dx.case_inputs(c)
            assert all(len(np.unique(X[:, i, k])) == c.B for i in range(c.n) for k in range(c.d))


def test_every_case_is_inside_the_condition_cap():
    worst = (0.0, None)
    for c in dx.all_cases():
        for b in range(c.B):
            ref = dx.case_reference(c, b)
            assert ref.kappa <= KAPPA_MAX, (c, b, ref.kappa)
            assert np.isfinite(ref.ld) and ref.unit_ld >= 0.0
            worst = max(worst, (ref.kappa, (c, b)), key=lambda t: t[0])
    print("largest cond_1(R) of the case list: %.3g at %s" % worst)


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("n,d,K", [(5, 2, 2), (14, 2, 2), (21, 4, 3)])
def test_reference_matches_mpmath_at_50_digits(n, d, K):
    """The long-double reference spends at most 1 % of a unit (eps_longdouble / eps = 4.9e-4 per rounding)."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng([11, n, d, K])
    X = rng.uniform(-1.0, 1.0, (n, d))
    row, _ = orc.conditioned_row(X, K, d, rng, dx.KAPPA_DRAW)
    ref = dx.reference(X, row, K)

    def mpf(v):             # a long double as the sum of two doubles
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))
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
    assert abs(mpf(ref.ld) - mp.log(mp.det(R))) <= 0.01 * ref.unit_ld
    for i in range(n):
        for k in range(d):
            v = -4 * sum(A[i, j] * (Xm[i][k] - Xm[j][k]) * sum(w2[q] / sw * th[q][k] * Rq[q][i, j] for q in range(K))
                         for j in range(n) if j != i)
            assert abs(mpf(ref.g[i, k]) - v) <= 0.01 * ref.unit_g[i, k], (i, k)


# ----------------------------------------------------------------------------- the constants
def test_lapack_figures_have_not_moved():
    """The largest |fp64 - ref| / unit of the plain fp64 implementation over the whole case list: the figures recorded as
    oracle.DESIGN_LD_LAPACK_MAX and oracle.DESIGN_GRAD_LAPACK_MAX, from which C_LD and C_G follow."""
    top_ld, top_g = (0.0, None), (0.0, None)
    for c in dx.all_cases():
        designs, row = dx.case_inputs(c)
        for b in range(c.B):
            ref = dx.case_reference(c, b)
            ld, g = dx.fp64_restatement(designs[b], row, c.K)
            top_ld = max(top_ld, (dx.ratio_ld(ld, ref), (c, b)), key=lambda t: t[0])
            if ref.g is not None:
                top_g = max(top_g, (dx.ratio_g(g, ref), (c, b)), key=lambda t: t[0])
    print("fp64 LAPACK log det: %.4g units at %s; gradient: %.4g units at %s" % (top_ld + top_g))
    C_LD, C_G = dx.design_constants()
    assert (C_LD, C_G) == (8.0, 16.0)
    # the recorded maxima are this host's LAPACK and libm; another build's must still leave the factor 32 under the same C
    # (as tests/test_oracle.py holds MARGINAL_LAPACK_MAX), and a figure that fell by half means the case list has changed
    assert 32.0 * top_ld[0] <= C_LD and 0.5 * orc.DESIGN_LD_LAPACK_MAX <= top_ld[0], top_ld
    assert 32.0 * top_g[0] <= C_G and 0.5 * orc.DESIGN_GRAD_LAPACK_MAX <= top_g[0], top_g


# ----------------------------------------------------------------------------- the bands bite
def _misses(mistake):
    """[(case, b, n_fixed, miss_ld / C_LD, miss_g / C_G)] of a planted mistake over the cases it can show on."""
    C_LD, C_G = dx.design_constants()
    out = []
    for c in dx.grad_cases():
        designs, row = dx.case_inputs(c)
        if c.n < 3 or (mistake == "theta_next" and c.K < 2):
            continue
        if (mistake == "next_row") != (c.cls == "position") or (mistake == "nfixed_row") != (c.cls == "fixed"):
            continue
        for b in range(min(c.B - 1, 3)):
            ref = dx.case_reference(c, b)
            for nf in (dx.fixed_values(c.n)[1:] if mistake == "nfixed_row" else [0]):
                ld, g = dx.fp64_restatement(designs[b], row, c.K, nf, mistake, designs[b + 1])
                out.append((c, b, nf, dx.ratio_ld(ld, ref) / C_LD, dx.ratio_g(g, ref, nf) / C_G))
    return out


@pytest.mark.parametrize("mistake,hits_ld", [("next_row", True), ("drop_sub", False), ("drop_i2", False), ("no_sw", False),
                                             ("w_unsquared", False), ("theta_next", False), ("trail_chunk", False),
                                             ("nfixed_row", False), ("ld_short", True), ("drop_small", True)])
def test_bands_reject_a_planted_mistake(mistake, hits_ld):
    res = _misses(mistake)
    col = 3 if mistake in ("ld_short", "drop_small") else 4
    worst = max(res, key=lambda r: r[col])
    caught = sum(r[col] >= 4.0 for r in res)
    print("%s: missed by %.3g C at %s (design %d, n_fixed %d); by >= 4 C on %d of %d" % (
        mistake, worst[col], worst[0], worst[1], worst[2], caught, len(res)))
    assert worst[col] >= 4.0
    if hits_ld:
        assert max(r[3] for r in res) >= 4.0
    if mistake in ("next_row", "nfixed_row", "ld_short", "no_sw", "w_unsquared"):
        assert caught == len(res)          # these show on every design they are planted in
    if mistake not in ("next_row", "ld_short", "drop_small"):
        assert max(r[3] for r in res) <= 1.0       # the log det is untouched by a mistake of the gradient alone


def test_forced_unit_diagonal_is_inside_the_band_by_construction():
    """Module docstring: the band grants the diagonal what the expanded form's rounding is."""
    res = _misses("diag_one")
    assert res and max(r[3] for r in res) <= 1.0 and max(r[4] for r in res) <= 1.0
    print("diag_one: at most %.3g C_LD and %.3g C_G" % (max(r[3] for r in res), max(r[4] for r in res)))


def test_zz_reference_seconds():
    print("references: %.2f s of host time; module: %.2f s" % (dx.REFERENCE_SECONDS[0], time.perf_counter() - T_START))
    assert dx.REFERENCE_SECONDS[0] <= dx.REFERENCE_SECONDS_MAX
