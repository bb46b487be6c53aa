"""Exact references and condition-free bands for the CGP comparator (cgp_state_kernel and cgp_predict_kernel of csrc/cgp.hip,
out of ccgp_cgp_state_batch, ccgp_cgp_predict and their sets forms).  Shared by tests/test_cgp_exact_host.py (the kernels'
arithmetic restated in numpy, no GPU) and tests/test_gpu_cgp_exact.py.  Conventions of tests/gauss_exact.py: fp64 inputs are exact
rationals, references are mpmath at DPS = 40 digits, and NOTHING IN A BAND COMES FROM A DEVICE RUN: every constant below is
counted from the operations of cgp.hip.  The vectors inside a band need two digits and are numpy fp64.

What is held.  Handle.cgp_predict returns keep = dict(s, res2, temp, sf, beta, tau2).  From the device's own s the fifth matrix

    Q = G + lambda diag(sqrt s) L diag(sqrt s)

is known exactly, so beta, temp, tau2, val and the six predict.CGP columns are held to identities whose bands are the backward
error of the operations performed -- no cond1(Q) anywhere.  u = 2^-53, gamma_k = k u / (1 - k u).

(a) Entries.  G, L, Gbw and the site vectors g, l, gbw: exp(-arg) with arg = sum_k rate_k (x_ik - x_jk)^2 an exact integer ratio
    (gauss_exact's integers), one 40-digit exp per distinct argument.  Relative band of an entry

        eps = expm1((d + 4) u arg) + 4 u          (+ 2 quanta absolute where the reference is below 2.3e-308)

    cgp_dist: df rounds once, df df once more (3 u on the square), then d fused multiply-adds over positive terms: (d + 3) u on the
    argument.  Gbw's rate is theta_k bw, rounded once before the sum in cgp_state_kernel (tb), and the whole sum times bw, rounded
    once after it, in cgp_predict_kernel: one more u either way, so (d + 4) u covers both orders (and is used for G and L too).
    4 u: two ulp of the exponential, as gauss_exact holds exp_cov; exp_cov_poly is the device library's exp, documented at 1 ulp.

(b) Reweighting.  sn = (Gbw res2) / (Gbw 1), sf = mean(sn), s = sn / sf from the kept res2 as exact input.  All terms positive,
    so the bands are relative: for row i the eps-weighted means of numerator and denominator, plus 9 u for each wave sum (two
    terms a lane, a 6-level shuffle tree, one rounding of the term) and u for the quotient; sf adds the sn-weighted mean of those,
    9 u for its sum and u for the division by n; s_i adds both and u.

(c) Fifth solve, a posteriori.  r = Q temp - (y - beta 1) and 1'temp, with Q exact from the kept s, against

        band_r  = gamma_(3n+6) M W + E W + u (|y| + |beta|),    M = |L||D||L'|,  W = |Q^-1 y| + |beta| |Q^-1 1|
        band_1t = |Q^-1 1|' band_r + |Q^-1 1|' (gamma_(3n+6) M + E) W + 12 u (sum_k |z1_k zy_k| / d_k + |beta| 1'Q^-1 1)

    M from the 40-digit factor of Q, E the entry bands of Q: g eps_g + lambda sqrt(s_i s_j) l (eps_l + 4 u) + u |q_ij| (sqrt s_i,
    sqrt s_j, two products, the final fused multiply-add); on the diagonal 3 u lambda s_i + u q_ii.  3n + 6: the column-oriented
    elimination puts at most n - 1 fused multiply-adds and the two roundings of l_jk = c_jk (1 / d_k) on an entry (n + 1); the two
    extra rows are entries of that elimination (the forward substitution, n + 1); r = zy - beta z1 rounds twice, r (1 / d) twice,
    and the back substitution applies c (1 / d) (two roundings) in n - 1 fused multiply-adds (n + 4).  The back substitution runs
    on the COMBINED r, the forward ones on y and 1 apart, hence W and not |temp|.  1'temp = (s1y - beta s11) + (Q^-1 1)' r: the
    second term is band_r's, the first is the error of the device's beta = s1y / s11, two D-weighted wave sums (4 roundings a term,
    7 levels) of the forward-substituted rows.  The two identities together determine (beta, temp).

(d) tau2.  The device forms quad / n with quad = sum_k r_k^2 / d_k in the factor's basis, not (y - beta)'temp / n.  Reference:
    (y - beta_dev 1)' Q^-1 (y - beta_dev 1) / n.  Band: (2 |temp|' (gamma_(3n+6) M + E) W + 12 u quad) / n + u tau2 -- the backward
    error of the quadratic form (first order: 2 temp' dQ-like terms against W), its wave sum, the division.

(e) val.  val - n log(tau2_dev) against log det Q(s_dev) = sum log d_k of the 40-digit factor.  Band, first order:
    sum_ij |Q^-1|_ij (gamma_(n+1) M + E)_ij + 10 u sum |log d_k| + 3 u n |log tau2| + 2 u |val|.  The first term is the
    determinant's own sensitivity to the factorisation's backward error -- it is what log det can be known to, and is stated as
    such; the rest are the n logs (1 ulp each), their wave sum, n log tau2 and the last sum.

(f) predict.CGP from the kept state as exact input.  v: ratio of positive sums, relative band rel_v = eps-weighted means + 18 u.
    dq_j = g_j eps_g + lambda sqrt(v) sqrt(s_j) l_j (eps_l + rel_v / 2 + 4 u) + u |q_j| on the entries of q.  Yp, gp, lp:
    sum_j |temp_j| dq_j + 10 u (|beta| + sum |term|).  ppp = 1 + lambda v - q'Q^-1 q + (1 - q'Q^-1 1)^2 / 1'Q^-1 1 with the exact
    Q^-1 1 and 1'Q^-1 1 of Q(s_dev); its band is ABSOLUTE, with w = Q^-1 q, x1 = Q^-1 1, B = gamma_(3n+6) M + E:

        lambda v rel_v + 2 u (1 + lambda v)  +  2 |w|' dq + |w|' B |w|                                          (q'Q^-1 q)
        + 2 |1 - qu| D / s11 + (1 - qu)^2 (|x1|' B |x1| + 11 u s11) / s11^2 + 3 u (1 - qu)^2 / s11,
              D = |w|' B |x1| + |x1|' dq + 9 u sum |q_j x1_j| + u (1 + |qu|)                                    (the kept u, s11)
        + 3 u (1 + lambda v + q'Q^-1 q + (1 - qu)^2 / s11)

    the backward error of the forward substitution through the kept factor (n fused multiply-adds, the kept l rounded once
    more, the n-term sum of z_k^2 (1 / d_k): within 3n + 6) and of the kept u and s11.  The interval is held through tau2 ppp:
    ((Y_up - Yp) / 1.96)^2 and ((Yp - Y_low) / 1.96)^2 against tau2_dev ppp, band tau2 (dppp + 8 u (ppp + dppp)) plus the rounding
    of Yp +- half.  A site ON a training point has ppp = 0 exactly and Yp = y_i + r_i: both are held.

(g) A diagonal closed form: LatticeCase below.
"""
import functools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

import cgp_ref
import gauss_exact as gx

DPS = 40
U = 2.0 ** -53
QUANTUM, TINY = gx.QUANTUM, gx.TINY
COLS = cgp_ref.COLS


def gamma(k):
    return k * U / (1.0 - k * U)


def _mpf(v):
    return mp.mpf(float(v))


def _mpv(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


def _fl(v):
    return np.array([float(x) for x in v])


def split_row(row, d):
    row = np.asarray(row, dtype=np.float64).ravel()
    assert row.shape[0] == 2 * d + 2
    return float(row[0]), row[1:1 + d], row[1 + d:1 + 2 * d], float(row[1 + 2 * d])


# ----------------------------------------------------------------------------- (a) entries
def entries(XA, XB, rate, factor=1.0, symmetric=False):
    """(ref: [m][n] mpf, eps: [m, n] relative band, tiny: [m, n] bool) of exp(-sum_k rate_k factor (a_ik - b_jk)^2): the product
    rate_k factor is taken exactly."""
    XA, XB, rate = np.asarray(XA, dtype=np.float64), np.asarray(XB, dtype=np.float64), np.asarray(rate, dtype=np.float64)
    (m, d), n = XA.shape, XB.shape[0]
    sx, sr, sf = gx._scale(XA, XB), gx._scale(rate), gx._scale([factor])
    A, B = gx._ints(XA, sx), gx._ints(XB, sx)
    R = gx._ints(rate, sr) * int(gx._ints([factor], sf)[0])
    D = A[:, None, :] - B[None, :, :]
    args = np.dot(D * D, R)
    shift = 2 * sx + sr + sf
    ref = [[None] * n for _ in range(m)]
    argf = np.zeros((m, n))
    tiny = np.zeros((m, n), dtype=bool)
    with mp.workdps(DPS):
        for i in range(m):
            for j in range(i + 1 if symmetric else n):
                a = args[i, j]
                e = gx.exp_neg(a, shift)
                ref[i][j] = e
                argf[i, j] = math.ldexp(float(a), -shift)
                tiny[i, j] = e < TINY
                if symmetric:
                    ref[j][i], argf[j, i], tiny[j, i] = e, argf[i, j], tiny[i, j]
    with np.errstate(over="ignore"):
        eps = np.expm1((d + 4) * U * argf) + 4.0 * U
    return ref, eps, tiny


def _float_rows(ref):
    return np.array([[float(v) for v in row] for row in ref])


# ----------------------------------------------------------------------------- 40-digit L D L'
def mp_ldl(Q):
    """Q (full rows of mpf, symmetric positive definite) -> (L: rows of the unit lower factor below the diagonal, d)"""
    n = len(Q)
    Lr, dv = [[] for _ in range(n)], []
    with mp.workdps(DPS):
        for j in range(n):
            v = [Lr[j][k] * dv[k] for k in range(j)]
            dj = Q[j][j] - mp.fdot(Lr[j], v)
            assert dj > 0
            dv.append(dj)
            for i in range(j + 1, n):
                Lr[i].append((Q[i][j] - mp.fdot(Lr[i][:j], v)) / dj)
    return Lr, dv


def mp_forward(Lr, b):
    z = []
    for i, bi in enumerate(b):
        z.append(bi - mp.fdot(Lr[i], z))
    return z


def mp_backward(Lr, z):
    n = len(z)
    x = list(z)
    for k in range(n - 1, 0, -1):
        xk, row = x[k], Lr[k]
        for i in range(k):
            x[i] -= row[i] * xk
    return x


def mp_solve(Lr, dv, b):
    with mp.workdps(DPS):
        z = mp_forward(Lr, b)
        return mp_backward(Lr, [zi / di for zi, di in zip(z, dv)]), z


class Tally:
    """largest fraction of each band used"""

    def __init__(self):
        self.frac = {}

    def add(self, key, value):
        value = float(value)
        if value != value:
            value = math.inf
        self.frac[key] = max(self.frac.get(key, 0.0), value)

    def merge(self, other):
        for k, v in other.frac.items():
            self.add(k, v)

    def worst(self):
        return max(self.frac.values()) if self.frac else 0.0

    def outside(self, limit=1.0):
        return {k: v for k, v in self.frac.items() if not v <= limit}

    def __str__(self):
        return ", ".join("%s %.2g" % kv for kv in sorted(self.frac.items()))


def _ratio(err, band):
    err, band = float(err), float(band)
    if band > 0:
        return err / band
    return 0.0 if err == 0 else math.inf


# ----------------------------------------------------------------------------- (b) - (f): one evaluation
class Posterior:
    """Everything known exactly about one evaluation from the device's kept state: X, y the design of the evaluation (a held-out
    row already deleted), row the parameter row, keep the dict of Handle.cgp_predict."""

    def __init__(self, X, y, row, keep):
        self.X, self.y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
        self.n, self.d = self.X.shape
        self.row = np.asarray(row, dtype=np.float64).ravel()
        self.lam, self.theta, self.alpha, self.bw = split_row(row, self.d)
        self.keep = keep
        n, lam = self.n, self.lam
        s = np.asarray(keep["s"], dtype=np.float64)
        assert s.shape == (n,) and np.all(s > 0)
        self.beta = float(keep["beta"])
        with mp.workdps(DPS):
            G, eg, tg = entries(self.X, self.X, self.theta, symmetric=True)
            Lc, el, tl = entries(self.X, self.X, self.alpha, symmetric=True)
            rs = [mp.sqrt(_mpf(v)) for v in s]
            lm = _mpf(lam)
            self.Q = [[G[i][j] + lm * rs[i] * Lc[i][j] * rs[j] for j in range(n)] for i in range(n)]
            self.Lr, self.dv = mp_ldl(self.Q)
            self.ym = _mpv(self.y)
            self.xy, self.zy = mp_solve(self.Lr, self.dv, self.ym)
            self.x1, self.z1 = mp_solve(self.Lr, self.dv, [mp.mpf(1)] * n)
            self.s11 = mp.fsum(self.x1)
            self.logdet = mp.fsum(mp.log(v) for v in self.dv)
        # the vectors of the bands, fp64
        Gf, Lf = _float_rows(G), _float_rows(Lc)
        rsf = np.sqrt(s)
        self.rsf = rsf
        lsl = lam * np.outer(rsf, rsf) * Lf
        self.Qf = Gf + lsl
        E = Gf * eg + lsl * (el + 4 * U) + U * np.abs(self.Qf) + 2 * QUANTUM * (tg + lam * np.outer(rsf, rsf) * tl)
        E[np.diag_indices(n)] = 3 * U * lam * s + U * np.diag(self.Qf)
        self.E = E
        Lm = np.eye(n)
        for i in range(n):
            Lm[i, :i] = [float(v) for v in self.Lr[i]]
        self.df = _fl(self.dv)
        self.M = np.abs(Lm) @ (self.df[:, None] * np.abs(Lm).T)
        self.B = gamma(3 * n + 6) * self.M + E
        self.xyf, self.x1f = _fl(self.xy), _fl(self.x1)
        self.W = np.abs(self.xyf) + abs(self.beta) * np.abs(self.x1f)
        self.band_r = self.B @ self.W + U * (np.abs(self.y) + abs(self.beta))
        self.s11f = float(self.s11)

    def cond1(self):
        return float(np.linalg.cond(self.Qf, 1))

    # ---- (b)
    def check_weights(self, t):
        n, keep = self.n, self.keep
        res2 = np.asarray(keep["res2"], dtype=np.float64)
        with mp.workdps(DPS):
            Gb, eb, tb = entries(self.X, self.X, self.theta, self.bw, symmetric=True)
            r2 = _mpv(res2)
            num = [mp.fdot(Gb[i], r2) for i in range(n)]
            den = [mp.fsum(Gb[i]) for i in range(n)]
            sn = [a / b for a, b in zip(num, den)]
            sf = mp.fsum(sn) / n
            s_ref = [v / sf for v in sn]
            Gbf = _float_rows(Gb)
            numf, denf, snf = _fl(num), _fl(den), _fl(sn)
            rel = ((Gbf * eb) @ res2 + 2 * QUANTUM * (tb @ res2)) / numf + ((Gbf * eb).sum(1) + 2 * QUANTUM * tb.sum(1)) / denf + 19 * U
            rel_sf = float(snf @ rel) / float(snf.sum()) + 10 * U
            t.add("sf", _ratio(abs(_mpf(keep["sf"]) - sf), rel_sf * float(sf)))
            for i in range(n):
                t.add("s", _ratio(abs(_mpf(keep["s"][i]) - s_ref[i]), (rel[i] + rel_sf + U) * float(s_ref[i])))

    # ---- (c)
    def check_solve(self, t):
        n = self.n
        temp = np.asarray(self.keep["temp"], dtype=np.float64)
        with mp.workdps(DPS):
            tm, bm = _mpv(temp), _mpf(self.beta)
            self.resid = [mp.fdot(self.Q[i], tm) - (self.ym[i] - bm) for i in range(n)]
            for i in range(n):
                t.add("resid", _ratio(abs(self.resid[i]), self.band_r[i]))
            one_t = mp.fsum(tm)
            zz = float(mp.fsum(abs(a * b) / c for a, b, c in zip(self.z1, self.zy, self.dv)))
            ax1 = np.abs(self.x1f)
            band = float(ax1 @ self.band_r) + float(ax1 @ (self.B @ self.W)) + 12 * U * (zz + abs(self.beta) * self.s11f)
            t.add("1'temp", _ratio(abs(one_t), band))

    # ---- (d)
    def check_tau2(self, t, tau2=None):
        n = self.n
        tau2 = float(self.keep["tau2"] if tau2 is None else tau2)
        temp = np.abs(np.asarray(self.keep["temp"], dtype=np.float64))
        with mp.workdps(DPS):
            bm = _mpf(self.beta)
            x = [a - bm * b for a, b in zip(self.xy, self.x1)]
            quad = mp.fdot(self.ym, x) - bm * mp.fsum(x)
            ref = quad / n
            band = (2.0 * float(temp @ (self.B @ self.W)) + 12 * U * float(quad)) / n + U * float(ref)
            t.add("tau2", _ratio(abs(_mpf(tau2) - ref), band))

    # ---- (e)
    def check_val(self, t, val):
        n = self.n
        tau2 = float(self.keep["tau2"])
        Qinv = np.abs(np.linalg.inv(self.Qf))
        with mp.workdps(DPS):
            got = _mpf(val) - n * mp.log(_mpf(tau2))
            band = (float((Qinv * (gamma(n + 1) * self.M + self.E)).sum()) + 10 * U * float(np.abs(np.log(self.df)).sum())
                    + 3 * U * n * abs(math.log(tau2)) + 2 * U * abs(float(val)))
            t.add("val", _ratio(abs(got - self.logdet), band))

    # ---- (f)
    def site_terms(self, Xt):
        """per site the exact v, q, w = Q^-1 q, ppp and every band (dict of lists / arrays)"""
        Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, self.d)
        m, n, lam, keep = Xt.shape[0], self.n, self.lam, self.keep
        res2, temp = np.asarray(keep["res2"], dtype=np.float64), np.asarray(keep["temp"], dtype=np.float64)
        sf, beta = float(keep["sf"]), self.beta
        out = []
        with mp.workdps(DPS):
            g, eg, tg = entries(Xt, self.X, self.theta)
            l, el, tl = entries(Xt, self.X, self.alpha)
            gb, eb, tb = entries(Xt, self.X, self.theta, self.bw)
            r2, tm, bm, lm = _mpv(res2), _mpv(temp), _mpf(beta), _mpf(lam)
            rs = [mp.sqrt(_mpf(v)) for v in keep["s"]]
            ax1, at = np.abs(self.x1f), np.abs(temp)
            for a in range(m):
                gbf, gf = _fl(gb[a]), _fl(g[a])
                num, den = mp.fdot(gb[a], r2), mp.fsum(gb[a])
                if den == 0:
                    out.append(None)                     # every gbw is 0: 0 / 0
                    continue
                v = (num / den) / _mpf(sf)
                vf = float(v)
                rel_v = ((float((gbf * eb[a]) @ res2) + 2 * QUANTUM * float(tb[a] @ res2)) / float(num) if num > 0 else 0.0) \
                    + (float(gbf @ eb[a]) + 2 * QUANTUM * float(tb[a].sum())) / float(den) + 18 * U
                lsv = lm * mp.sqrt(v)
                ls = [l[a][j] * rs[j] for j in range(n)]
                q = [g[a][j] + lsv * ls[j] for j in range(n)]
                lsf = float(lsv) * _fl(ls)
                qf = gf + lsf
                dq = gf * eg[a] + lsf * (el[a] + 0.5 * rel_v + 4 * U) + U * np.abs(qf) + 2 * QUANTUM * (tg[a] + tl[a])
                Yp = bm + mp.fdot(q, tm)
                gp = bm + mp.fdot(g[a], tm)
                lp = lsv * mp.fdot(ls, tm)
                bYp = float(at @ dq) + 10 * U * (abs(beta) + float(np.abs(qf * temp).sum()))
                bgp = float(at @ (gf * eg[a] + 2 * QUANTUM * tg[a])) + 10 * U * (abs(beta) + float(np.abs(gf * temp).sum()))
                blp = float(at @ (lsf * (el[a] + 0.5 * rel_v + 4 * U) + 2 * QUANTUM * tl[a])) + 10 * U * float(np.abs(lsf * temp).sum())
                w, _ = mp_solve(self.Lr, self.dv, q)
                wf = np.abs(_fl(w))
                qq, qu = mp.fdot(q, w), mp.fdot(q, self.x1)
                w1 = 1 - qu
                ppp = (1 + lm * v - qq) + w1 * w1 / self.s11
                lv, qqf, w1f, s11 = lam * vf, float(qq), abs(float(w1)), self.s11f
                D = float(wf @ (self.B @ ax1)) + float(ax1 @ dq) + 9 * U * float(np.abs(qf * self.x1f).sum()) + U * (1 + abs(float(qu)))
                dppp = (lv * rel_v + 2 * U * (1 + lv) + 2 * float(wf @ dq) + float(wf @ (self.B @ wf))
                        + 2 * w1f * D / s11 + w1f ** 2 * (float(ax1 @ (self.B @ ax1)) + 11 * U * s11) / s11 ** 2 + 3 * U * w1f ** 2 / s11
                        + 3 * U * (1 + lv + qqf + w1f ** 2 / s11))
                out.append(dict(v=v, rel_v=rel_v, Yp=Yp, gp=gp, lp=lp, bYp=bYp, bgp=bgp, blp=blp, ppp=ppp, dppp=dppp))
        return out

    def check_predict(self, t, Xt, out, on_training=None):
        """out: the device's [m, 6]; on_training: {site index: design row} of the sites that ARE training points.  Returns the
        sites whose v is 0 / 0 (the caller holds their NaN pattern)."""
        out = np.asarray(out, dtype=np.float64)
        tau2 = float(self.keep["tau2"])
        nan_sites = []
        with mp.workdps(DPS):
            c196 = mp.mpf(1.96)
            for a, st in enumerate(self.site_terms(Xt)):
                if st is None:
                    nan_sites.append(a)
                    continue
                Yp, gp, lp, v, lo, up = (_mpf(x) for x in out[a])
                t.add("v", _ratio(abs(v - st["v"]), st["rel_v"] * float(st["v"])))
                t.add("Yp", _ratio(abs(Yp - st["Yp"]), st["bYp"]))
                t.add("gp", _ratio(abs(gp - st["gp"]), st["bgp"]))
                t.add("lp", _ratio(abs(lp - st["lp"]), st["blp"]))
                ymax = float(np.abs(out[a, [0, 4, 5]]).max())
                want = _mpf(tau2) * st["ppp"]
                for key, h in (("Y_up", up - Yp), ("Y_low", Yp - lo)):
                    hs = h / c196
                    band = tau2 * (st["dppp"] + 8 * U * (abs(float(st["ppp"])) + st["dppp"])) \
                        + 2 * abs(float(hs)) * U * ymax / 1.96 + (U * ymax / 1.96) ** 2
                    t.add(key, _ratio(abs(hs * hs - want), band) if h >= 0 else math.inf)
                if on_training and a in on_training:
                    i = on_training[a]
                    # v = s_i and q = Q e_i there, so the exact ppp is 0 to second order in the roundings of the kept s_i: a
                    # kept state whose s, res2 and sf do not belong together fails here
                    t.add("ppp = 0 on y_i", 0.0 if abs(float(st["ppp"])) <= 1e-20 else math.inf)
                    t.add("Yp on y_i", _ratio(abs(Yp - self.ym[i]), self.band_r[i] + st["bYp"]))
        return nan_sites


def check_evaluation(X, y, row, keep, val=None, Xt=None, out=None, on_training=None, logdet=True):
    """checks (b) - (f) of one evaluation -> (Tally, Posterior, sites with 0 / 0)"""
    t = Tally()
    p = Posterior(X, y, row, keep)
    p.check_weights(t)
    p.check_solve(t)
    p.check_tau2(t)
    if val is not None and logdet:
        p.check_val(t, val)
    nan_sites = p.check_predict(t, Xt, out, on_training) if Xt is not None else []
    return t, p, nan_sites


def loo_check(t, p, x0, loo):
    """the jackknife's prediction of the held-out point x0 against band (f)'s Yp formula from the deleted design's Posterior p"""
    st = p.site_terms(np.asarray(x0, dtype=np.float64)[None])[0]
    with mp.workdps(DPS):
        t.add("loo", _ratio(abs(_mpf(loo) - st["Yp"]), st["bYp"]))


# ----------------------------------------------------------------------------- the kernels restated
def _tree(v):
    """cgp_wave_sum on [..., 64]"""
    v = np.array(v, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :64 - off] = v[..., :64 - off] + v[..., off:64]
    return v[..., 0]


def _lanes(P):
    """the lane accumulators acc = term + acc over j = lane, lane + 64 of [..., n <= 128] -> [..., 64]"""
    n = P.shape[-1]
    a = np.zeros(P.shape[:-1] + (128,))
    a[..., :n] = P
    return a[..., 64:] + (a[..., :64] + 0.0)


def _wsum(P):
    return _tree(_lanes(np.asarray(P, dtype=np.float64)))


def _dist(A, B, rate):
    s = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        df = A[:, None, k] - B[None, :, k]
        s = (df * df) * rate[k] + s
    return s


PLANTS = ("s_prev", "sf_prev", "tau2_n0", "temp_1e-10", "rinv_1e-12", "exp_1e-13", "qq_dnext")


def restate(X, y, row, skip=-1, Xt=None, plant=None, gbw_order="state"):
    """cgp_state_kernel (and cgp_predict_kernel at the sites Xt) in numpy fp64 in the kernel's operation order, without fused
    multiply-adds and with numpy's exp -> dict(val, beta, tau2, loo, status, keep, out).  plant: one of PLANTS, a mistake the
    bands must reject.  gbw_order 'predict': the state's Gbw from (sum theta df^2) bw, the other order band (a) covers."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
    n0, d = X.shape
    lam, th, al, bw = split_row(row, d)
    x0 = None
    if skip >= 0:
        pick = np.arange(n0) != skip
        x0, X, y = X[skip], X[pick], y[pick]
    n = X.shape[0]
    ex = (lambda a: np.exp(-a) * (1 + 1e-13)) if plant == "exp_1e-13" else (lambda a: np.exp(-a))
    tb = th * bw
    with np.errstate(all="ignore"):
        G, Lc = ex(_dist(X, X, th)), ex(_dist(X, X, al))
        Gbw = ex(_dist(X, X, tb)) if gbw_order == "state" else ex(_dist(X, X, th) * bw)
        G1 = G.copy()
        G1[np.diag_indices(n)] = 1.0
        s, rs = np.ones(n), np.ones(n)
        sf = e2 = None
        sf_hist, s_hist = [], []
        for rep in range(5):
            A = np.zeros((n + 2, n))
            A[:n] = lam * ((rs[:, None] * Lc) * rs[None, :]) + G
            A[np.arange(n), np.arange(n)] = lam * (rs * rs) + 1.0
            A[n], A[n + 1] = y, 1.0
            for k in range(n):
                piv = A[k, k]
                if not piv > n * cgp_ref.EPS:
                    return dict(status=k + 1)
                rinv = 1.0 / piv
                if plant == "rinv_1e-12" and k == 0 and rep == 4:
                    rinv *= 1 + 1e-12
                ljk = A[k + 1:n, k] * rinv
                A[k + 1:, k + 1:] = A[k + 1:, k + 1:] + (-A[k + 1:, k])[:, None] * ljk[None, :]
            dg = np.diag(A[:n]).copy()
            rd = 1.0 / dg
            zy, z1 = A[n].copy(), A[n + 1].copy()
            s11 = _wsum((z1 * z1) * rd)
            s1y = _wsum((z1 * zy) * rd)
            beta = s1y / s11
            r = zy - beta * z1
            quad = _wsum((r * r) * rd)
            logdet = _wsum(np.log(dg))
            tv, uv = r * rd, z1 * rd
            for k in range(n - 1, 0, -1):
                c = A[k, :k] * rd[:k]
                tv[:k] = tv[:k] + (-c) * tv[k]
                uv[:k] = uv[:k] + (-c) * uv[k]
            if rep == 4:
                break
            e = (y - beta) - _wsum(G1 * tv[None, :])
            e2 = e * e
            sn = _wsum(Gbw * e2[None, :]) / _wsum(Gbw)
            sf = _wsum(sn) / n
            s = sn / sf
            sf_hist.append(sf)
            s_hist.append(s.copy())
            if plant == "s_prev" and rep == 3:
                s[n // 2] = s_hist[2][n // 2]
            rs = np.sqrt(s)
        tau2 = quad / (n0 if plant == "tau2_n0" else n)
        val = logdet + n * np.log(tau2)
        if plant == "sf_prev":
            sf = sf_hist[2]
        if plant == "temp_1e-10":
            tv[n // 3] *= 1 + 1e-10
        keep = dict(s=s.copy(), res2=e2.copy(), temp=tv.copy(), sf=float(sf), beta=float(beta), tau2=float(tau2))
        res = dict(status=0, val=float(val), beta=float(beta), tau2=float(tau2), loo=math.nan, keep=keep, out=None, n=n)
        Lf = np.tril(A[:n] / dg[None, :], -1)                    # the kept factor: l_ik = c_ik / d_k

        def sites(P, state_order):
            dt, da = _dist(P, X, th), _dist(P, X, al)
            g, l = ex(dt), ex(da)
            gb = ex(_dist(P, X, tb)) if state_order else ex(dt * bw)
            v = (_wsum(gb * e2[None, :]) / _wsum(gb)) / sf
            lsv = lam * np.sqrt(v)
            ls = l * rs[None, :]
            q = lsv[:, None] * ls + g
            return g, ls, lsv, q, v

        if x0 is not None:
            g, ls, lsv, q, v = sites(x0[None], True)
            res["loo"] = float(beta + _wsum((lsv[:, None] * ls + g) * tv[None, :])[0])
        if Xt is not None:
            Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, d)
            g, ls, lsv, q, v = sites(Xt, False)
            Yp = beta + _wsum(q * tv[None, :])
            gp = beta + _wsum(g * tv[None, :])
            lp = lsv * _wsum(ls * tv[None, :])
            qu = _wsum(q * uv[None, :])
            z = q.T.copy()                                       # [n, m]
            qq = np.zeros(Xt.shape[0])
            for k in range(n):
                dk = dg[k + 1] if (plant == "qq_dnext" and k + 1 < n) else dg[k]
                qq = (z[k] * z[k]) * (1.0 / dk) + qq
                z[k + 1:] = z[k + 1:] + (-Lf[k + 1:, k])[:, None] * z[k][None, :]
            w = 1.0 - qu
            ppp = ((1.0 + lam * v) - qq) + w * w / s11
            ppp = np.where(ppp < 0.0, 0.0, ppp)
            half = 1.96 * np.sqrt(tau2 * ppp)
            res["out"] = np.stack([Yp, gp, lp, v, Yp - half, Yp + half], axis=1)
    return res


# ----------------------------------------------------------------------------- the cases of the device module
CASES = ((5, 1), (14, 2), (63, 2), (64, 9), (65, 2), (128, 2), (128, 21))
LAMBDAS = (0.001, 1.0)
JACK_N = (14, 65, 128)
ILL = (128, 2, 0.001)                   # cond1 >= 1e6, asserted from the reference
FAR_ARG = 460.0                         # exp(-460) = 1.7e-200


def rows_in_the_box(Xs, B, seed):
    """as tests/test_gpu_cgp.py draws them"""
    from ccgp_amd import cgp
    lo, hi = cgp.bounds(Xs)
    ww = lo + np.random.default_rng(seed).random((B, lo.shape[0])) * (hi - lo)
    ww[0::2, 0] = 0.001
    ww[1::2, 0] = 1.0
    return cgp.rows_from_ww(ww)


@functools.lru_cache(maxsize=None)
def case(n, d):
    """(Xs, y, rows [2]: lambda 0.001 and 1, Xt [7, d], the design row of site 4) of one shape: the design and rows of
    tests/test_gpu_cgp.py; sites: four random, training point n // 3, the midpoint of training points 0 and 1, and one along the
    diagonal far enough out that the largest g is exp(-FAR_ARG) under the first row's theta."""
    from conftest import synthetic_design
    from ccgp_amd import cgp
    X, y = synthetic_design(n, d, 1000 + 10 * n + d)
    Xs, _ = cgp.standardise(X)
    rows = rows_in_the_box(Xs, 2, 7 * n + d)
    Xt = np.random.default_rng(n + d).random((7, d))
    Xt[4] = Xs[n // 3]
    Xt[5] = 0.5 * (Xs[0] + Xs[1])
    theta = np.maximum(rows[0, 1:1 + d], rows[1, 1:1 + d])
    lo, hi = 1.0, 1e6
    for _ in range(200):                                        # the smallest argument over the design is FAR_ARG
        mid = 0.5 * (lo + hi)
        arg = (((np.full(d, mid) - Xs) ** 2) * theta).sum(1).min()
        lo, hi = (mid, hi) if arg < FAR_ARG else (lo, mid)
    Xt[6] = hi
    return Xs, y, rows, Xt, n // 3


# ----------------------------------------------------------------------------- (g) the diagonal closed form
LATTICE_RATE = 1000.0
LATTICE_STEP = 3.0
LATTICE_LAMBDA = 1.0
VARIANTS = ("gbw_identity", "gbw_ones", "l_rows")


class DegenerateChain(ArithmeticError):
    """the exact chain reaches 0 / 0"""


def lattice_side(n, two_rows):
    """points in a lattice row: a square lattice, or (l_rows) two rows.  Two rows because 1'temp = 0 makes the two rows' sums of
    temp opposite at the first pass, so every residual has one magnitude and the weights stay near 1; with three equal rows one
    of them falls below 1e-3 within four passes."""
    return (n + 1) // 2 if two_rows else int(math.ceil(math.sqrt(n)))


def lattice_y(n, by_row):
    """two tight clusters below 1 and above 2, alternating from point to point (by_row: from lattice row to lattice row, so that
    the residuals of a row share a sign): no response lies near the weighted mean, and the exact chain keeps every s_i >= 1e-3
    (asserted by LatticeCase)"""
    i = np.arange(n)
    k = i // lattice_side(n, True) if by_row else i
    w = 4.0 if by_row else 128.0        # by_row: temp is what is left of y within its row, so the rows are spread, not tight
    return np.where(k % 2 == 0, 1.0 - ((7 * i) % 4) / w, 2.0 + ((5 * i) % 4) / w)


class LatticeCase:
    """An integer lattice scaled by 3 under rates of 1000 (or `rate`): every off-diagonal distance is at least 9000, exp gives
    exactly 0 and G = I.  Variants:
      gbw_identity   alpha = rate, bw = 1: L = Gbw = I, the chain is n scalar recurrences
      gbw_ones       bw = 0: Gbw is all ones and s stays 1
      l_rows         alpha = (0, rate), bw = 1: L is 1 between the points of one lattice row, so Q = I + lambda a_b a_b' on each
                     row b (a = sqrt s) and the device's elimination, substitutions and site products run on dense blocks
    The chain in fractions.Fraction, block by block through Sherman-Morrison, Q_b^-1 = I - lambda P_b / (1 + lambda tr P_b) with
    P_b = a_b a_b': its entries sqrt(s_i s_j) = |e_i e_j| / sf are rational although a_i is not.
    alpha = 0 in BOTH coordinates (L all ones) has no chain to hold: with G = I, e = (Q - G) temp = lambda a (a'temp), and at the
    first pass a = 1 and 1'temp = 0, so e = 0 exactly, sf = 0 and s = 0 / 0; in fp64 e is rounding noise and s is its square over
    its mean.  one_block = True builds that case; _chain raises DegenerateChain (tests/test_cgp_exact_host.py holds that)."""

    def __init__(self, n, variant, skip=-1, rate=LATTICE_RATE, lam=LATTICE_LAMBDA, one_block=False):
        assert variant in VARIANTS
        self.n0, self.variant, self.skip, self.lam = n, variant, skip, lam
        side = lattice_side(n, variant == "l_rows")
        i = np.arange(n)
        self.X = LATTICE_STEP * np.stack([i % side, i // side], axis=1).astype(np.float64)
        self.y = lattice_y(n, variant == "l_rows")
        alpha = [rate, rate]
        if variant == "l_rows":
            alpha = [0.0, 0.0 if one_block else rate]
        bw = 0.0 if variant == "gbw_ones" else 1.0
        self.row = np.array([lam, rate, rate, alpha[0], alpha[1], bw])
        pick = i != skip
        self.Xe, self.ye = self.X[pick], self.y[pick]
        self.n = self.Xe.shape[0]
        self.x0 = self.X[skip] if skip >= 0 else None
        if variant != "l_rows":
            self.blocks = [[j] for j in range(self.n)]
        elif one_block:
            self.blocks = [list(range(self.n))]
        else:
            rows = sorted(set(self.Xe[:, 1]))
            self.blocks = [[j for j in range(self.n) if self.Xe[j, 1] == r] for r in rows]
        self._chain()

    def solve(self, b):
        """Q^-1 b with the final P"""
        return self._solve(self.P, b)

    def _solve(self, P, b):
        lam = Fraction(self.lam)
        x = [None] * self.n
        for blk, Pb in zip(self.blocks, P):
            den = 1 + lam * sum(Pb[k][k] for k in range(len(blk)))
            for a, i in enumerate(blk):
                x[i] = b[i] - lam * sum(Pb[a][c] * b[j] for c, j in enumerate(blk)) / den
        return x

    def _chain(self):
        F = Fraction
        n, lam = self.n, F(self.lam)
        y = [F(float(v)) for v in self.ye]
        gbw_ones = self.variant == "gbw_ones"
        P = [[[F(1)] * len(b) for _ in b] for b in self.blocks]
        self.smin = F(1)
        for rep in range(5):
            xy, x1 = self._solve(P, y), self._solve(P, [F(1)] * n)
            s11 = sum(x1)
            beta = sum(xy) / s11
            temp = [a - beta * b for a, b in zip(xy, x1)]
            if rep == 4:
                break
            e = [yi - beta - ti for yi, ti in zip(y, temp)]          # G = I
            res2 = [v * v for v in e]
            sn = [sum(res2) / n] * n if gbw_ones else res2
            sf = sum(sn) / n
            if sf == 0:
                raise DegenerateChain("pass %d: every residual is exactly 0" % (rep + 1))
            s = [v / sf for v in sn]
            self.smin = min(self.smin, min(s))
            if not gbw_ones:
                P = [[[abs(e[i] * e[j]) / sf for j in b] for i in b] for b in self.blocks]
        assert self.smin >= F(1, 1000), "the exact chain must keep every weight"
        self.P = P
        self.beta, self.temp, self.s, self.res2, self.sf, self.s11, self.x1 = beta, temp, s, res2, sf, s11, x1
        self.tau2 = sum((yi - beta) * ti for yi, ti in zip(y, temp)) / n
        with mp.workdps(DPS):
            self.logdet = mp.fsum(mp.log(_fm(1 + lam * sum(Pb[k][k] for k in range(len(Pb))))) for Pb in P)
            self.val = self.logdet + n * mp.log(_fm(self.tau2))

    def sites(self):
        """[3, 2]: lattice point 1; the midpoint of lattice points 0 and 1; a point 1e3 away.
        The midpoint is NOT a finite off-lattice prediction in two of the three variants.  Its distance to the nearest points is
        1.5, so under rates of 1000 every g and l is 0 there, and with bw = 1 (gbw_identity, l_rows) every gbw too: v = 0 / 0,
        a second NaN site, where only gp = beta is finite.  With correlations that are exactly 0 or 1 a site has a finite v only
        where some gbw is 1: on a lattice point, or anywhere under bw = 0 -- so gbw_ones alone predicts finitely off the lattice
        (v = 1, Yp = gp = beta, the interval from ppp = 1 + lambda + 1 / s11), and in the other two variants the lattice-point
        site is the only finite interval.  The random, midpoint and far sites of the general cases hold the off-design
        prediction; what these sites hold is the NaN pattern and the lattice-point row."""
        return np.array([self.Xe[1], 0.5 * (self.Xe[0] + self.Xe[1]), self.Xe[0] - 1e3])

    def predict(self, Xt):
        """the exact Yp, gp, lp, v, ppp (Fractions; gp alone where v is 0 / 0) at sites whose correlations with the design are
        exactly 0 or 1"""
        F = Fraction
        n, lam = self.n, F(self.lam)
        th, al, bw = self.row[1:3], self.row[3:5], self.row[5]
        Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, 2)
        gs, ls, gbs = (cgp_ref.corr(Xt, self.Xe, r) for r in (th, al, th * bw))
        out = []
        for a in range(Xt.shape[0]):
            g, l, gb = ([F(int(v)) for v in M[a]] for M in (gs, ls, gbs))
            if sum(gb) == 0:                          # v is 0 / 0: only gp does not pass through it
                out.append(dict(gp=self.beta + sum(p * b for p, b in zip(g, self.temp))))
                continue
            v = (sum(p * q for p, q in zip(gb, self.res2)) / sum(gb)) / self.sf
            # sqrt(v s_j) is rational where s = 1 and v = 1 (gbw_ones), or where v = s_i of a lattice point i: P_ij in i's block
            if self.variant == "gbw_ones":
                assert v == 1
                vs = [F(1)] * n
            else:
                i = [int(x) for x in gb].index(1)
                assert v == self.s[i]
                vs = [F(0)] * n
                for blk, Pb in zip(self.blocks, self.P):
                    if i in blk:
                        for c, j in enumerate(blk):
                            vs[j] = Pb[blk.index(i)][c]
                assert all(l[j] == 0 or vs[j] != 0 for j in range(n))
            q = [p + lam * b * c for p, b, c in zip(g, vs, l)]
            w = self.solve(q)
            Yp = self.beta + sum(p * b for p, b in zip(q, self.temp))
            gp = self.beta + sum(p * b for p, b in zip(g, self.temp))
            qu = sum(p * b for p, b in zip(q, self.x1))
            ppp = 1 + lam * v - sum(p * b for p, b in zip(q, w)) + (1 - qu) ** 2 / self.s11
            out.append(dict(Yp=Yp, gp=gp, lp=Yp - gp, v=v, ppp=ppp))
        return out


def _fm(q):
    return mp.mpf(q.numerator) / mp.mpf(q.denominator)


# ----------------------------------------------------------------------------- (g) running first-order error bounds
class R:
    """An fp64 array with a running first-order bound of what the device's value may differ from the exact one by.  Every
    operation adds u |result| for its own rounding -- except where it is exact on any machine: adding an exact 0, multiplying by
    an exact 0 or 1.  On the lattice that is every step of the elimination and of the substitutions (variants with L = I), so a
    bound carries neither n nor a condition number: only the roundings the values actually went through.  The bound is
    evaluated along the fp64 values, the references come from the Fraction chain: the two differ at second order."""
    __array_priority__ = 100

    def __init__(self, v, e=None):
        self.v = np.array(v, dtype=np.float64)
        self.e = np.zeros(self.v.shape) if e is None else np.array(np.broadcast_to(e, self.v.shape), dtype=np.float64)

    @staticmethod
    def of(o):
        return o if isinstance(o, R) else R(o)

    def _exact(self, c):
        return (self.v == c) & (self.e == 0)

    def __add__(self, o):
        o = R.of(o)
        v = self.v + o.v
        free = self._exact(0) | o._exact(0)
        return R(v, self.e + o.e + np.where(free, 0.0, U * np.abs(v)))
    __radd__ = __add__

    def __neg__(self):
        return R(-self.v, self.e)

    def __sub__(self, o):
        return self + (-R.of(o))

    def __rsub__(self, o):
        return R.of(o) + (-self)

    def __mul__(self, o):
        o = R.of(o)
        v = self.v * o.v
        free = self._exact(0) | o._exact(0) | self._exact(1) | o._exact(1)
        return R(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + np.where(free, 0.0, U * np.abs(v)))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R.of(o)
        v = self.v / o.v
        free = self._exact(0) | o._exact(1)
        return R(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + np.where(free, 0.0, U * np.abs(v)))

    def __rtruediv__(self, o):
        return R.of(o) / self

    def __getitem__(self, i):
        return R(self.v[i], self.e[i])

    def __setitem__(self, i, o):
        o = R.of(o)
        self.v[i], self.e[i] = o.v, o.e

    def copy(self):
        return R(self.v, self.e)

    def sqrt(self):
        v = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            small = self.e * 16 < self.v                              # |sqrt(x + t) - sqrt x| <= (t / (2 sqrt x)) (1 + t / x)
            lin = np.where(small, self.e / (2 * v) * (1 + self.e / self.v), 0.0)
        wide = np.maximum(v - np.sqrt(np.maximum(self.v - self.e, 0.0)), np.sqrt(self.v + self.e) - v)
        return R(v, np.where(small, lin, wide) + np.where(self._exact(0) | self._exact(1), 0.0, U * v))

    def log(self):
        v = np.log(self.v)
        return R(v, self.e / np.abs(self.v) + np.where(self._exact(1), 0.0, 2 * U * np.abs(v)))

    def wsum(self):
        """cgp_wave_sum of two terms a lane: at most 7 additions on any path"""
        live = np.count_nonzero((self.v != 0) | (self.e != 0), axis=-1)
        return R(self.v.sum(-1), self.e.sum(-1) + np.where(live > 1, 7 * U * np.abs(self.v).sum(-1), 0.0))


def running(G, Lc, Gbw, y, lam, site=None, held=None, rep0=0, s0=None, stop=None):
    """cgp_state_kernel and cgp_predict_kernel in R arithmetic on correlation matrices known exactly (entries 0 or 1): dict of R
    (beta, tau2, val, temp, s, sf, res2; Yp gp lp v tp = tau2 ppp at the sites (g, l, gbw) of `site`; loo at `held`).  The chain
    enters pass rep0 (0-based) with the weights s0 taken as exact; stop: return the weights pass `stop` leaves."""
    n = len(y)
    G, Lc, Gbw, y, lam = R(G), R(Lc), R(Gbw), R(y), R(lam)
    G1 = G.copy()
    G1[np.diag_indices(n)] = 1.0
    rs = R(np.ones(n) if s0 is None else s0).sqrt()
    with np.errstate(all="ignore"):
        for rep in range(rep0, 5):
            A = R(np.zeros((n + 2, n)))
            A[:n] = lam * ((rs[:, None] * Lc) * rs[None, :]) + G
            dq = lam * (rs * rs) + 1.0
            A.v[np.arange(n), np.arange(n)], A.e[np.arange(n), np.arange(n)] = dq.v, dq.e
            A[n], A[n + 1] = y, 1.0
            for k in range(n):
                rinv = 1.0 / A[k, k]
                ljk = A[k + 1:n, k] * rinv
                A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - A[k + 1:, k][:, None] * ljk[None, :]
            dg = R(np.diag(A.v[:n]), np.diag(A.e[:n]))
            rd = 1.0 / dg
            zy, z1 = A[n].copy(), A[n + 1].copy()
            s11 = ((z1 * z1) * rd).wsum()
            beta = ((z1 * zy) * rd).wsum() / s11
            r = zy - beta * z1
            quad = ((r * r) * rd).wsum()
            logdet = dg.log().wsum()
            tv, uv = r * rd, z1 * rd
            for k in range(n - 1, 0, -1):
                c = A[k, :k] * rd[:k]
                tv[:k] = tv[:k] - c * tv[k]
                uv[:k] = uv[:k] - c * uv[k]
            if rep == 4:
                break
            e = (y - beta) - (G1 * tv[None, :]).wsum()
            e2 = e * e
            sn = (Gbw * e2[None, :]).wsum() / Gbw.wsum()
            sf = sn.wsum() / float(n)
            s = sn / sf
            if stop == rep:
                return s
            rs = s.sqrt()
        tau2 = quad / float(n)
        res = dict(beta=beta, tau2=tau2, val=logdet + float(n) * tau2.log(), logdet=logdet, temp=tv, s=s, sf=sf, res2=e2)
        Lf = R(np.tril(A.v[:n], -1), np.tril(A.e[:n], -1)) / dg[None, :]

        def terms(g, l, gb):
            g, l, gb = R(g), R(l), R(gb)
            v = ((gb * e2[None, :]).wsum() / gb.wsum()) / sf
            lsv = lam * v.sqrt()
            ls = l * rs[None, :]
            return g, ls, lsv, lsv[:, None] * ls + g, v

        if held is not None:
            g, ls, lsv, q, v = terms(*held)
            res["loo"] = beta + (q * tv[None, :]).wsum()
        if site is not None:
            g, ls, lsv, q, v = terms(*site)
            Yp = beta + (q * tv[None, :]).wsum()
            gp = beta + (g * tv[None, :]).wsum()
            lp = lsv * (ls * tv[None, :]).wsum()
            qu = (q * uv[None, :]).wsum()
            z = R(q.v.T, q.e.T)
            qq = R(np.zeros(z.v.shape[1]))
            for k in range(n):
                qq = (z[k] * z[k]) * (1.0 / dg[k]) + qq
                z[k + 1:] = z[k + 1:] - Lf[k + 1:, k][:, None] * z[k][None, :]
            w = 1.0 - qu
            ppp = ((1.0 + lam * v) - qq) + w * w / s11
            res.update(Yp=Yp, gp=gp, lp=lp, v=v, tp=tau2 * ppp)
    return res


def _fchain(G, Lc, Gbw, y, lam, s, rep0, stop=None, site=None, held=None):
    """the same chain in plain fp64 through numpy's solves: the function whose derivatives carry a bound from pass to pass"""
    n = len(y)
    one = np.ones(n)
    with np.errstate(all="ignore"):
        for rep in range(rep0, 5):
            rs = np.sqrt(s)
            Q = G + lam * np.outer(rs, rs) * Lc
            Wm = np.linalg.solve(Q, np.stack([y, one], axis=1))
            s11 = Wm[:, 1].sum()
            beta = Wm[:, 0].sum() / s11
            temp = Wm[:, 0] - beta * Wm[:, 1]
            if rep == 4:
                break
            e = y - beta - G @ temp
            e2 = e * e
            sn = (Gbw @ e2) / Gbw.sum(1)
            sf = sn.mean()
            s = sn / sf
            if stop == rep:
                return dict(s=s)
        tau2 = (y - beta) @ temp / n
        res = dict(beta=beta, tau2=tau2, val=np.linalg.slogdet(Q)[1] + n * np.log(tau2), temp=temp, s=s, sf=sf, res2=e2)

        def terms(g, l, gb):
            v = ((gb @ e2) / gb.sum(1)) / sf
            return v, g + lam * np.sqrt(v)[:, None] * (l * rs[None, :])
        if held is not None:
            res["loo"] = beta + terms(*held)[1] @ temp
        if site is not None:
            g = site[0]
            v, q = terms(*site)
            ppp = 1 + lam * v - (q * np.linalg.solve(Q, q.T).T).sum(1) + (1 - q @ Wm[:, 1]) ** 2 / s11
            res.update(Yp=beta + q @ temp, gp=beta + g @ temp, lp=(q - g) @ temp, v=v, tp=tau2 * ppp)
    return res


def lattice_bands(G, Lc, Gbw, y, lam, site=None, held=None):
    """A bound per output of the chain on exactly known correlation matrices, to first order:

        the roundings of each pass, bounded in R arithmetic from that pass's input taken as exact (eps_k, k = 0, 1, 2), carried to
        the weights that enter the fourth pass through the passes' own derivatives:  ds3 = eps_2 + |J_2| eps_1 + |J_2 J_1| eps_0;
        the roundings of the fourth and fifth pass and of the prediction, in R arithmetic from those weights as exact;
        |d output / d s3| ds3.

    The derivatives (one-sided differences of _fchain, relative step 1e-6) are the chain's own sensitivity -- where a weight falls
    super-quadratically it is large, and stated as such -- and carry the common-mode cancellations (an error of beta moves every
    residual alike and leaves s = sn / sf nearly alone) that a running bound through all five passes cannot see: that one is 1e7
    roundings wide on the gbw_ones variant, whose weights are exactly 1."""
    n = len(y)
    y = np.asarray(y, dtype=np.float64)
    S = [np.ones(n)]
    for k in range(3):
        S.append(_fchain(G, Lc, Gbw, y, lam, S[k], k, stop=k)["s"])
    eps = [running(G, Lc, Gbw, y, lam, rep0=k, s0=S[k], stop=k).e for k in range(3)]

    def jac(f, s):
        base = f(s)
        cols = []
        for i in range(n):
            sp = s.copy()
            h = 1e-6 * s[i]
            sp[i] += h
            cols.append({key: (np.asarray(v) - np.asarray(base[key])) / h for key, v in f(sp).items()})
        return {key: np.stack([np.asarray(c[key], dtype=np.float64).reshape(-1) for c in cols], axis=1) for key in base}

    J1 = jac(lambda s: _fchain(G, Lc, Gbw, y, lam, s, 1, stop=1), S[1])["s"]
    J2 = jac(lambda s: _fchain(G, Lc, Gbw, y, lam, s, 2, stop=2), S[2])["s"]
    ds3 = eps[2] + np.abs(J2) @ eps[1] + np.abs(J2 @ J1) @ eps[0]
    tail = running(G, Lc, Gbw, y, lam, site, held, rep0=3, s0=S[3])
    JT = jac(lambda s: _fchain(G, Lc, Gbw, y, lam, s, 3, site=site, held=held), S[3])
    with np.errstate(invalid="ignore"):
        return {key: (tail[key].e.reshape(-1) + np.abs(J) @ ds3).reshape(tail[key].e.shape) for key, J in JT.items()}


def _fr(v):
    return Fraction(float(v))


def lattice_check(t, lc, dev, Xt=None, out=None):
    """the device's (or the restatement's) outputs of LatticeCase lc against the Fraction chain under the running bounds.  dev:
    dict(val, beta, tau2, loo or None, keep or None); out: [m, 6] at the sites Xt.  NaN must stand exactly where cgp_ref has it."""
    X, y, row, lam = lc.Xe, lc.ye, lc.row, lc.lam
    th, al, bw = row[1:3], row[3:5], row[5]
    mats = [cgp_ref.corr(X, X, r) for r in (th, al, th * bw)]

    def vecs(P):
        return [cgp_ref.corr(np.asarray(P, dtype=np.float64).reshape(-1, 2), X, r) for r in (th, al, th * bw)]
    held = vecs(lc.x0) if lc.x0 is not None else None
    site = vecs(Xt) if Xt is not None else None
    for M in mats + (held or []) + (site or []):
        assert np.all((M == 0) | (M == 1)), "the lattice's correlations are exactly 0 or 1"
    run = lattice_bands(mats[0], mats[1], mats[2], y, lam, site, held)

    def hold(key, got, ref, bound):
        t.add(key, _ratio(abs(_fr(got) - ref), float(bound)))

    hold("lattice beta", dev["beta"], lc.beta, run["beta"])
    hold("lattice tau2", dev["tau2"], lc.tau2, run["tau2"])
    with mp.workdps(DPS):
        t.add("lattice val", _ratio(abs(_mpf(dev["val"]) - lc.val), float(run["val"])))
    keep = dev.get("keep")
    if keep is not None:
        hold("lattice sf", keep["sf"], lc.sf, run["sf"])
        for i in range(lc.n):
            hold("lattice temp", keep["temp"][i], lc.temp[i], run["temp"][i])
            hold("lattice s", keep["s"][i], lc.s[i], run["s"][i])
            hold("lattice res2", keep["res2"][i], lc.res2[i], run["res2"][i])
    ref64 = cgp_ref.state(lc.X, lc.y, row, lc.skip)
    if lc.x0 is not None:
        if math.isnan(float(ref64["loo"])):
            t.add("lattice loo nan", 0.0 if math.isnan(dev["loo"]) else math.inf)
        else:
            # the only finite held-out prediction on the lattice: gbw_ones, where g = l = 0 and the prediction is beta
            assert lc.variant == "gbw_ones"
            hold("lattice loo", dev["loo"], lc.beta, run["loo"][0])
    if Xt is not None:
        out = np.asarray(out, dtype=np.float64)
        want_nan = np.isnan(cgp_ref.predict(lc.Xe, lc.ye, row, Xt)[0])
        t.add("lattice nan pattern", 0.0 if np.array_equal(np.isnan(out), want_nan) else math.inf)
        exact, ro = lc.predict(Xt), run
        for a, ex in enumerate(exact):
            if "v" not in ex:
                assert want_nan[a].tolist() == [True, False, True, True, True, True]
                hold("lattice gp", out[a, 1], ex["gp"], ro["gp"][a])
                continue
            assert not want_nan[a].any()
            for c, key in ((0, "Yp"), (1, "gp"), (2, "lp"), (3, "v")):
                hold("lattice " + key, out[a, c], ex[key], ro[key][a])
            ymax = float(np.abs(out[a, [0, 4, 5]]).max())
            want = lc.tau2 * ex["ppp"]
            for key, h in (("Y_up", _fr(out[a, 5]) - _fr(out[a, 0])), ("Y_low", _fr(out[a, 0]) - _fr(out[a, 4]))):
                hs = h / _fr(1.96)
                band = float(ro["tp"][a]) + 8 * U * (abs(float(want)) + float(ro["tp"][a])) \
                    + 2 * abs(float(hs)) * U * ymax / 1.96 + (U * ymax / 1.96) ** 2
                t.add("lattice " + key, _ratio(abs(hs * hs - want), band) if h >= 0 else math.inf)
