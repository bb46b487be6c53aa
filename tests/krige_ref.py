"""Reference for ccgp_krige_predict_batch -- the single-GP comparator's prediction in its three variance forms -- shared by
tests/test_krige_ref.py (host) and tests/test_gpu_krige.py (device).  Nothing here runs on the device.

The forms, in long double on top of oracle.ccgp_oracle.predict_factor / predict_parts (direct squared differences, the
hand-written Cholesky), with q = r'R^-1 r, u = 1 - 1'R^-1 r, s11 = 1'R^-1 1, g = R^-1 (y - beta 1):
    Q_ref    = (y - beta 1)'g
    ordinary = sigma2 (1 - q + u^2 / s11)            predict.post, HX:669 / D1:490
    plugin   = sigma2 (1 - q)                        mlegp's se.fit^2
    unbiased = Q_ref / (n - 1) (1 - q + u^2 / s11)   D1:504-516
Another family than the Gaussian passes Rc, rc, rho and rho_t as tests/test_gpu_family_end_to_end.py does.

The bands are component-wise, with C = oracle.ccgp_oracle.PREDICT_TOL_C and Q(., .), eta, eta0 and W exactly as
oracle.ccgp_oracle.predict_bands defines them (a backward error |dR| <= eta W of the factorisation and the solves, a relative
eps (1 + rho) of every entry of R and r):
    band_ordinary = predict_bands' band_var
    band_plugin   = sigma2 (Q(r, r) + eps (1 + ww))
    band_Q        = eta0 (|g|'W|g| + 2 |g|'|y - beta 1|) + eps sum_i |y_i (R^-1 y)_i|
    band_unbiased = Q_ref / (n - 1) band_var(sigma2 = 1) + |1 - q + u^2 / s11| band_Q / (n - 1)
band_Q has no first-order term in beta: dQ / dbeta = -2 1'g = 0 at the profile beta; its last term is the size of y'R^-1 y
before the cancellation against beta^2 s11.  No condition number and no floor.

The margin (tests/test_krige_ref.py asserts at least 8, as tests/test_oracle.py asks of band_var): over the cases of
tests/test_gpu_krige.py a plain fp64 restatement of the device formula (oracle.predict_device_restatement, then the three
forms) uses at most 0.55 units of band / C for plugin, 0.55 for unbiased and 0.030 for Q -- about 230 times inside C = 128."""
import numpy as np

from oracle import ccgp_oracle as orc

EPS = float(np.finfo(np.float64).eps)
C = orc.PREDICT_TOL_C
ORDINARY, PLUGIN, UNBIASED = 0, 1, 2
FORMS = (ORDINARY, PLUGIN, UNBIASED)
FORM_NAMES = {ORDINARY: "ordinary", PLUGIN: "plugin", UNBIASED: "unbiased"}

# (route, n, d, K, m) of the exactness cases of tests/test_gpu_krige.py; the d = 1 case has theta ~ n^2 (interior and far sites only)
CASES = [("kept", 2, 4, 2, 64), ("kept", 9, 4, 3, 64), ("kept", 40, 1, 2, 65), ("kept", 64, 2, 3, 65), ("kept", 104, 9, 3, 257),
         ("extra", 105, 2, 2, 62), ("extra", 128, 9, 1, 63), ("extra", 50, 4, 4, 31),
         ("blocked", 129, 3, 2, 129), ("blocked", 257, 2, 3, 1)]


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def reference(X, y, row, K, Xtest, factor=None, Rc=None, **family):
    """One model at the rows of Xtest, in long double: dict(parts: predict_parts at sigma2 = 1, mean[m], unit[m] = 1 - q + u^2 /
    s11, plug_unit[m] = 1 - q, beta, s11, Q, n, factor).  family: rc, raw_r, rho, rho_t of predict_parts (with Rc for the factor)."""
    d = X.shape[1]
    f = factor if factor is not None else orc.predict_factor(X, y, row, K, d, np.longdouble, Rc=Rc)
    parts = orc.predict_parts(X, y, row, K, d, 1.0, Xtest, np.longdouble, factor=f, **family)
    yc = f["y"] - f["beta"]
    return dict(parts=parts, mean=parts["mean"], unit=parts["var"], plug_unit=np.longdouble(1) - parts["ww"], beta=f["beta"],
                s11=f["s11"], Q=yc @ f["g"], n=f["y"].shape[0], factor=f)


def variance(ref, form, sigma2=None):
    """The form's variance [m] in long double; UNBIASED takes no sigma2."""
    if form == PLUGIN:
        return np.longdouble(sigma2) * ref["plug_unit"]
    if form == UNBIASED:
        return ref["Q"] / np.longdouble(ref["n"] - 1) * ref["unit"]
    return np.longdouble(sigma2) * ref["unit"]


def bands(ref, c=C):
    """dict(mean[m], beta, s11, unit[m] = band_var at sigma2 = 1, plug_unit[m], Q) around reference()."""
    parts, f = ref["parts"], ref["factor"]
    b = orc.predict_bands(parts, 1.0, c)
    W, r, a, ww = (_f64(parts[k]) for k in ("W", "r", "a", "ww"))
    A, Rr = np.abs(a), np.abs(r)
    eta0 = c * EPS * (1.0 + parts["rho"])
    eta = c * EPS * (1.0 + np.maximum(parts["rho"], parts["rho_t"]))
    q_ww = eta * (((A @ W) * A).sum(axis=1) + 2.0 * (A * Rr).sum(axis=1))
    G = np.abs(_f64(f["g"]))
    yc = np.abs(_f64(f["y"] - f["beta"]))
    size = float(np.sum(np.abs(_f64(f["y"])) * np.abs(_f64(f["Rinv_y"]))))
    band_Q = eta0 * (G @ W @ G + 2.0 * (G @ yc)) + EPS * size
    return dict(mean=b["mean"], beta=b["beta"], s11=b["s11"], unit=b["var"], plug_unit=q_ww + EPS * (1.0 + ww), Q=float(band_Q))


def variance_band(ref, bnd, form, sigma2=None):
    """The form's band [m]."""
    if form == PLUGIN:
        return sigma2 * bnd["plug_unit"]
    if form == UNBIASED:
        n1 = ref["n"] - 1
        return float(ref["Q"]) / n1 * bnd["unit"] + np.abs(_f64(ref["unit"])) * bnd["Q"] / n1
    return sigma2 * bnd["unit"]


def device_restatement(X, y, row, K, Xtest):
    """Plain fp64 restatement of the device formula: oracle.predict_device_restatement, then dict(mean[m], unit[m], plug_unit[m],
    beta, s11, Q) with Q summed as the device's likelihood sums it: sum_c (zy_c - beta z1_c)^2 / d_c."""
    dev = orc.predict_device_restatement(X, y, row, K, X.shape[1], Xtest)
    mean, unit, ww, _, _ = orc.predict_device_finish(dev, 1.0)
    v = dev["zy"] - dev["beta"] * dev["z1"]
    return dict(mean=mean, unit=unit, plug_unit=1.0 - ww, beta=dev["beta"], s11=dev["s11"], Q=float(np.sum(v * v * dev["rd"])))


def literal_d1_unbiased(R, r, y, sigma2):
    """post.var.single and post.stdev.single^2 of the 1-D script, line by line in fp64 (D1:481-516): explicit R.Inv, S and Q.sq.
    R[n, n], r[m, n] (row t = corr.vec at site t); returns (var[m], var_post[m])."""
    n = R.shape[0]
    R_Inv = np.linalg.inv(R)
    ones = np.ones(n)
    var = sigma2 * (1.0 - np.diag(r @ R_Inv @ r.T) + (1.0 - ones @ R_Inv @ r.T) ** 2 / R_Inv.sum())       # D1:490
    U = R_Inv.sum(axis=1)                                                                                      # D1:510
    S = np.tile(U, (n, 1)) / U.sum()                                                                           # D1:511, byrow
    Q_sq = y @ (R_Inv - R_Inv @ S) @ y                                                                         # D1:512
    return var, Q_sq * var / (sigma2 * (n - 1))                                                                # D1:513-514
