"""Reference, bands and case list of the exact yardstick of the max-entropy design criteria: ccgp_mixed_logdet_designs,
ccgp_mixed_logdet_grad_designs (small_reg_kernel, INV = 3) and the Entropy* functions built on them.  No GPU and no device
number in here: tests/test_design_exact_host.py holds this module to mpmath, measures the two constants and shows that the
bands bite; tests/test_gpu_design_exact.py runs the cases on the device.

Reference (long double, eps 1.1e-19; oracle.require_extended_precision).  R = sum_q (w_q^2 / sw) R_q from direct squared
differences (oracle.component_corr), L = oracle._chol_lower(R), A = R^-1 = L^-T L^-1 (oracle._lower_inverse), and

    ld_ref     = 2 sum_i log L_ii
    g_ref[i,k] = -4 sum_{j != i} A_ij (x_ik - x_jk) S_ijk,      S_ijk = sum_q (w_q^2 / sw) theta_qk R_q,ij.

Bands: first order, component-wise, no norm-wise condition number (the stance of tests/test_gpu_marginal_exact.py).  A device
entry of R is granted the relative error e_ab = eps (1 + rho_ab), rho_ab = max_q (u_qa + u_qb + 2 |x_a' Theta_q x_b|), u_qa =
sum_k theta_qk x_ak^2: the size of the terms of the expanded exponent the kernels form (HX:352-355; per entry what
oracle.expanded_form_magnitude gives as one number per case).  With E = |R| o e:

    log det moves by tr(A dR):   unit_ld      = sum_ab |A_ab| E_ab
    dA = -A dR A:                unit_g[i,k]  = 4 sum_j ((|A| E |A|)_ij + eps (1 + rho_ij) |A_ij|) |x_ik - x_jk| S_ijk

(the first term: the perturbation of the inverse; the second: the rounding of the term itself and of its sum).  A result
passes when |dev - ref| <= C_LD unit_ld and |dev - ref| <= C_G unit_g entry by entry; the only floor is 1e-300.  First order
holds only while eps cond_1(R) is small: every case asserts cond_1(R) <= KAPPA_MAX (the gradient module's) from the
long-double inverse, none is skipped, and the parameter rows come from oracle.conditioned_row so that the reference alone
stays inside the cap (checked on the CPU for the whole list by the host module).  The `dyadic` class has design coordinates
on the 2^-6 lattice and thetas that are powers of two, so u, the dot product and the exponent are exact in fp64: it is held
with rho = 0, so that the allowance for the expanded form cannot hide an error.

The constants.  The host module evaluates fp64_restatement() -- a correct plain fp64 implementation: exponent in the scripts'
expanded form (oracle.corr_matrix), LAPACK Cholesky and inverse -- on all_cases() below and records the largest |fp64 - ref| /
unit as oracle.DESIGN_LD_LAPACK_MAX and oracle.DESIGN_GRAD_LAPACK_MAX.  C is 32 times that figure (the device's own
summation orders, a 2-ulp exp, the register evaluator's elimination order), rounded up to a power of two and capped at
GRAD_TOL_C = 128: design_constants().  Nothing here comes from a device run.

Routes are asserted through the restatement of csrc/small_layout.h's RegCarve below (reg_carve_total: the whole carve,
per-design copies included; the host module pins it against the restatements tests/test_gpu_failure_contract.py and
tests/test_gpu_gradient_exact.py carry and against tests/route_witnesses.py).
"""
import functools
import math
import time
from collections import namedtuple

import numpy as np

from oracle import ccgp_oracle as orc

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
FLOOR = 1e-300
KAPPA_DRAW = 1e6                    # conditioned_row's cap for the design the row is drawn on; its batch mates share the row
REFERENCE_SECONDS = [0.0]           # host time spent on long-double references through case_reference()
REFERENCE_SECONDS_MAX = 6.0         # the references of the whole case list take 2.7 s where this was written; asserted by both modules


# ----------------------------------------------------------------------------- csrc/small_layout.h, default build (no exp table)
def lds_fits(total, per_cu=1):
    return 8 * total <= 160 * 1024 // per_cu - 64


def reg_carve_total(G, NB, NE, inv, per_design, n, d, K):
    """RegCarve(G, NB, NE, inv, per_design, n, d, K).total in doubles."""
    NP, XR, MPW = G * NB, G * NE, 256 // (G * G)
    mat0 = d * n
    tail = K * NP + K * d + K + 2 * (NP + XR) + NP + 2 * NP + 8
    per_mat = tail + (NP * (NP + 2) + 1 + 4 * 28 if inv else (K * XR + 3 * XR * G if NE > 1 else 0))
    xs_own = mat0 + MPW * per_mat + (d * XR if NE > 1 and not inv else 0)
    return xs_own + (MPW * d * n if per_design else 0)


def small_reg_fits8(n, d, K, per_design):
    return lds_fits(reg_carve_total(8, (n + 7) // 8, 1, False, per_design, n, d, K))


def small_reg_supported(n, d, K, per_design=False):
    if n > 128:
        return False
    G = 8 if n <= 64 else 16
    return lds_fits(reg_carve_total(G, (n + G - 1) // G, 1, False, per_design, n, d, K))


def small_reg_inverse_supported(n, d, K, per_design=False):
    NB = (n + 15) // 16
    return n <= 128 and lds_fits(reg_carve_total(16, NB, NB + 1, True, per_design, n, d, K))


def design_grad_route(n, d, K):
    """small_route(Op::DesignGrad): 'r' or 'u' (refused)."""
    return "r" if small_reg_inverse_supported(n, d, K, True) else "u"


def logdet_route(n, d, K):
    """small_route(Op::LogdetDesigns): 'r' or 'b' (the blocked sweep, one design at a time)."""
    return "r" if small_reg_supported(n, d, K, True) else "b"


def logdet_instance(n, d, K):
    """Which instance dispatch() (csrc/small_reg.hip) gives a per-design call, which is never `wide`: `reg8` the 8 x 8 grid with
    NB 1..8 (four designs per workgroup, a private xs_own copy each), `wave` the same grid with NB 9..13 where the per-design
    carve fits, `reg16` the 16 x 16 grid, `blocked` the sweep."""
    if logdet_route(n, d, K) == "b":
        return "blocked"
    if n <= 64:
        return "reg8"
    return "wave" if n <= 104 and small_reg_fits8(n, d, K, True) else "reg16"


# ----------------------------------------------------------------------------- cases
Case = namedtuple("Case", "cls n d K B")

# small_reg.hip:1117 dispatch_inv<3>: pick<1, 8>((n + 15) / 16) -- every NB at its first, last and one-past size; d and K
# cycle through {1, 2, 3, 7} and {1, 2, 3, 8} so that every NB sees an odd d and (where its carve takes it) K = 8
INSTANCES = [(1, 1, 1), (2, 2, 2), (15, 3, 3), (16, 7, 8),          # NB 1
             (17, 1, 2), (31, 2, 3), (32, 3, 8),                    # NB 2
             (33, 7, 1), (47, 1, 8), (48, 2, 2),                    # NB 3
             (49, 3, 3), (63, 7, 8), (64, 1, 1),                    # NB 4
             (65, 2, 8), (79, 3, 2), (80, 7, 3),                    # NB 5
             (81, 1, 8), (95, 2, 1), (96, 3, 3),                    # NB 6
             (97, 7, 8), (111, 1, 2), (112, 2, 3),                  # NB 7
             (113, 3, 8), (127, 7, 3), (128, 9, 3)]                 # NB 8 (n = 127, 128 at d = 9: K <= 3 stays on route r)
# small_reg.hip:676-710, pass 2: nkc = ceil(d / 8) chunks, the clamped lanes kk = d - 1 of the last chunk, the output's odd
# leading dimension nfree = 49; and small_reg.hip:678 `item += TPM`: nfree nkc > 256 runs the loop's second trip
CHUNKS = [(49, 8, 1), (49, 9, 2), (49, 16, 3), (49, 17, 1), (49, 24, 2), (49, 25, 3),
          (100, 17, 1), (97, 17, 2), (65, 25, 2), (65, 33, 2), (81, 17, 8), (97, 17, 8)]
# (81, 17, 8) has 81 x 3 = 243 items, one trip: it stays as a three-chunk K = 8 case, and (97, 17, 8) is the K = 8 second trip
SECOND_TRIP = [c for c in CHUNKS if c[0] * ((c[1] + 7) // 8) > 256]
# small_reg.hip:664-672, where pass 1 parks R^-1_ij: Z[i][j] for j <= i - 2, Z[i][NP] for j = i - 1; `i < nf` skips the
# (fixed, fixed) pairs.  n < NP = 48 and n == NP; n_fixed at 1, at odd and even rows and at a multiple of 16
FIXED = [(33, 3, 2), (48, 2, 3)]
# small_reg.hip:696-697, the expanded exponent: exact in fp64 on these inputs, held with rho = 0
DYADIC = [(14, 2, 2), (33, 4, 1), (64, 3, 3)]
# small_reg.hip:1140 / 1136 launch_one<8, NB>: four designs per workgroup, each with its xs_own copy (small_layout.h:87);
# small_reg.hip:707 the gradient's per-design output block
POSITION = [(7, 3, 2), (14, 2, 2), (64, 2, 3), (100, 3, 2)]
POSITION_B = (1, 3, 5, 70)
# small_reg.hip:1135-1142 dispatch<1>() with x_stride != 0, and capi.hip:1608 the blocked loop over designs
LOGDET = [(1, 1, 1), (7, 3, 2), (8, 2, 8), (9, 7, 3), (63, 2, 2), (64, 9, 3),        # 8 x 8 grid, NB 1..8
          (65, 2, 1), (72, 3, 2), (73, 7, 3), (104, 2, 8),                             # NB 9..13
          (105, 3, 2), (128, 2, 3),                                                    # 16 x 16 grid
          (49, 63, 8), (129, 2, 2), (193, 3, 1), (257, 4, 2)]                          # blocked sweep; the first: the route witness
# rsurface.py:206-226: Entropy, Entropy_batch, Augmented_Mixed_Entropy at 14 and 14 + 7 points in [-1, 1]^2
PYTHON_PRIOR = (0.7, 2.0, 16.0)     # p, theta1, theta2 of test_gpu_parity.test_entropy_criteria_over_candidate_designs
PYTHON_14 = Case("python", 14, 2, 2, 5)
PYTHON_21 = Case("python", 21, 2, 2, 1)


def fixed_values(n):
    return sorted({0, 1, 2, 15, 16, 17, n - 2, n - 1})


def grad_cases():
    """Every case whose gradient (and log det) is held: Case(cls, n, d, K, B)."""
    out = [Case("instances", n, d, K, 2) for n, d, K in INSTANCES]
    out += [Case("chunks", n, d, K, 2) for n, d, K in CHUNKS]
    out += [Case("fixed", n, d, K, 2) for n, d, K in FIXED]
    out += [Case("dyadic", n, d, K, 2) for n, d, K in DYADIC]
    out += [Case("position", n, d, K, max(POSITION_B)) for n, d, K in POSITION]
    return out


def logdet_cases():
    """Every case whose log det alone is held (the gradient cases go through ccgp_mixed_logdet_designs as well where the
    device module says so)."""
    return [Case("logdet", n, d, K, 2) for n, d, K in LOGDET] + [PYTHON_14, PYTHON_21]


def all_cases():
    return grad_cases() + logdet_cases()


_CLASS_ID = {"instances": 1, "chunks": 2, "fixed": 3, "dyadic": 4, "position": 5, "logdet": 6, "python": 7}


def _dyadic_inputs(case, rng):
    """Distinct points on the 2^-6 lattice of [-1, 1]^d and thetas 2^(m + q + k mod 2): m the smallest at which every design of
    the batch has an fp64 cond_1(R) <= KAPPA_DRAW."""
    designs = np.empty((case.B, case.n, case.d))
    for b in range(case.B):
        while True:
            pts = rng.integers(-64, 65, size=(case.n, case.d))
            if len({tuple(p) for p in pts}) == case.n:
                break
        designs[b] = pts / 64.0
    w = 0.2 + 0.6 * rng.random(case.K)
    for m in range(-4, 20):
        Th = np.array([[2.0 ** (m + q + k % 2) for k in range(case.d)] for q in range(case.K)])
        if max(np.linalg.cond(orc.mixed_corr_matrix_general(D, w, Th), 1) for D in designs) <= KAPPA_DRAW:
            return designs, np.concatenate([w, Th.ravel()])
    raise RuntimeError("no dyadic theta with cond1 <= %g" % KAPPA_DRAW)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(designs[B, n, d], row) of a case: seeded, uniform in [-1, 1]^d (pairwise different in every coordinate), one
    oracle.conditioned_row drawn on design 0 and shared by the batch as the entry points share it."""
    rng = np.random.default_rng([_CLASS_ID[case.cls], case.n, case.d, case.K])
    if case.cls == "dyadic":
        designs, row = _dyadic_inputs(case, rng)
    elif case.cls == "python":
        designs = rng.uniform(-1.0, 1.0, (case.B, case.n, case.d))
        if case == PYTHON_21:           # D.old U D.new: the first 14-point design and seven new points
            designs[0, :14] = case_inputs(PYTHON_14)[0][0]
        row = orc.params_from_iso(*PYTHON_PRIOR, case.d)
    else:
        designs = rng.uniform(-1.0, 1.0, (case.B, case.n, case.d))
        row, _ = orc.conditioned_row(designs[0], case.K, case.d, rng, KAPPA_DRAW)
    designs.setflags(write=False)
    row.setflags(write=False)
    return designs, row


# ----------------------------------------------------------------------------- reference and bands
Ref = namedtuple("Ref", "ld g unit_ld unit_g kappa")


def expanded_magnitude(X, row, K):
    """rho[a, b] = max_q (u_qa + u_qb + 2 |x_a' Theta_q x_b|), fp64 (a size, not a value)."""
    X = np.asarray(X, dtype=np.float64)
    _, Th = orc.unpack_params(row, K, X.shape[1])
    rho = np.zeros((X.shape[0], X.shape[0]))
    for q in range(K):
        u = (X ** 2) @ Th[q]
        rho = np.maximum(rho, u[:, None] + u[None, :] + 2.0 * np.abs((X * Th[q]) @ X.T))
    return rho


def reference(X, row, K, want_grad=True, exact_exponent=False):
    """Ref(ld, g[n, d], unit_ld, unit_g[n, d], cond_1(R)) of one design; ld and g stay in long double (rounding them to fp64
    would spend up to half a unit), the units and cond_1 are fp64 sizes.  exact_exponent: rho = 0 (the dyadic class)."""
    orc.require_extended_precision()
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    w, Th = orc.unpack_params(row, K, d)
    w2 = np.asarray(w, dtype=LD) ** 2
    wh = w2 / w2.sum()
    Rq = [orc.component_corr(X, Th[q], LD) for q in range(K)]
    R = np.zeros((n, n), dtype=LD)
    for q in range(K):
        R += wh[q] * Rq[q]
    L = orc._chol_lower(R, LD)
    Z = orc._lower_inverse(L, LD)
    A = Z.T @ Z
    ld = LD(2) * np.log(np.diag(L)).sum()
    kappa = orc.cond1(R, A)
    rho = np.zeros((n, n)) if exact_exponent else expanded_magnitude(X, row, K)
    e = EPS * (1.0 + rho)
    aA, aR = np.abs(A.astype(np.float64)), np.abs(R.astype(np.float64))
    E = aR * e
    unit_ld = float((aA * E).sum())
    if not want_grad:
        return Ref(ld, None, unit_ld, None, kappa)
    W = aA @ E @ aA + e * aA                                   # (|A| E |A|)_ij + eps (1 + rho_ij) |A_ij|
    g = np.zeros((n, d), dtype=LD)
    unit_g = np.zeros((n, d))
    for k in range(d):
        x = np.asarray(X[:, k], dtype=LD)
        diff = x[:, None] - x[None, :]                         # x_ik - x_jk, exact in long double; 0 at j = i
        S = np.zeros((n, n), dtype=LD)
        for q in range(K):
            S += (wh[q] * LD(Th[q, k])) * Rq[q]
        g[:, k] = LD(-4) * (A * diff * S).sum(axis=1)
        unit_g[:, k] = 4.0 * (W * np.abs(diff.astype(np.float64)) * S.astype(np.float64)).sum(axis=1)
    return Ref(ld, g, unit_ld, unit_g, kappa)


@functools.lru_cache(maxsize=None)
def case_reference(case, b):
    """The reference of design b of a case: computed once and shared, never changed (the arrays are read-only)."""
    t0 = time.perf_counter()
    designs, row = case_inputs(case)
    ref = reference(designs[b], row, case.K, want_grad=case.cls not in ("logdet", "python"),
                    exact_exponent=case.cls == "dyadic")
    for a in (ref.g, ref.unit_g):
        if a is not None:
            a.setflags(write=False)
    REFERENCE_SECONDS[0] += time.perf_counter() - t0
    return ref


def ratio_ld(ld, ref):
    return float(abs(LD(ld) - ref.ld)) / max(ref.unit_ld, FLOOR)


def ratio_g(g, ref, n_fixed=0):
    """Largest |g - g_ref| / unit_g over the free rows; g: [n - n_fixed, d]."""
    g = np.asarray(g, dtype=np.float64)
    assert g.shape == ref.g[n_fixed:].shape, (g.shape, ref.g.shape, n_fixed)
    r = np.abs(g - ref.g[n_fixed:]).astype(np.float64) / np.maximum(ref.unit_g[n_fixed:], FLOOR)
    return float(np.where(np.isnan(r), np.inf, r).max())


def design_constants():
    """(C_LD, C_G): 32 times the recorded fp64 LAPACK figure, rounded up to a power of two, capped at GRAD_TOL_C."""
    def c(fig):
        return min(2.0 ** math.ceil(math.log2(32.0 * fig)), orc.GRAD_TOL_C)
    return c(orc.DESIGN_LD_LAPACK_MAX), c(orc.DESIGN_GRAD_LAPACK_MAX)


# ----------------------------------------------------------------------------- plain fp64, and the mistakes planted in it
MISTAKES = ("next_row", "drop_sub", "drop_i2", "diag_one", "no_sw", "w_unsquared", "theta_next", "trail_chunk",
            "nfixed_row", "ld_short", "drop_small")


def fp64_restatement(X, row, K, n_fixed=0, mistake=None, X_next=None):
    """(log det R, d log det R / d x of the rows >= n_fixed) in plain fp64: the exponent in the scripts' expanded form
    (oracle.corr_matrix), LAPACK Cholesky and inverse.  mistake: one of MISTAKES, what a wrong kernel would compute --
      next_row     the design's last row read from the next design of the batch (X_next)
      drop_sub     the terms j = i - 1 (the entries parked at Z[i][NP]) dropped; drop_i2: the terms j = i - 2
      diag_one     R_ii forced to 1 where the expanded form gives exp(-rounding)
      no_sw        the gradient without the normalisation 1 / sw
      w_unsquared  the gradient's weights not squared
      theta_next   theta_qk taken from component q + 1
      trail_chunk  dimension d - 2 of the trailing chunk written from the clamped kk = d - 1
      nfixed_row   the output rows taken from one row too early
      ld_short     the log det of the first n - 1 rows
      drop_small   the one pair of entries of R nearest to e^-20 left out (what rel = 1e-8 on the log det lets pass)."""
    X = np.array(X, dtype=np.float64)
    n, d = X.shape
    if mistake == "next_row":
        X[-1] = X_next[-1]
    w, Th = orc.unpack_params(row, K, d)
    w2 = w ** 2
    sw = w2.sum()
    Rq = [orc.corr_matrix(X, Th[q]) for q in range(K)]
    if mistake == "diag_one":
        for M in Rq:
            np.fill_diagonal(M, 1.0)
    R = None
    for q in range(K):
        R = w2[q] * Rq[q] if R is None else R + w2[q] * Rq[q]
    R = R / sw
    if mistake == "drop_small" and n > 1:
        off = np.where(np.eye(n, dtype=bool), np.inf, np.abs(np.log(np.maximum(R, 1e-300)) + 20.0))
        a, b = np.unravel_index(np.argmin(off), off.shape)
        if off[a, b] <= 5.0:                                   # a design with no entry in e^-25 .. e^-15 has nothing to drop
            for M in Rq + [R]:
                M[a, b] = M[b, a] = 0.0
    A, ld = orc._chol_inverse(R, np.float64)
    if mistake == "ld_short" and n > 1:
        ld = orc._chol_inverse(R[:n - 1, :n - 1], np.float64)[1]
    wg = (w if mistake == "w_unsquared" else w2) * (1.0 if mistake == "no_sw" else 1.0 / sw)
    Thg = np.roll(Th, -1, axis=0) if mistake == "theta_next" else Th
    S = np.einsum("q,qk,qij->ijk", wg, Thg, np.stack(Rq))
    T = A[:, :, None] * (X[:, None, :] - X[None, :, :]) * S
    if mistake in ("drop_sub", "drop_i2"):
        i, j = np.indices((n, n))
        T[np.abs(i - j) == (1 if mistake == "drop_sub" else 2)] = 0.0
    g = -4.0 * T.sum(axis=1)
    if mistake == "trail_chunk" and d >= 2 and (d - 2) // 8 == (d - 1) // 8:
        g[:, d - 2] = g[:, d - 1]
    if mistake == "nfixed_row" and n_fixed >= 1:
        return ld, g[n_fixed - 1:n - 1]
    return ld, g[n_fixed:]
