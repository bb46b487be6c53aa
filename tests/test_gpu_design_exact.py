"""The max-entropy design criteria on the device against an exact reference: ccgp_mixed_logdet_designs and
ccgp_mixed_logdet_grad_designs (small_reg_kernel, INV = 3) through the handle, and CombinedGP.Entropy, Entropy_batch and
Augmented_Mixed_Entropy built on them.  These are the only calls that read one design per batch entry (x_stride != 0).

Reference, bands, constants and the case list are tests/design_exact.py's (its docstring states them; nothing in them comes
from a device run, and tests/test_design_exact_host.py shows on the CPU that the bands reject a wrong row, a dropped
sub-diagonal or i - 2 term, a missing 1 / sw, an unsquared weight, a theta of the wrong component, a clamped dimension
written, an output row off by one and a log det one row short, each by far more than 4 C):

    |ld_dev - ld_ref| <= C_LD unit_ld,    |g_dev[i,k] - g_ref[i,k]| <= C_G unit_g[i,k],    C_LD = 8, C_G = 16,

status 0 everywhere, cond_1(R) <= KAPPA_MAX asserted for every design from the long-double inverse.  One test per case class;
the comment beside each class in design_exact.py names the lines of csrc/small_reg.hip it is aimed at.  Every gradient case
also sends its designs through ccgp_mixed_logdet_designs (another kernel instance: the factorising one, four designs per
workgroup on the 8 x 8 grid), whose log det is held to the same band.

Route: the gradient exists on the register evaluator only (design_exact.design_grad_route says `r` for every shape, asserted
on the host too).  The log det's tier is asserted by the timing counters as in tests/test_gpu_routes.py (`fused` for the
register evaluator, `diag` / `update` for the blocked sweep); inside the register evaluator the counters cannot tell the
instances apart, csrc/small_reg.hip dispatch() decides by n and by the per-design carve, restated in design_exact.
logdet_instance: reg8 (n <= 64), wave (NB 9..13), reg16.

The python class: -exp(ld) has the relative error |ld_dev - ld_ref| + 2 eps (the host's exp and its rounding), the Schur
ratio -exp(ld_all - ld_old) the sum of the two log dets' errors + eps (|ld_all - ld_old| + 2) (the subtraction's rounding as
well).

Measured on an MI355X after the bands were fixed (test_zz_report_headroom prints the table; nowhere asserted): the log det
uses at most 0.37 of its 8 units (the 8 x 8 grid and the gradient call at the `instances`; 0.036 on the blocked sweep), the
gradient at most 0.44 of its 16 (`position`); DESIGN.md, `Design criteria: the exact yardstick`, has the table per class.
"""
import numpy as np
import pytest

import design_exact as dx
from test_gpu_gradient_exact import KAPPA_MAX, _bits, _timed

pytestmark = pytest.mark.gpu

EPS = dx.EPS
C_LD, C_G = dx.design_constants()
MAX_RATIO = {}                      # (class, route, `ld` | `g`) -> largest |dev - ref| / unit seen


def _ids(cases):
    return ["n%d-d%d-K%d" % c for c in cases]


def _small(t):
    assert t["fused"][1] > 0 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t


def _blocked(t, n):
    assert t["fused"][1] == 0 and t["diag"][1] > 0 and (n <= 128 or t["update"][1] > 0), t


def _note(cls, route, what, ratio):
    key = (cls, route, what)
    MAX_RATIO[key] = max(MAX_RATIO.get(key, 0.0), ratio)


def check_ld(case, b, route, ld, st):
    ref = dx.case_reference(case, b)
    assert ref.kappa <= KAPPA_MAX, (case, b, ref.kappa)
    assert st == 0, (case, b, route, st)
    r = dx.ratio_ld(ld, ref)
    print("%s design %d %s: ld %.17g ref %.17g  %.3g units (cond1 %.3g)" % (case, b, route, ld, float(ref.ld), r, ref.kappa))
    _note(case.cls, route, "ld", r)
    assert r <= C_LD, (case, b, route, ld, float(ref.ld), r)


def check_grad(case, b, g, n_fixed=0):
    ref = dx.case_reference(case, b)
    r = dx.ratio_g(g, ref, n_fixed)
    print("%s design %d n_fixed %d: gradient %.3g units" % (case, b, n_fixed, r))
    _note(case.cls, "grad", "g", r)
    if not r <= C_G:
        bad = np.argwhere(~(np.abs(g - ref.g[n_fixed:]).astype(np.float64) <= C_G * np.maximum(ref.unit_g[n_fixed:], dx.FLOOR)))
        raise AssertionError((case, b, n_fixed, r, bad[:4].tolist()))


def run_case(handle, case, n_fixed=0):
    """The case's designs through both entry points; every design inside its bands.  Returns (ld of the gradient call, g)."""
    designs, row = dx.case_inputs(case)
    assert dx.design_grad_route(case.n, case.d, case.K) == "r"
    (ld, g, st), t = _timed(handle, lambda: handle.mixed_logdet_grad_designs(designs, case.K, row, n_fixed))
    _small(t)
    assert g.shape == (case.B, case.n - n_fixed, case.d)
    (ld2, st2), t2 = _timed(handle, lambda: handle.mixed_logdet_designs(designs, case.K, row))
    inst = dx.logdet_instance(case.n, case.d, case.K)
    assert inst != "blocked"
    _small(t2)
    for b in range(case.B):
        check_ld(case, b, "grad", ld[b], st[b])
        check_grad(case, b, g[b], n_fixed)
        check_ld(case, b, inst, ld2[b], st2[b])
    return ld, g


@pytest.mark.parametrize("n,d,K", dx.INSTANCES, ids=_ids(dx.INSTANCES))
def test_instances(handle, n, d, K):
    """Every NB of dispatch_inv<3> at its first, last and one-past size."""
    run_case(handle, dx.Case("instances", n, d, K, 2))


@pytest.mark.parametrize("n,d,K", dx.CHUNKS, ids=_ids(dx.CHUNKS))
def test_chunks(handle, n, d, K):
    """The dimension chunks of pass 2, the clamped lanes of the last one, and the second trip of its item loop."""
    run_case(handle, dx.Case("chunks", n, d, K, 2))


@pytest.mark.parametrize("n,d,K", dx.FIXED, ids=_ids(dx.FIXED))
def test_fixed(handle, n, d, K):
    """n_fixed at 0, 1, 2, 15, 16, 17, n - 2, n - 1: the free rows against the reference of the whole design, the log det the
    bits of the n_fixed = 0 call."""
    case = dx.Case("fixed", n, d, K, 2)
    ld0, _ = run_case(handle, case, 0)
    for nf in dx.fixed_values(n)[1:]:
        ld, _ = run_case(handle, case, nf)
        assert np.array_equal(_bits(ld), _bits(ld0)), nf


@pytest.mark.parametrize("n,d,K", dx.DYADIC, ids=_ids(dx.DYADIC))
def test_dyadic(handle, n, d, K):
    """Inputs on which the expanded exponent is exact: held with rho = 0."""
    run_case(handle, dx.Case("dyadic", n, d, K, 2))


@pytest.mark.parametrize("n,d,K", dx.POSITION, ids=_ids(dx.POSITION))
def test_position(handle, n, d, K):
    """70 pairwise different designs: each inside its own bands sent alone, and each with the bits of that call in batches of
    1, 3, 5 and 70 rotated through the four sub-matrix slots of a workgroup, for both entry points."""
    case = dx.Case("position", n, d, K, max(dx.POSITION_B))
    designs, row = dx.case_inputs(case)
    inst = dx.logdet_instance(n, d, K)
    alone = []
    for b in range(case.B):
        ld, g, st = handle.mixed_logdet_grad_designs(designs[b:b + 1], K, row, 0)
        ld2, st2 = handle.mixed_logdet_designs(designs[b:b + 1], K, row)
        check_ld(case, b, "grad", ld[0], st[0])
        check_grad(case, b, g[0])
        check_ld(case, b, inst, ld2[0], st2[0])
        alone.append((ld[0], g[0], ld2[0]))
    for B in dx.POSITION_B:
        for shift in range(min(B, 4)):
            idx = np.roll(np.arange(B), shift)
            ld, g, st = handle.mixed_logdet_grad_designs(designs[idx], K, row, 0)
            ld2, st2 = handle.mixed_logdet_designs(designs[idx], K, row)
            assert not st.any() and not st2.any()
            for pos, b in enumerate(idx):
                assert _bits(ld[pos]) == _bits(alone[b][0]), (B, shift, pos)
                assert np.array_equal(_bits(g[pos]), _bits(alone[b][1])), (B, shift, pos)
                assert _bits(ld2[pos]) == _bits(alone[b][2]), (B, shift, pos)


@pytest.mark.parametrize("n,d,K", dx.LOGDET, ids=_ids(dx.LOGDET))
def test_logdet(handle, n, d, K):
    """ccgp_mixed_logdet_designs alone on each of its instances, B = 2."""
    case = dx.Case("logdet", n, d, K, 2)
    designs, row = dx.case_inputs(case)
    inst = dx.logdet_instance(n, d, K)
    (ld, st), t = _timed(handle, lambda: handle.mixed_logdet_designs(designs, K, row))
    (_blocked(t, n) if inst == "blocked" else _small(t))
    for b in range(2):
        check_ld(case, b, inst, ld[b], st[b])


def test_python(handle):
    """CombinedGP.Entropy, Entropy_batch and Augmented_Mixed_Entropy at the 14- and 14 + 7-point shapes."""
    from ccgp_amd.rsurface import CombinedGP
    gp = CombinedGP("BSQ", handle=handle)
    p, t1, t2 = dx.PYTHON_PRIOR
    D14, _ = dx.case_inputs(dx.PYTHON_14)
    D21, _ = dx.case_inputs(dx.PYTHON_21)
    refs = [dx.case_reference(dx.PYTHON_14, b) for b in range(dx.PYTHON_14.B)]
    ref21 = dx.case_reference(dx.PYTHON_21, 0)
    assert max(r.kappa for r in refs + [ref21]) <= KAPPA_MAX

    def held(got, ld_ref, rel, tag):
        want = -np.exp(ld_ref)
        r = float(abs(np.longdouble(got) - want) / abs(want)) / rel
        print("%s: %.17g ref %.17g  %.3g of its band / C" % (tag, got, float(want), r * C_LD))
        _note("python", tag, "ld", r * C_LD)
        assert r <= 1.0, (tag, got, float(want), r)

    got = gp.Entropy_batch(D14, p, t1, t2)
    for b, ref in enumerate(refs):
        held(got[b], ref.ld, C_LD * ref.unit_ld + 2.0 * EPS, "Entropy_batch")
    held(gp.Entropy(D14[3], p, t1, t2), refs[3].ld, C_LD * refs[3].unit_ld + 2.0 * EPS, "Entropy")
    held(gp.Entropy(D21[0], p, t1, t2), ref21.ld, C_LD * ref21.unit_ld + 2.0 * EPS, "Entropy")
    diff = ref21.ld - refs[0].ld
    held(gp.Augmented_Mixed_Entropy(D14[0], D21[0, 14:], p, t1, t2), diff,
         C_LD * (ref21.unit_ld + refs[0].unit_ld) + EPS * (abs(float(diff)) + 2.0), "Augmented_Mixed_Entropy")


def test_zz_report_headroom():
    """Largest observed |dev - ref| / unit per class and route, against C_LD = 8 (`ld`) and C_G = 16 (`g`), and the host time
    the references took."""
    for k in sorted(MAX_RATIO):
        print("max ratio %-10s %-24s %-2s %.3g of %g" % (k + (MAX_RATIO[k], C_G if k[2] == "g" else C_LD)))
    print("references: %.2f s of host time" % dx.REFERENCE_SECONDS[0])
    assert dx.REFERENCE_SECONDS[0] <= dx.REFERENCE_SECONDS_MAX
