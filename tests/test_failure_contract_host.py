"""Host side of the failure-contract tests (no GPU): the exact-design fixture of tests/exact_designs.py really has the
statuses it derives -- by a plain numpy LDL', by the fp64 oracle and by the compiled CPU evaluator -- and the shared
checker rejects every way a device route could break the contract."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_designs as ex
from oracle import ccgp_oracle as orc
from oracle.cpu_baseline import loader as cpu


def _unique(rows, exp):
    _, first = np.unique(rows, axis=0, return_index=True)
    return [(rows[i], int(exp[i])) for i in sorted(first)]


@pytest.mark.parametrize("D,K,zero_sets", [pytest.param(D, K, z, id="n%d-d%d-K%d-B%d" % (D.n, D.d, K, len(z)))
                                           for D, K, z in ex.all_designs()])
def test_fixture_fails_where_it_says(D, K, zero_sets):
    rows, exp = D.draws(K, zero_sets)
    assert exp[0] != 0 and exp[-1] != 0 and exp[len(exp) // 2] != 0 and (exp == 0).any()     # failed draws first, middle, last
    D.guard(K, rows)
    n, sigma2 = D.n, ex.mode1_sigma2(K)
    for row, want in _unique(rows, exp):
        w, Th = orc.unpack_params(row, K, D.d)
        R = orc.mixed_corr_matrix_general(D.X, w, Th)
        # both thresholds of pivot_tolerance: mean mode 1 (0) and mean mode 0 (n eps)
        assert ex.first_bad_pivot(R, 0.0) == want and ex.first_bad_pivot(R, n * ex.EPS) == want
        if want == 0:
            assert np.array_equal(R, np.eye(n))
        for mode in (0, 1):
            try:
                ll, beta = orc.loglik_general(D.X, D.y, w, Th, sigma2, mode, 0.0)
            except np.linalg.LinAlgError:
                ll = float("nan")
            assert math.isnan(ll) == (want != 0), (mode, want, ll)
            if want == 0:
                c_ll, c_beta, b_ll, b_beta = ex.identity_closed_forms(D.y, sigma2, K, mode)
                assert abs(ll - c_ll) <= b_ll and abs(beta - c_beta) <= b_beta
    # the compiled CPU evaluator reports the same status (built-in Cholesky up to n = 128, LAPACK dpotrf beyond)
    urows = np.stack([r for r, _ in _unique(rows, exp)])
    uexp = np.array([e for _, e in _unique(rows, exp)])
    for mode in (0, 1):
        ll, beta, st = cpu.loglik_batch(D.X, D.y, K, urows, sigma2, mode, 0.0)
        assert np.array_equal(st, uexp), (mode, st, uexp)
        assert np.isnan(ll[uexp != 0]).all() and np.isfinite(ll[uexp == 0]).all()


def test_duplicate_designs_fail_where_they_say():
    designs, K, row, exp = ex.duplicate_designs()
    assert np.array_equal(designs[0], designs[3]) and exp[0] != 0 and exp[-1] != 0 and exp[2] != 0
    w, Th = orc.unpack_params(row, K, 2)
    for X, want in zip(designs, exp):
        R = orc.mixed_corr_matrix_general(X, w, Th)
        assert np.isin(R, (0.0, 1.0)).all()
        assert ex.first_bad_pivot(R, 0.0) == want
        assert (np.linalg.slogdet(R)[1] == 0.0) if want == 0 else (np.linalg.matrix_rank(R) < len(R))


def test_sites_are_on_or_far():
    D = ex.ExactDesign(64, ex.predict_seps(64))
    Xt, on = D.sites(65, 64)
    assert sorted(np.nonzero(on >= 0)[0]) == [0, 63, 64] and len(set(on[on >= 0])) == 3
    row = D.row(2)
    for t in range(65):
        r = orc.mixed_corr_vec_general(Xt[t], D.X, *orc.unpack_params(row, 2, D.d))
        want = np.zeros(64)
        if on[t] >= 0:
            want[on[t]] = 1.0
        assert np.array_equal(r, want)


def test_kept_factor_mirrors_match_the_layout_header(tmp_path):
    """The Python mirrors through which the device tests assert the kept-factor scheme and its chunk of draws, against
    csrc/small_layout.h itself (compiled on the host), over n 1..128 at several d, K and m."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import test_gpu_failure_contract as dev
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "convex-combination-of-gaussian-processes_amd", "csrc")
    exe = str(tmp_path / "sites_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", csrc,
                    os.path.join(root, "tests", "host_small", "sites_plan_check.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    seen = set()
    for line in filter(None, lines):
        n, d, K, m, ok, scratch = (int(v) for v in line.split())
        assert dev.sites_supported(n, d, K) == bool(ok), line
        assert dev.sites_scratch(n, m) == scratch, line
        seen.add(bool(ok))
    assert seen == {True, False}


# ---- the checker rejects each way of breaking the contract ----------------------------------------------------------
def _good():
    """A fabricated batch of 8 (two chunks of 4): draws 0, 3, 5 and 7 fail; draw 5 zeroes pivots 40 and 9."""
    exp = np.array([9, 0, 0, 200, 0, 9, 0, 40], dtype=np.int32)
    rng = np.random.default_rng(0)
    ok = exp == 0
    ref = dict(status=np.zeros(int(ok.sum()), dtype=np.int32), ll=rng.random(4), beta=rng.random(4), grad=rng.random((4, 6)),
               mean=rng.random((4, 5)), var=rng.random((4, 5)))
    out = dict(status=exp.copy())
    for k, v in ref.items():
        if k != "status":
            a = np.full((8,) + v.shape[1:], np.nan)
            a[ok] = v
            out[k] = a
    return exp, out, ref, int(np.count_nonzero(exp))


def test_checker_accepts_a_correct_result():
    ex.check_contract(*_good())


def _status(fn):
    def breaker(exp, out, ref, ret):
        fn(out["status"])
        return exp, out, ref, ret
    return breaker


def _set(name, idx, value):
    def breaker(exp, out, ref, ret):
        out[name][idx] = value
        return exp, out, ref, ret
    return breaker


BREAKERS = {
    "status one too low": _status(lambda st: st.__setitem__(0, 8)),
    "status one too high": _status(lambda st: st.__setitem__(0, 10)),
    "status off by a tile of 128, up": _status(lambda st: st.__setitem__(3, 328)),
    "status off by a tile of 128, down": _status(lambda st: st.__setitem__(3, 72)),
    "last bad pivot instead of the first": _status(lambda st: st.__setitem__(5, 40)),
    # the second chunk's words written from the start of the array (indexed from the chunk, not the batch)
    "status indexed from the chunk start": _status(lambda st: st.__setitem__(slice(None), [0, 9, 0, 40, 0, 0, 0, 0])),
    "failure not reported": _status(lambda st: st.__setitem__(7, 0)),
    "finite ll in a failed draw": _set("ll", 0, 1.5),
    "finite beta in a failed draw": _set("beta", 3, 0.0),
    "one finite gradient component in a failed draw": _set("grad", (5, 4), -2.0),
    "one finite mean in a failed draw": _set("mean", (7, 4), 0.25),
    "one finite variance in a failed draw": _set("var", (0, 0), 0.0),
    "infinity in a failed draw": _set("ll", 7, np.inf),
    "NaN in a passing neighbour": _set("mean", (1, 2), np.nan),
    "a passing neighbour off by one ulp": lambda exp, out, ref, ret: (
        exp, dict(out, ll=np.where(np.arange(8) == 4, np.nextafter(out["ll"], 2.0), out["ll"])), ref, ret),
    "return count one too high": lambda exp, out, ref, ret: (exp, out, ref, ret + 1),
    "return count one too low": lambda exp, out, ref, ret: (exp, out, ref, ret - 1),
}


@pytest.mark.parametrize("name", sorted(BREAKERS))
def test_checker_rejects(name):
    args = BREAKERS[name](*_good())
    with pytest.raises(AssertionError):
        ex.check_contract(*args)
