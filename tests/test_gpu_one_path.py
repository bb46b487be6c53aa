"""The host arithmetic the single-set and the sets entry points share (capi.hip: the log posterior's wrapper, the chunked
call, the CGP state call), where the other tests do not already hold it.  Every comparison is on bytes.

Held elsewhere: ccgp_logpost_sets against ccgp_logpost_batch for C >= 3 on passing rows
(test_gpu_sets.py::test_logpost_sets_is_logpost_batch_per_set), ccgp_logpost_batch against ccgp_logpost
(test_gpu_parity.py), the sets rows against the single-set calls for C >= 2 and the cut into chunks
(test_gpu_comparator_sets.py, test_gpu_cgp.py).  New here: the three log-posterior calls against each other INCLUDING a row
whose factorisation fails -- one failing row among passing ones with C = 2, and C = 1 on the failing set itself -- and
every sets call with C = 1.

A failing row lies on a set with two coincident design points, the integer grid and the scales 2048 / 4096 of
tests/exact_designs.py: its correlation matrix is 0 / 1 to the bit, so the second pivot is exactly 0."""
import numpy as np
import pytest

import exact_designs as ex
from conftest import synthetic_design
from ccgp_amd import api, cgp
from test_gpu_cgp import rows_in_the_box
from test_gpu_failure_contract import _Returned
from test_gpu_random_shapes import draws

pytestmark = pytest.mark.gpu
N, B = 6, 5
PRIORS = [("INVGAMMA", 2, (7.0, 3.0, 3.0, 28.0)), ("GV", 3, None), ("ISO", 2, None), ("ANI", 2, None)]


def _logpost_case(d, q, layout):
    """B = 5 transformed rows on sets of n = 6.  "clean": one set, every row passes.  "mixed": two sets, row 2 alone on the
    second, the grid with point 2 on point 1.  "coincident": that grid as the ONE set, so every row fails, at pivot 2."""
    X0, y0 = synthetic_design(N, d, 30 + d)
    dup = np.zeros((N, d))
    dup[:, :2] = ex.duplicate_designs(N)[0][0]
    sets = {"clean": [(X0, y0, 1.3)], "mixed": [(X0, y0, 1.3), (dup, np.cos(np.arange(N)), 0.8)],
            "coincident": [(dup, np.cos(np.arange(N)), 0.8)]}[layout]
    rng = np.random.default_rng(q)
    T = np.stack([np.log(rng.uniform(0.5, 3.0, B)), np.log(rng.uniform(2.0 * N, 4.0 * N, B)), rng.normal(0.0, 0.8, B)] +
                 ([rng.normal(0.0, 0.3, B)] if q == 4 else []), axis=1)
    T[2, :2] = np.log(ex.THETA)
    set_of = np.zeros(B, dtype=np.int32)
    set_of[2] = len(sets) - 1
    fails = {"clean": [], "mixed": [2], "coincident": list(range(B))}[layout]
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]), np.array([s[2] for s in sets]), T, set_of, fails


@pytest.mark.parametrize("layout", ["clean", "mixed", "coincident"])
@pytest.mark.parametrize("prior,d,pars", PRIORS, ids=[p[0] for p in PRIORS])
def test_the_three_log_posterior_calls_agree_to_the_bit(handle, prior, d, pars, layout):
    pid = getattr(api, "PRIOR_" + prior)
    Xs, ys, s2, T, set_of, fails = _logpost_case(d, 4 if prior == "ANI" else 3, layout)
    with _Returned(handle) as r:
        got = handle.logpost_sets(Xs, ys, s2, pid, T, set_of, pars)
    failed = r.rcs[0]
    assert failed == len(fails) and np.flatnonzero(got[3]).tolist() == fails
    for b in fails:
        assert got[3][b] == 2 and all(np.isnan(got[k][b]) for k in range(3))
    batch_failed = row_failed = 0
    for c in range(len(Xs)):
        rows = np.flatnonzero(set_of == c)
        with _Returned(handle) as r:
            want = handle.logpost_batch(Xs[c], ys[c], s2[c], pid, T[rows], pars)
        batch_failed += r.rcs[0]
        for g, w in zip(got, want):
            assert g[rows].tobytes() == w.tobytes()
        for b in rows:
            with _Returned(handle) as r:
                one = handle.logpost(Xs[c], ys[c], s2[c], pid, T[b], pars, want_Rinv=False)
            row_failed += r.rcs[0]
            for g, k in zip(got, ("val", "beta", "loglik", "status")):
                assert np.asarray(g[b]).tobytes() == np.asarray(one[k], dtype=g.dtype).tobytes(), (b, k)
    assert batch_failed == failed and row_failed == failed


@pytest.fixture(scope="module")
def one_set():
    X, y = synthetic_design(N, 2, 77)
    return X, y


@pytest.mark.parametrize("grad", [True, False])
def test_profile_sets_with_one_set_is_the_single_set_call(handle, one_set, grad):
    X, y = one_set
    P = draws(np.random.default_rng(3), N, 2, 2, 7)
    got = handle.profile_batch_sets(X[None], y[None], 2, P, np.zeros(7, dtype=np.int32), grad=grad)
    want = handle.profile_batch(X, y, 2, P, grad=grad)
    assert not want[4].any() and (got[3] is None) == (not grad)
    for g, w in zip(got, want):
        assert g is None and w is None or g.tobytes(order="A") == w.tobytes(order="A")


@pytest.mark.parametrize("with_skip", [True, False])
def test_cgp_state_sets_with_one_set_is_the_single_set_call(handle, one_set, with_skip):
    X, y = one_set
    Xs, _ = cgp.standardise(X)
    P = rows_in_the_box(Xs, 7, 9)
    skip = np.array([-1, 0, 5, -1, 3, 2, -1], dtype=np.int32) if with_skip else None
    got = handle.cgp_state_batch_sets(Xs[None], y[None], P, np.zeros(7, dtype=np.int32), skip=skip)
    want = handle.cgp_state_batch(Xs, y, P, skip=skip)
    assert not want[4].any() and (got[3] is None) == (not with_skip)
    for g, w in zip(got, want):
        assert g is None and w is None or g.tobytes() == w.tobytes()
