"""Who owns the scheduler's time account (ccgp_last_sched_profile, CCGP_OPT_SCHED_POLICY bit 2).  The account lies inside
the memory of the sweep that wrote it -- the handle's workspace, or a factor set --, so whoever frees that memory forgets
the account, and a scheduled sweep without bit 2 leaves none: the call then reports 0 workgroups and copies nothing,
where it used to copy from freed memory or hand back rows nobody wrote.  One scheduled sweep per case, at SCHED_CASE of
tests/test_gpu_marginal_exact.py; each case has a handle of its own, since the session's may already hold a workspace too
large to grow."""
import numpy as np
import pytest

from test_gpu_marginal_exact import SCHED_CASE, make_case

pytestmark = pytest.mark.gpu

N, D, K, B = SCHED_CASE
NT = (N + 127) // 128
TASKS = NT + sum(NT - 1 - j for j in range(1, NT)) + sum(NT - j for j in range(NT))   # per matrix, as tests/test_gpu_sched.py counts them


@pytest.fixture()
def own_handle():
    from ccgp_amd import api
    h = api.Handle(0)
    h.set_option(api.OPT_SCHED, 1)
    yield h
    h.close()


def test_workspace_growth_forgets_the_account(own_handle):
    from ccgp_amd import api
    h = own_handle
    X, y, rows = make_case(N, D, K, B)
    h.set_option(api.OPT_SCHED_POLICY, 11 | 4)
    h.loglik_batch(X, y, K, rows, 1.0)
    acc = h.last_sched_profile()
    assert acc.shape[0] > 0 and acc.shape[1] == 8
    assert acc[:, 5].sum() == TASKS * B
    before = h.workspace_bytes()[0]
    h.set_option(api.OPT_SCHED, 0)
    h.loglik_batch(X, y, K, np.tile(rows, (8, 1)), 1.0)          # B = 24: the workspace of 3 matrices does not hold them
    assert h.workspace_bytes()[0] > before
    assert h.last_sched_profile().shape == (0, 8)


def test_freeing_the_factor_set_forgets_the_account(own_handle):
    from ccgp_amd import api
    h = own_handle
    X, y, rows = make_case(N, D, K, B)
    h.set_option(api.OPT_SCHED_POLICY, 11 | 4)
    fs = h.factor_batch(X, y, K, rows, 1.0)
    acc = h.last_sched_profile()
    assert acc.shape[0] > 0 and acc[:, 5].sum() == TASKS * B     # the sweep ran inside the set's memory
    fs.free()
    assert h.last_sched_profile().shape == (0, 8)


def test_a_sweep_without_bit_2_leaves_no_account(own_handle):
    from ccgp_amd import api
    h = own_handle
    X, y, rows = make_case(N, D, K, B)
    h.set_option(api.OPT_SCHED_POLICY, 11)
    ll, _, st = h.loglik_batch(X, y, K, rows, 1.0)
    assert np.isfinite(ll).all() and not st.any()
    assert h.last_sched_profile().shape == (0, 8)
