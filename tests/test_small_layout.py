"""The LDS carves and route predicates of the small-n evaluators (csrc/small_layout.h) executed on the CPU:
tests/host_small/small_layout_check.cpp walks n 1..128, d 1..64, K 1..8 and every kernel instance the dispatchers of
csrc/small_reg.hip can form.  Per build setting (CCGP_SMALL_EXP_TABLE 0 and 1) it holds that every carve's regions are in
order, disjoint and inside `total`, zmat is 16-byte aligned, the factor block's pieces are 8-word aligned, and every total
and predicate equals the hand-summed formula it replaced (written out in the check program).

Routes.  No accepted shape has the in-LDS tier (csrc/small.hip) fit while the register-resident evaluator does not, for
the likelihood or for prediction: those two in-LDS routes are gone.  small.hip is still reached by the gradient at 2711
shapes (3227 with the exp table) and by solve(R) of ccgp_logpost, K = 2, at 235 (d, n) pairs (296): counted twice by the
check program, once from small_route and once from the replaced formulas, and pinned here.

small_route (which tier serves which call) is held by the same program to the route expressions the entry points carried
before it, over n 1..129, both kernel families and all six ops; prediction's route equals ccgp_factor_batch's former
`fused` on every shape.  Pinned here: the shapes at which ccgp_reserve now reserves the sweep's workspace and did not
before, and one witness shape per reachable (op, route) cell (tests/route_witnesses.py, which tests/test_gpu_routes.py
runs on the device)."""
import os
import shutil
import subprocess

import pytest

import route_witnesses
import test_gpu_gradient_exact as grad_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "small_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
LDS_ROUTE_COUNTS = {0: (2711, 235), 1: (3227, 296)}      # exp table off / on: (gradient, solve(R) at K = 2)


_RUNS = {}


def _run(table, tmp_path_factory, mode="table"):
    """stdout lines of the check program built with CCGP_SMALL_EXP_TABLE = table (one build per setting, one run per mode)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if table not in _RUNS:
        exe = str(tmp_path_factory.mktemp("small_layout") / "small_layout_check")
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, "-I", CSRC, SRC,
                        "-o", exe], check=True)
        _RUNS[table] = {"exe": exe}
    if mode not in _RUNS[table]:
        r = subprocess.run([_RUNS[table]["exe"], mode], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
        _RUNS[table][mode] = r.stdout.splitlines()
    return _RUNS[table][mode]


@pytest.mark.parametrize("table", [0, 1], ids=["poly", "table"])
def test_carves_and_predicates(table, tmp_path_factory):
    lines = _run(table, tmp_path_factory)
    assert lines[-1] == "ok"
    words = lines[-2].split()
    assert words[0] == "dead" and (int(words[1]), int(words[2])) == (0, 0)
    assert (int(words[4]), int(words[6])) == LDS_ROUTE_COUNTS[table]


@pytest.mark.parametrize("table", [0, 1], ids=["poly", "table"])
def test_route_function_counts_and_witnesses(table, tmp_path_factory):
    """The exhaustive equality of small_route with the replaced expressions is the program's exit status (_run); here the
    counts of its `reserve` line and the witness list."""
    words = _run(table, tmp_path_factory)[-3].split()
    assert words[0] == "reserve" and words[3] == "predict_outside_lds"
    assert (int(words[1]), int(words[2])) == route_witnesses.RESERVE_CHANGES[table]
    assert int(words[4]) == route_witnesses.PREDICT_OUTSIDE_LDS[table]
    got = [(w[0], w[1], int(w[2]), int(w[3]), int(w[4])) for w in (l.split() for l in _run(table, tmp_path_factory, "witness"))]
    assert got == route_witnesses.WITNESSES[table]


def test_python_mirrors_of_the_route_predicates(tmp_path_factory):
    """small_lds_bytes, small_reg_inverse_supported and route of tests/test_gpu_gradient_exact.py (which mirror the default
    build: no exp table) against the header, shape by shape."""
    rows = _run(0, tmp_path_factory)[:-3]
    assert len(rows) == 128 * 64
    name = {"b": "blocked", "r": "reg", "l": "lds"}
    for line in rows:
        n, d, lds1, inv, routes = line.split()
        n, d = int(n), int(d)
        assert grad_routes.small_lds_bytes(n, d, 1) == int(lds1), (n, d)
        for K in range(1, 9):
            assert grad_routes.small_reg_inverse_supported(n, d, K) == (inv[K - 1] == "1"), (n, d, K)
            assert grad_routes.route(n, d, K) == name[routes[K - 1]], (n, d, K)
