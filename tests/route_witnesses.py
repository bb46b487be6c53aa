"""One shape per reachable (op, route) cell of csrc/small_layout.h's small_route, Gaussian family: the shape with the
smallest n, then d, then K, as tests/host_small/small_layout_check.cpp prints them in its `witness` mode.  Pinned against
that program by tests/test_small_layout.py (which needs a compiler) and run on the device by tests/test_gpu_routes.py
(which does not).  Routes: r = register-resident evaluator, l = in-LDS evaluator (small.hip), b = blocked sweep,
u = refused.  `inverse` (solve(R) of ccgp_logpost) is walked at K = 2, the only K that entry point has.  Keyed by the
build setting CCGP_SMALL_EXP_TABLE; 0 is the default build.

`reserve`: the first shape at which ccgp_reserve(..., m > 0) reserves the sweep's workspace and did not before
small_route: a Gaussian n <= 128 shape whose prediction takes the blocked sweep.  The counts below are of those shapes
over n 1..129, d 1..64, K 1..8 and both families, without test sites (m = 0: none, because no Gaussian n <= 128
likelihood takes the sweep) and with them."""

_HEAD = [("loglik", "r", 1, 1, 1), ("predict", "r", 1, 1, 1), ("grad", "r", 1, 1, 1), ("logdet_designs", "r", 1, 1, 1),
         ("design_grad", "r", 1, 1, 1), ("inverse", "r", 1, 1, 2), ("logdet_designs", "b", 49, 63, 8)]
_TAIL = [("predict", "b", 108, 63, 1), ("grad", "b", 108, 63, 1), ("reserve", "b", 108, 63, 1), ("inverse", "b", 108, 63, 2),
         ("loglik", "b", 129, 1, 1)]

WITNESSES = {
    0: _HEAD + [("design_grad", "u", 81, 56, 8), ("grad", "l", 97, 56, 8), ("inverse", "l", 101, 64, 2)] + _TAIL,
    1: _HEAD + [("design_grad", "u", 81, 55, 8), ("grad", "l", 97, 54, 8), ("inverse", "l", 97, 64, 2)] + _TAIL,
}
RESERVE_CHANGES = {0: (0, 4216), 1: (0, 4216)}      # (m = 0, m > 0)
PREDICT_OUTSIDE_LDS = {0: 4216, 1: 4216}            # n <= 128 shapes whose prediction instance fits but small.hip's carve does not
