"""The domain and routes of the 1-D families' profiled mode and analytic gradient on the register-resident evaluator, on the
CPU: tests/host_small/family_fused_grad_layout_check.cpp walks n 1..40, d 1..3, K 1..4 and the three kernel families and holds
small_family_fused_profile_supported and small_family_fused_grad_supported (csrc/small_layout.h) to their stated domain --
family 1 or 2 (K = 2 for the two-family kernel), d = 1, n <= 32 --, small_route(Op::Loglik), small_route(Op::Grad) and
small_route_profile_grad_sets to Reg there when called as capi.hip calls them under CCGP_OPT_FAMILY_FUSED_GRAD, the same functions
under the plain `gauss` flag to what they say without the option, and the carves of the instances those routes launch to the
LDS they may take.  Built plain for both exp settings, and once as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "family_fused_grad_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
CELLS = 3 * 40 * 3 * 4
# inside the walk: Matern at d = 1, n 1..32 with K 1..4; Matern + spline at K = 2
DOMAIN = 32 * 4 + 32
# dynamic LDS in bytes of the largest gradient instance at n = 32, d = 1, K = 4 (the exp table adds 256 doubles):
#   16 x 16 grid:  8 (32 + 128 + 4 + 4 + 160 + 32 + 64 + 8 + 32 x 34 + 1 + 112)
GRAD16 = 8 * 1633


@pytest.mark.parametrize("table,flags", [(0, []), (1, []), (0, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["poly", "table", "sanitized"])
def test_domain_and_routes(table, flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "family_fused_grad_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    w = lines[-2].split()
    got = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert got == dict(cells=CELLS, profile=DOMAIN, grad=DOMAIN, kept=2 * CELLS // 3 - DOMAIN, grad16=GRAD16 + 2048 * table)
