"""The fused family evaluators' domain and routes on the CPU: tests/host_small/family_fused_layout_check.cpp walks n 1..40,
d 1..3, K 1..4 and the three kernel families and holds small_family_fused_supported (csrc/small_layout.h) to its stated domain
-- family 1 or 2, d = 1, 1 <= n <= 32, K = 2 for the two-family kernel --, the four route functions that take
CCGP_OPT_FAMILY_FUSED (Op::Loglik, sets, chain, search) to Reg there when called as capi.hip calls them with the option on, and
the same functions under the plain `gauss` flag to what they said before the option existed.  Built plain for both exp settings,
and once as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "family_fused_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
CELLS = 3 * 40 * 3 * 4
# the domain inside the walk: Matern at d = 1, n 1..32, K 1..4, and Matern + spline at d = 1, n 1..32, K = 2
SUPPORTED = 32 * 4 + 32
# dynamic LDS in bytes of the largest instance of the walk, the search at n = 32 (NB = 2), d = 1, K = 4:
#   8 (32 + 4 x 32 + 4 + 4 + 2 (32 + 16) + 32 + 2 x 32 + 8 + 526 + 54) = 8 x 948; the exp table adds 256 doubles
LDS = {0: 7584, 1: 7584 + 2048}


@pytest.mark.parametrize("table,flags", [(0, []), (1, []), (0, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["poly", "table", "sanitized"])
def test_domain_and_routes(table, flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "family_fused_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    w = lines[-2].split()
    got = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    assert got == dict(cells=CELLS, supported=SUPPORTED, gauss=CELLS // 3, kept=2 * CELLS // 3 - SUPPORTED, lds=LDS[table])
