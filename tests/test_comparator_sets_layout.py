"""The sets forms of the comparator fits on the CPU: tests/host_small/comparator_sets_layout_check.cpp walks
small_route_profile_grad_sets over n 1..129, every d, K and kernel family (one launch exactly where the family is Gaussian and
the single-set gradient takes the register-resident instance: the tier boundary and the carve are summed by hand in the
program), pins the dynamic LDS total of the eight new instances, and checks that the pieces of profile_sets_stage and
cgp_sets_stage (csrc/call_stage.h) tile a chunk's buffer in order without overlap, the sets in front and pushed with the first
chunk only.  Built plain for both exp settings, and once as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (the program writes every byte of every staged piece)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "comparator_sets_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
# one-launch / grouped cells over (n 1..129) x (d 1..64) x (K 1..8) x 3 families, and the Gaussian shapes of the in-LDS tier
# whose gradient instance does not fit (they go set by set); exp table off / on
COUNTS = {0: (58609, 139535, 2711), 1: (58093, 140051, 3227)}
# dynamic LDS in bytes of small_reg_kernel<16, NB, NB + 1, false, 2, false, true, true>, NB = 1 .. 8, at (n, d, K) =
# (5,1,1) (17,2,1) (48,4,2) (50,9,1) (80,3,2) (96,2,3) (105,2,2) (128,3,3): 8 (d n + K NP + K d + K + 2 (NP + 16 (NB + 1)) + 3 NP
# + 8 + 1 + NP (NP + 2) + 112) with NP = 16 NB, e.g. NB = 4 at (50,9,1): 8 (450 + 64 + 9 + 1 + 288 + 192 + 9 + 4224 + 112) = 42792
LDS = {0: [4608, 12272, 25496, 42792, 61448, 85776, 113160, 147752]}
LDS[1] = [b + 2048 for b in LDS[0]]


@pytest.mark.parametrize("table,flags", [(0, []), (1, []), (0, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["poly", "table", "sanitized"])
def test_route_lds_and_staging(table, flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "comparator_sets_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    words = lines[-3].split()
    assert (int(words[1]), int(words[3]), int(words[5])) == COUNTS[table]
    assert int(words[1]) + int(words[3]) == 129 * 64 * 8 * 3
    assert [int(w) for w in lines[-2].split()[1:]] == LDS[table]
    assert max(LDS[table]) <= 160 * 1024 - 64
