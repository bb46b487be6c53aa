"""The predictions over sets (ccgp_predict_batch_sets, ccgp_krige_predict_batch_sets, ccgp_predict_summary_sets) on the CPU:
tests/host_small/predict_sets_layout_check.cpp walks small_route_predict_sets over n 1..129, every d, K and kernel family (one
set of launches exactly where the family is Gaussian, the single-set call keeps its factor -- n <= 104, K <= 3, its carves fit
-- and the sets instance's carve fits, summed by hand in the program), pins the dynamic LDS of the FAC + SETS instances on
both grids at the eight kept-factor shapes of tests/test_gpu_predict_sets.py, and checks that the pieces of
predict_sets_one_stage and predict_sets_stage (csrc/call_stage.h) tile their buffers in order without overlap, what goes up
one span in front and what comes down one span behind (for a summary: behind the tables, which stay on the device).  Built
plain for both exp settings, and once as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (the
program writes every byte of every staged piece)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "predict_sets_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
# one-launch / grouped cells over (n 1..129) x (d 1..64) x (K 1..8) x 3 families
COUNTS = (8808, 189336)
# dynamic LDS in bytes of small_reg_kernel<G, NB, 1, false, 0, true, false, true> at (n, d, K) = (5,1,1) (14,2,2) (17,2,1) (40,3,2)
# (50,9,2) (64,4,2) (65,3,3) (104,2,2).  16 x 16 grid, one matrix: 8 (d n + K NP + K d + K + 2 (NP + 16) + 3 NP + 8), e.g. (50,9,2),
# NP = 64: 8 (450 + 128 + 18 + 2 + 160 + 192 + 8) = 7664.  8 x 8 grid, four matrices with a design copy each:
# 8 (d n + 4 (K NP + K d + K + 2 (NP + 8) + 3 NP + 8) + 4 d n), e.g. (50,9,2), NP = 56: 8 (450 + 4 436 + 1800) = 31952
LDS16 = {0: [1144, 1488, 2152, 4032, 7664, 6032, 7096, 8304]}
LDS8 = {0: [2568, 5664, 6832, 14784, 31952, 25664, 27384, 32576]}
LDS16[1], LDS8[1] = [b + 2048 for b in LDS16[0]], [b + 2048 for b in LDS8[0]]
CASES = 7 * 6 * (2 + 2 + 2 * 3) + 6 * 3 * 3 * 2


@pytest.mark.parametrize("table,flags", [(0, []), (1, []), (0, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["poly", "table", "sanitized"])
def test_route_lds_and_staging(table, flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "predict_sets_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[-2] == "cases %d" % CASES
    words = lines[-5].split()
    assert (int(words[1]), int(words[3])) == COUNTS and sum(COUNTS) == 129 * 64 * 8 * 3
    assert [int(w) for w in lines[-4].split()[1:]] == LDS16[table]
    assert [int(w) for w in lines[-3].split()[1:]] == LDS8[table]
    assert max(LDS16[table] + LDS8[table]) <= 160 * 1024 - 64
