"""The design search's route and carve on the CPU: tests/host_small/design_fit_layout_check.cpp walks small_route_design_fit
over n 1..129, every d, K, kernel family and n_fixed from -1 to n (Reg exactly where the family is Gaussian, the design gradient
has its register-resident instance, the start has 1 .. 64 variables and its words fit behind the per-design carve: the condition
and the carve are summed by hand in the program) and pins the dynamic LDS total of the eight new instances.  Built plain for
both exp settings, and once as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "design_fit_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
# Reg / Unsupported cells over (n 1..129) x (d 1..64) x (K 1..8) x 3 families x (n_fixed -1..n), and the cells refused for the
# start's words alone (the evaluator serves the shape and the stepper takes its nv); exp table off / on
COUNTS = {0: (237868, 13037780, 4169), 1: (235930, 13039718, 4607)}
# dynamic LDS in bytes of small_reg_kernel<16, NB, NB + 1, false, 3, ..., DFIT> at (n, d, n_fixed), K = 2: (14,2,0) NB 1,
# (21,2,14) and (17,9,10) NB 2, (33,3,16) NB 3, (50,9,43) NB 4, (65,1,1) NB 5, (81,2,60) NB 6, (97,5,90) NB 7, (128,4,112) NB 8:
#   8 (2 d n + K NP + K d + K + 2 (NP + 16 (NB + 1)) + 3 NP + 8 + 1 + NP (NP + 2) + 112 + 2 + nv + 16 + 16 nv), NP = 16 NB,
# e.g. NB = 8 at (128,4,112), nv = 64: 8 (1024 + 256 + 8 + 2 + 544 + 384 + 9 + 16640 + 112 + 66 + 1040) = 8 x 20085 = 160680
LDS = {0: [9128, 15000, 23552, 32608, 55696, 69384, 91896, 124192, 160680]}
LDS[1] = [b + 2048 for b in LDS[0]]


@pytest.mark.parametrize("table,flags", [(0, []), (1, []), (0, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["poly", "table", "sanitized"])
def test_route_and_lds(table, flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "design_fit_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    words = lines[-3].split()
    assert (int(words[1]), int(words[3]), int(words[5])) == COUNTS[table]
    assert int(words[1]) + int(words[3]) == sum(n + 2 for n in range(1, 130)) * 64 * 8 * 3
    assert [int(w) for w in lines[-2].split()[1:]] == LDS[table]
    assert max(LDS[table]) <= 160 * 1024 - 64
