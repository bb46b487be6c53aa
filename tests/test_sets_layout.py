"""The sets form's route and staging on the CPU: tests/host_small/sets_layout_check.cpp walks small_route_sets over n 1..129,
every d, K and kernel family (Reg exactly where the family is Gaussian and the sets instance's carves, summed by hand in the
program, fit), holds the grid chooser to an instance that exists and fits, and checks that the pieces of sets_stage
(csrc/call_stage.h) tile their buffer in order without overlap.  Built plain for both exp settings, and once as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer (the program writes every byte of every staged piece)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "sets_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
# Reg / Blocked cells over (n 1..129) x (d 1..64) x (K 1..8) x 3 families; exp table off / on
COUNTS = {0: (64891, 133253), 1: (64815, 133329)}


@pytest.mark.parametrize("table,flags", [(0, []), (1, []), (0, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["poly", "table", "sanitized"])
def test_route_grid_and_staging(table, flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sets_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCCGP_SMALL_EXP_TABLE=%d" % table, *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    words = lines[-2].split()
    assert (int(words[1]), int(words[3])) == COUNTS[table]
    assert int(words[1]) + int(words[3]) == 129 * 64 * 8 * 3
    assert int(words[5]) > 0 and int(words[7]) > 0      # both grids are chosen somewhere
