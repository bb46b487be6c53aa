"""The staging of ccgp_cgp_predict_sets on the CPU: tests/host_small/cgp_predict_sets_layout_check.cpp checks that the pieces
of cgp_predict_sets_stage (csrc/call_stage.h) tile a chunk's buffer in order without overlap -- the sets and their test sites
in front and pushed with the first chunk only, the results one span down, the kept blocks behind them -- and that a row's
share is what the chunk planner is told.  Built plain, and once as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (the program writes every byte of every staged piece)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "cgp_predict_sets_layout_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_staging(flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cgp_predict_sets_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[-2] == "cases 63"
