"""The buffer layouts of the C entry points (csrc/stage_layout.h -- the header csrc/capi.hip sizes and carves its staging
buffers, workspace tails and factor sets with) executed on the CPU: tests/host_stage/stage_layout_check.cpp declares a few
piece lists once and runs each declaration as the library does, first without a base to get the size and then over a base
to get the pointers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_stage", "stage_layout_check.cpp")


def test_planning_and_carving_agree(tmp_path):
    """Zero-length pieces, int pieces of odd count and sizes above 4 GiB among them: both passes end at the same offset,
    every pointer is 256-byte aligned, pieces do not overlap and lie inside [base, base + off)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "stage_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert r.stdout.strip() == "ok"
