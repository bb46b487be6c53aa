"""The buffer layouts of the C entry points (csrc/stage_layout.h -- the header csrc/capi.hip sizes and carves its staging
buffers, workspace tails and factor sets with -- and csrc/call_stage.h, the layouts ccgp_reserve or several entry points
share) executed on the CPU: tests/host_stage/stage_layout_check.cpp runs a few piece lists and the library's own
declarations as the library does, first without a base to get the size and then over a base to get the pointers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_stage", "stage_layout_check.cpp")


def test_planning_and_carving_agree(tmp_path):
    """Zero-length pieces, int pieces of odd count and sizes above 4 GiB among them: both passes end at the same offset,
    every pointer is 256-byte aligned, pieces do not overlap and lie inside [base, base + off).  The shared layouts at three
    shapes, with and without each optional piece: the same, what a call pushes and what it pulls are each one run of
    aligned pieces back to back, ccgp_reserve's staging holds every layout it reserves for, and the offsets of the
    gradient layouts at (5, 2, 2, B = 3) are the ones written down by hand."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "stage_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert r.stdout.strip() == "ok"
