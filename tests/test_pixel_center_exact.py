"""The fused flow pass takes its pixel centres (i + 0.5) / n from a host reciprocal with one correction step and walks (row, item in the
row) with integer adds (pixel_center_recip, item_walk: flowmap_amd/csrc/fm_math.h).  Both must equal the division they replace, exactly:
tests/host_checks/pixel_center_exact.cpp checks every length 1..16 384 with every index, and the walk for every row length 1..1 024 (and
1 025, 2 048, 4 097) along the first three workgroups' threads.  The program stands alone — nothing is loaded into this process — and is
built twice: as the kernels' host twin is (-O2 -ffp-contract=off), and under the address and undefined-behaviour sanitizers."""

import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "host_checks" / "pixel_center_exact.cpp"
QUOTIENTS = 16384 * 16385 // 2          # every (i, n), i < n <= 16 384
WALK_STEPS = (1024 + 3) * 3 * 256 * 8   # row lengths x starting items of three workgroups x iterations


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_reciprocal_centres_and_item_walk_equal_the_divisions(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "a host C++ compiler is required"
    exe = tmp_path / "pixel_center_exact"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", *flags, str(SOURCE), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    centres = re.search(r"pixel centres: (\d+) quotients, (\d+) mismatches", run.stdout)
    walk = re.search(r"item walk: (\d+) steps, (\d+) mismatches", run.stdout)
    assert centres and (int(centres.group(1)), int(centres.group(2))) == (QUOTIENTS, 0)
    assert walk and (int(walk.group(1)), int(walk.group(2))) == (WALK_STEPS, 0)
