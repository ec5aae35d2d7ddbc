"""CPU test of the plan of the block kinds' persistent tCG (manisdp-matlab_amd/csrc/msdp_blockpersist_plan.h: lanes per block,
grid, row slots, LDS bytes, which handles are eligible): tools/block_persist_plan_selftest.cpp compares every plan with brute
force of its own over nb = 1 .. 20000 (sampled), B in {2, 3, 4}, p = 1 .. 64, 64 / 256 / 304 compute units and grid caps 0, 8,
16; here it is compiled with the host compiler and run.  The program includes nothing but that header, so it needs neither HIP
nor a device.

The same program is what a sanitizer run uses, by hand and as a stand-alone program:
    g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imanisdp-matlab_amd/csrc
        tools/block_persist_plan_selftest.cpp -o $OUT/block_persist_plan_selftest && $OUT/block_persist_plan_selftest"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_persist_plans_match_brute_force(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "block_persist_plan_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "manisdp-matlab_amd", "csrc"),
                    os.path.join(ROOT, "tools", "block_persist_plan_selftest.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "all checks passed", r.stdout + r.stderr
    assert len(lines) == 4 * 3 * 3 * 8 + 1 and all(l.endswith(" ok") for l in lines[:-1])
