"""CPU test of the affine set-ups' host index arithmetic (manisdp-matlab_amd/csrc/msdp_affine_plan.h: the SDDMM items and units, the
upper view, the banded tile order, the tiled adjoint, the B route with its packed form, the support list, the per-block tables):
tools/affine_plan_selftest.cpp compares every plan with brute force of its own; here it is compiled with the host compiler and
run.  The program includes nothing but that header, so it needs neither HIP nor a device.

The same program is what a sanitizer run uses, by hand and as a stand-alone program:
    g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imanisdp-matlab_amd/csrc
        tools/affine_plan_selftest.cpp -o $OUT/affine_plan_selftest && $OUT/affine_plan_selftest"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_affine_plans_match_brute_force(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "affine_plan_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "manisdp-matlab_amd", "csrc"),
                    os.path.join(ROOT, "tools", "affine_plan_selftest.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "all checks passed", r.stdout + r.stderr
    assert len(lines) > 40 and all(l.endswith(" ok") for l in lines[:-1])
