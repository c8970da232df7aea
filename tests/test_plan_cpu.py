"""The launch decisions of csrc/launch_plan.h (collide variant, XCD grid, z-solve plan, column blocks and their counts) against the
predicates they replaced.  tests/plan_check.cpp - a stand-alone program that includes the header, which has no HIP in it - is built
with plain g++ under the address and undefined-behaviour sanitizers and run as a child process.  Its model is the launchers' former
`if` chains and block arithmetic, transcribed literally; the sweep is rows 0 .. 600, ny and nxh 1 .. 40 and the large plane sizes,
tri_partition 0 .. 2, with and without the LDS grant, single context and slab, block counts 1 .. 16, and n_lattices 1, 3, 4 with
both flags.  For every point family, R, LANES, modes per workgroup, LDS bytes and the kernel's name are equal, for every block
(x0, bw); where nxh is a multiple of 8 the blocks tile [0, nxh) in whole lines and whole workgroups.  No device needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_matches_the_former_predicates(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "plan_check")
    build = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 12_000_000, run.stdout
    assert run.stderr == ""
