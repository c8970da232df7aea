"""The index arithmetic of the time series' shared ring (csrc/ring.h: ring_held, ring_range_ok, ring_pieces) against a brute-force
model.  tests/ring_check.cpp - a stand-alone program that includes the HIP-free part of the header - is built with plain g++ under
the address and undefined-behaviour sanitizers and run as a child process.  For capacity 1, 2, 3, 5, recorded 0 .. 3 * capacity + 1
and every (first, count) up to one row past what is held it checks: held and dropped, acceptance or refusal of the range, that the
pieces name exactly the model's rows in order, that there are at most two, and that none crosses the end of the ring.  No device
needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_arithmetic_matches_a_deque_model(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "ring_check")
    build = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "ring_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 1000, run.stdout
    assert run.stderr == ""
