"""The decisions of the batch search's launch logic (blurrily_amd/csrc/find_choice.h: the ranges of latency mode, the
class of a batch, the static rule, the pick among measured sweeps, the watch's verdict) as plain arithmetic, without a
GPU: tests/cpp/find_choice_check.cpp includes that header alone and holds the expectations, written down from the
expressions run_find_on had inline.  Built with g++ and run, plainly and under the address and undefined-behaviour
sanitizers (a stand-alone program: nothing loaded into this interpreter runs under a sanitizer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (the sanitizers' runtimes linked statically: the program starts whatever else its environment preloads)
SANITIZED = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_the_decisions_match_what_was_written_down(tmp_path, sanitize):
    exe = str(tmp_path / "find_choice_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *sanitize,
           "-I", os.path.join(ROOT, "blurrily_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "find_choice_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "find_choice: 0 expectations failed", r.stdout + r.stderr
