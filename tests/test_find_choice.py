"""The decisions of the batch search's launch logic (blurrily_amd/csrc/find_choice.h: the ranges of latency mode, the
class of a batch, the static rule, the pick among measured sweeps, the watch's verdict; find_few's ranges, the shape of
its shared launch, the merge's pool) as plain arithmetic, without a GPU: tests/cpp/find_choice_check.cpp includes that
header alone and holds the expectations, written down from the expressions run_find_on and find_few had inline.
Likewise tests/cpp/find_few_layout_check.cpp over blurrily_amd/csrc/find_few_layout.h: find_few's pinned page and
device lists at the kernels' limits, and the merge of a needle's two lists of rows; and
tests/cpp/cluster_plan_check.cpp over blurrily_amd/csrc/cluster_plan.h: the clustering entries' node numbering, block
plan, new numbers and record order.  Built with g++ and run, plainly
and under the address and undefined-behaviour sanitizers (stand-alone programs: nothing loaded into this interpreter
runs under a sanitizer)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (the sanitizers' runtimes linked statically: the program starts whatever else its environment preloads)
SANITIZED = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _build_and_run(tmp_path, program, sanitize, says):
    exe = str(tmp_path / program)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *sanitize,
           "-I", os.path.join(ROOT, "blurrily_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", program + ".cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == says, r.stdout + r.stderr


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_the_decisions_match_what_was_written_down(tmp_path, sanitize):
    _build_and_run(tmp_path, "find_choice_check", sanitize, "find_choice: 0 expectations failed")


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_find_fews_page_lists_and_row_merge_match_what_was_written_down(tmp_path, sanitize):
    _build_and_run(tmp_path, "find_few_layout_check", sanitize, "find_few_layout: 0 expectations failed")


@pytest.mark.parametrize("sanitize", [[], SANITIZED], ids=["plain", "sanitized"])
def test_the_cluster_entries_numbering_plan_new_numbers_and_record_order_match_what_was_written_down(tmp_path, sanitize):
    _build_and_run(tmp_path, "cluster_plan_check", sanitize, "cluster_plan: 0 expectations failed")
