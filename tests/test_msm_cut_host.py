"""The MSM's bucket-cutting rule (uzkge_amd/csrc/msm_cut.hpp) on the CPU.  The rule is a __host__ __device__ function in a header
without HIP in it, so plain g++ builds tests/cpp/msm_cut_host.cpp -- once plain, once under Address- and
UndefinedBehaviorSanitizer.  The program checks, for plans with the taper off, automatic and forced and for random and extreme
bucket populations: the pieces of every bucket add up to its population; no piece is longer than the bucket's cut length or than
L <= 256, and its bin of the schedule's length histogram is inside kLenBins; a short-cut bucket has no more tasks than the last
fold level is told; all tasks together stay within the bound the host reserves for; with the taper off every bucket has
ceil(p / L) tasks and the bound is the one of before."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "msm_cut_host.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_cut_rule_and_task_bound(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "msm_cut_host")
    subprocess.run(["g++", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr, r.stderr[:4000]
