"""The host scaffolding the key-holding modules share (uzkge_amd/csrc/handles.hpp) on the CPU: the handle table and the workspace
carver have no HIP in them, so plain g++ builds tests/cpp/handles_host.cpp -- once plain, once under ThreadSanitizer (eight threads
insert and remove through one table), once under Address- and UndefinedBehaviorSanitizer.  The program checks: handles are
tag | 1, tag | 2, ...; tables with different tags refuse each other's handles; a removed handle is gone for good; a drain frees
every live entry once and the count goes on behind it; the carver's offsets are the sums of the preceding sizes, each rounded up
to 256, for arrays of 0, 1, 255, 256 and 257 bytes and for mixed element types, and every typed pointer is base + offset."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "handles_host.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "tsan", "asan_ubsan"])
def test_handle_table_and_carver(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "handles_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr, r.stderr[:4000]
