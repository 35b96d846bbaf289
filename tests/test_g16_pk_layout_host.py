"""The walk over a compressed Groth16 proving key (uzkge_amd/csrc/g16_pk_layout.hpp, what uzk_g16_pk_layout and the two key-level
decoders start from) on the CPU: the header has no HIP in it, so plain g++ builds tests/cpp/g16_pk_layout_host.cpp as a stand-alone
program -- once plain, once under Address- and UndefinedBehaviorSanitizer.  The program checks the real key's offsets, counts and
infinities; the key cut at every section boundary and one byte before and after each (from a heap block of exactly that length);
a byte behind the key; length words of 2^63, 2^64 - 1 and one too many; the empty input."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "g16_pk_layout_host.cpp")
PARTS = [os.path.join(ROOT, "tests", "golden", "groth16-reveal-%s.bin" % k) for k in ("head", "b-queries", "tail")]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_key_walk(tmp_path, flags):
    exe = os.path.join(str(tmp_path), "g16_pk_layout_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe, *PARTS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr, r.stderr[:4000]
