"""The library's layout builder of the reveal circuit (uzkge_amd/csrc/revealcs_layout.cpp) held to the restatement
(tests/reveal_cs_ref.py).  The builder has no HIP in it, so g++ compiles tests/cpp/revealcs_host.cpp (which includes it) plain and under
Address- and UndefinedBehaviorSanitizer; the program runs as a child process, nothing is loaded into Python.  Its dump -- the three CSR
matrices, the variable map and the 256 constant multiples -- is compared entry for entry with the restatement."""
import os
import subprocess

import numpy as np
import pytest

import reveal_cs_ref as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "revealcs_host.cpp")
Q = rc.Q
R_INV = pow(1 << 256, -1, Q)


def elems(words):
    """[k, 8] uint32 Montgomery words -> integers"""
    w = np.asarray(words, dtype=np.int64).reshape(-1, 8)
    return [sum(int(x) << (32 * i) for i, x in enumerate(row)) * R_INV % Q for row in w]


def parse(path):
    a = np.fromfile(path, dtype="<u4").astype(np.int64)
    n_vars, n_inputs, nc, domain = (int(v) for v in a[:4])
    at, out = 4, {"n_vars": n_vars, "n_inputs": n_inputs, "n_constraints": nc, "domain": domain, "mats": []}
    for _ in range(3):
        nnz = int(a[at]); at += 1
        ptr = a[at:at + nc + 1].tolist(); at += nc + 1
        col = a[at:at + nnz].tolist(); at += nnz
        val = elems(a[at:at + 8 * nnz]); at += 8 * nnz
        assert ptr[0] == 0 and ptr[-1] == nnz
        out["mats"].append([[(col[k], val[k]) for k in range(ptr[i], ptr[i + 1])] for i in range(nc)])
    out["roles"] = a[at:at + n_vars].tolist(); at += n_vars
    out["multiples"] = elems(a[at:at + 512 * 8]); at += 512 * 8
    assert at == len(a)
    return out


def run_host(tmp, flags):
    exe = os.path.join(tmp, "revealcs_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[:4000]
    return parse(os.path.join(tmp, "reveal.bin"))


def same_layout(got):
    assert (got["n_vars"], got["n_inputs"], got["n_constraints"], got["domain"]) == (rc.N_VARS, rc.N_INPUTS, rc.N_CONSTRAINTS, rc.DOMAIN)
    for tag, mine, ref in zip("ABC", got["mats"], rc.matrices()):
        assert mine == ref, tag
    roles = rc.roles()
    want = [0xFFFFFFFF] * rc.N_INPUTS + [(roles[i][0] << 24) | (roles[i][1] << 8) | roles[i][2] for i in range(rc.N_INPUTS, rc.N_VARS)]
    assert got["roles"] == want
    assert got["multiples"] == [c for p in rc.fixed_multiples() for c in p]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return run_host(str(tmp_path_factory.mktemp("revealcs")), [])


def test_the_layout_is_the_restated_one(dump):
    same_layout(dump)


def test_the_layout_builder_is_clean_under_asan_and_ubsan(tmp_path):
    same_layout(run_host(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
