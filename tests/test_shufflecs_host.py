"""The library's layout builder for zshuffle's circuit (uzkge_amd/csrc/shufflecs_layout.cpp) on the CPU, against the restatement.

The builder has no HIP in it, so g++ compiles tests/cpp/shufflecs_host.cpp (which includes it) plain and under Address- and
UndefinedBehaviorSanitizer.  The program checks the layout's own invariants and dumps it; here the dump is compared word for word with
tests/shuffle_cs_ref.py -- wiring, permutation, selectors, boolean rows, remark blocks, public-input rows -- and every variable's
DEFINITION (what the witness kernel will compute) is evaluated in Python integers and compared with the value the restated build_cs
gives that variable for a real game."""
import os
import subprocess

import numpy as np
import pytest

import shuffle_cs_ref as cr
import shuffle_ref as sr
from test_shuffle_cs_ref_host import game, pk_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shufflecs_host.cpp")
SIZES = [1, 2, 3, 4, 5, 6, 7, 20, 52, 63, 64]      # 63: the most cards with a ragged last product; 64: UZK_SHUFFLE_CS_MAX_CARDS
R = cr.R


def parse(path):
    a = np.fromfile(path, dtype="<u4").astype(np.int64)
    cards, size, n, num_vars, pi_count = (int(v) for v in a[:5])
    at, out = 5, {"cards": cards, "size": size, "n": n, "num_vars": num_vars}
    for name, count in (("wiring", 5 * n), ("perm", 5 * n), ("sel", 9 * n), ("qb", n), ("block", n), ("defs", num_vars), ("pi_rows", pi_count),
                        ("pi_vars", pi_count)):
        out[name] = a[at:at + count].tolist()
        at += count
    assert at == len(a)
    return out


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def dumps(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("shufflecs"))
    exe = os.path.join(d, "shufflecs_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *request.param, "-o", exe, SRC], check=True)
    r = subprocess.run([exe, d] + [str(s) for s in SIZES], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr, r.stderr[:4000]
    return {s: parse(os.path.join(d, "%d.bin" % s)) for s in SIZES}


@pytest.mark.parametrize("cards", SIZES)
def test_the_layout_is_the_restated_one(dumps, cards):
    got, cs = dumps[cards], cr.layout(cards)
    n = cs.size
    assert (got["cards"], got["size"], got["n"], got["num_vars"]) == (cards, cs.gates, n, cs.num_vars)
    assert got["wiring"] == [v for w in cs.wiring for v in w]
    assert got["perm"] == cr.compute_permutation(cs)
    assert [(v - 1) % R for v in got["sel"]] == [v for s in cs.selectors for v in s]
    assert [i for i, v in enumerate(got["qb"]) if v] == cs.boolean_constraint_indices
    block = [0] * n
    for k, row in enumerate(cr.remark_rows(cs)):
        for j in range(cr.ITER):
            block[row + j] = 1 + cr.ITER * k + j
    assert got["block"] == block
    assert got["pi_rows"] == cs.public_vars_constraint_indices and got["pi_vars"] == cs.public_vars_witness_indices


def eval_defs(defs, deck, traces, perm):
    """The value of every variable from its definition (uzkge_amd/csrc/shufflecs.hpp)."""
    n = len(deck)
    m = lambda i, j: 1 if perm[i] == j else 0
    rem = lambda k, c: traces[k][cr.ITER - 1][c]

    def product(i, c, t):
        v = m(i, 2 * t) * rem(2 * t, c)
        return v + m(i, 2 * t + 1) * rem(2 * t + 1, c) if 2 * t + 1 < n else v
    out = []
    for d in defs:
        kind, a, b, c = d >> 28, (d >> 16) & 0xFFF, (d >> 8) & 0xFF, d & 0xFF
        if kind == 0:
            v = a
        elif kind == 1:
            v = deck[a][b // 2][b % 2]
        elif kind == 2:
            v = traces[a][b][c]
        elif kind == 3:
            v = m(a, b)
        elif kind == 4:
            v = sum(m(a, j) for j in range(c))
        elif kind == 5:
            v = sum(m(i, a) for i in range(c))
        elif kind == 6:
            v = product(a, b, c)
        else:
            assert kind == 7
            v = sum(product(a, b, t) for t in range(c))
        out.append(v % R)
    return out


@pytest.mark.parametrize("cards", [1, 2, 3, 4, 5, 6, 7, 20, 63, 64])
def test_every_variable_definition_gives_the_restated_value(dumps, cards):
    pk, deck, digits, perm = game(cards, 300 + cards)
    t_pk = pk_tables(pk)
    cs = cr.build_cs(deck, digits, perm, t_pk)
    traces = [sr.eval_remark_with_trace(c, d, t_pk) for c, d in zip(deck, digits)]
    assert eval_defs(dumps[cards]["defs"], deck, traces, perm) == cs.witness
