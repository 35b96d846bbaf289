"""tests/match_cs_ref.py, the restatement of zmatchmaking's circuit, held to the reference's own verifier key, and the library's
layout builder (uzkge_amd/csrc/matchcs_layout.cpp) held to the restatement.

tests/golden/matchmaking_vk_golden.json carries what the reference generated for 50 players: 18 commitments (8 selectors -- the file
predates q_ecc, today's slot 7, which is all zero in this circuit -- 5 permutation vectors, qb, 4 q_prk), k, the public-input rows.  A
commitment of an evaluation vector over the reference's Lagrange SRS is a function of every entry of the vector, and the s vectors are
a function of every wire of every row -- so a layout that reproduces all 18 bit for bit is the reference's layout, with no Rust run.

The builder has no HIP in it, so g++ compiles tests/cpp/matchcs_host.cpp (which includes it) plain and under Address- and
UndefinedBehaviorSanitizer; the program runs as a child process, nothing is loaded into Python.  Its dump is compared word for word
with the restatement, and every variable's DEFINITION (what the witness kernel computes) is evaluated on Python integers and compared
with the value the restated build_cs gives that variable."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import anemoi_ref as an
import bn254_py as opy
import match_cs_ref as mr
import oracle_c as oc
from util import GOLDEN, affine_of, load_srs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "matchcs_host.cpp")
R = mr.R
SIZES = [3, 4, 5, 7, 8, 50]          # one output chunk with 2 and 3 outputs; two chunks, ragged and full; three chunks; the real size
DUMPED = SIZES + [63, 64]            # the most players in 8192 rows; UZK_MATCH_CS_MAX_PLAYERS, the only size of 16384 rows


def golden_vk():
    return json.load(open(os.path.join(GOLDEN, "matchmaking_vk_golden.json")))


def golden_key(vk):
    """the fixture's 18 commitments in today's order of 19: q_ecc, slot 7, is the identity"""
    return vk["cm_q"][:7] + [None] + vk["cm_q"][7:] + vk["cm_s"] + [vk["cm_qb"]] + vk["cm_prk"]


def match(players, seed, zero=False):
    if zero:
        return [0] * players, 0, 0
    rng = random.Random("match-%d-%s" % (players, seed))
    return [rng.randrange(R) for _ in range(players)], rng.randrange(R), rng.randrange(R)


_BUILT = {}


def built(players, seed=0, zero=False):
    key = (players, seed, zero)
    if key not in _BUILT:
        _BUILT[key] = mr.build_cs(*match(players, seed, zero))
    return _BUILT[key]


def test_the_restated_tables_commit_to_the_golden_verifier_key():
    vk = golden_vk()
    cs = built(50, zero=True)
    assert (cs.num_vars, cs.size, cs.gates) == (vk["num_vars"], vk["cs_size"], 5208) and vk["cs_size"] == 8192
    assert cs.public_vars_constraint_indices == vk["pi_rows"] == list(range(5106, 5208))
    assert (vk["anemoi_generator"], vk["anemoi_generator_inv"]) == (an.G, an.DELTA)
    root = opy.root_of_unity(cs.size)
    group = mr.domain(cs.size, root)
    n_inv = pow(cs.size, -1, R)
    assert vk["pi_lagrange_constants"] == [group[r] * n_inv % R for r in vk["pi_rows"]]
    vecs, want = mr.key_vectors(cs, vk["k"], root), golden_key(vk)
    assert len(vecs) == len(want) == 19 == sum(c for _, c in mr.KEY_ORDER)
    wire, _ = load_srs("lagrange-srs-%d.bin" % cs.size)
    for i, (vec, w) in enumerate(zip(vecs, want)):
        got = affine_of(oc.msm_pippenger(wire, oc.fr_from_ints(vec), 0, 4)) if any(vec) else None
        assert (None if got is None else list(got)) == w, "commitment %d" % i
    assert not any(vecs[7]) and all(w is not None for j, w in enumerate(want) if j != 7)


def test_the_size_formula_is_the_built_layout_for_every_player_count():
    for players in range(mr.MIN_PLAYERS, mr.MAX_PLAYERS + 1):
        cs = built(players, zero=True)
        assert (cs.gates, cs.num_vars) == (mr.gate_count(players), mr.var_count(players)), players
        assert len(cs.anemoi_constraints_indices) == 1 + mr.stream_permutations(players) == 1 + an.permutations(2, players - 1)
        assert cs.size == 1 << (cs.gates - 1).bit_length() and len(cs.public_vars_constraint_indices) == 2 * players + 2


@pytest.mark.parametrize("zero", [False, True], ids=["random", "all_zero"])
@pytest.mark.parametrize("players", SIZES)
def test_the_restated_witness_satisfies_the_restated_circuit(players, zero):
    inputs, seed, rnd = match(players, 1, zero)
    cs, lay = built(players, 1, zero), built(players, zero=True)
    assert cs.wiring == lay.wiring and cs.selectors == lay.selectors and cs.defs == lay.defs         # the layout is a function of N
    assert cs.public_vars_constraint_indices == lay.public_vars_constraint_indices
    assert cs.boolean_constraint_indices == lay.boolean_constraint_indices and cs.anemoi_constraints_indices == lay.anemoi_constraints_indices
    pi = mr.public_inputs(cs)
    assert pi[:players] == inputs and pi[-2:] == [rnd, an.eval_variable_length_hash([seed])]
    assert sorted(pi[players:2 * players]) == sorted(inputs)
    assert mr.verify_witness(cs, cs.witness, pi) is None
    assert mr.check_copies(cs, mr.extend_witness(cs)) is None
    assert mr.evaluate_defs(cs.defs, inputs, seed, rnd) == cs.witness


def test_distinct_inputs_come_out_as_a_permutation():
    inputs = list(range(100, 150))
    cs = mr.build_cs(inputs, 7, 9)
    out = [cs.witness[v] for v in cs.output_vars]
    assert sorted(out) == inputs and out != inputs
    # the Fisher-Yates steps of matchmaking.rs:83-226 on plain integers
    stream, want = an.eval_stream_cipher([7, 9], 49), list(inputs)
    for i in range(1, 50):
        r = stream[i - 1] % (i + 1)
        want[i], want[r] = want[r], want[i]
    assert out == want


@pytest.mark.parametrize("players", [5, 8])
def test_one_changed_value_of_each_kind_fails_the_check(players):
    cs = built(players, 1)
    pi = mr.public_inputs(cs)
    seen = set()
    for v, d in enumerate(cs.defs):
        if d[0] in seen:
            continue
        seen.add(d[0])
        bad = list(cs.witness)
        bad[v] = (bad[v] + 1) % R
        assert mr.verify_witness(cs, bad, pi) is not None, "variable %d (%s)" % (v, mr.KIND_NAMES[d[0]])
    assert seen == set(range(len(mr.KIND_NAMES)))
    ext = mr.extend_witness(cs)
    ext[2][cs.gates - 3] = (ext[2][cs.gates - 3] + 1) % R                # one cell of the extended witness: a copy constraint
    assert "copy constraint" in mr.check_copies(cs, ext)
    assert mr.verify_witness(cs, cs.witness, pi[:-1] + [(pi[-1] + 1) % R]) is not None


def test_the_generated_round_key_table_is_the_restatement():
    """uzkge_amd/csrc/matchcs_consts.inc: the 56 round keys after the linear layer as Montgomery words"""
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_matchcs_consts.py"), "--check"]).returncode == 0
    text = open(os.path.join(ROOT, "uzkge_amd", "csrc", "matchcs_consts.inc")).read()
    rows = re.findall(r"\{((?:0x[0-9a-f]{8}u(?:, )?){8})\}", text)
    vals = [sum(int(w, 16) << (32 * i) for i, w in enumerate(re.findall(r"0x([0-9a-f]{8})u", row))) for row in rows]
    assert vals == [(v << 256) % R for r in range(14) for v in mr.PRK[r]]


# ---- the C++ layout ------------------------------------------------------------------------------------------------------------------
def parse(path):
    a = np.fromfile(path, dtype="<u4").astype(np.int64)
    players, size, n, num_vars, pi_count, blocks = (int(v) for v in a[:6])
    at, out = 6, {"players": players, "size": size, "n": n, "num_vars": num_vars}
    for name, count in (("wiring", 5 * n), ("perm", 5 * n), ("sel", 9 * n), ("qb", n), ("prk_row", n), ("defs", num_vars), ("pi_rows", pi_count),
                        ("pi_vars", pi_count), ("block_rows", blocks)):
        out[name] = a[at:at + count].tolist()
        at += count
    assert at == len(a)
    return out


def run_host(tmp, flags, sizes):
    exe = os.path.join(tmp, "matchcs_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe, tmp] + [str(s) for s in sizes], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[:4000]
    return {s: parse(os.path.join(tmp, "%d.bin" % s)) for s in sizes}


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return run_host(str(tmp_path_factory.mktemp("matchcs")), [], DUMPED)


def same_layout(got, cs):
    n = cs.size
    assert (got["players"], got["size"], got["n"], got["num_vars"]) == (cs.players, cs.gates, n, cs.num_vars)
    assert got["wiring"] == [v for w in cs.wiring for v in w]
    assert got["perm"] == mr.compute_permutation(cs)
    assert [v - 32768 for v in got["sel"]] == [v for s in cs.selectors for v in s]
    assert [i for i, v in enumerate(got["qb"]) if v] == cs.boolean_constraint_indices
    assert got["prk_row"] == mr.prk_rows(cs) and got["block_rows"] == cs.anemoi_constraints_indices
    assert got["pi_rows"] == cs.public_vars_constraint_indices and got["pi_vars"] == cs.public_vars_witness_indices
    assert [(d >> 28, (d >> 16) & 0xFFF, (d >> 8) & 0xFF, d & 0xFF) for d in got["defs"]] == cs.defs


@pytest.mark.parametrize("players", DUMPED)
def test_the_layout_is_the_restated_one(dumps, players):
    same_layout(dumps[players], built(players, zero=True))


@pytest.mark.parametrize("players", DUMPED)
def test_every_variable_definition_gives_the_restated_value(dumps, players):
    for zero in (False, True):
        defs = [(d >> 28, (d >> 16) & 0xFFF, (d >> 8) & 0xFF, d & 0xFF) for d in dumps[players]["defs"]]
        assert mr.evaluate_defs(defs, *match(players, 1, zero)) == built(players, 1, zero).witness


def test_the_layout_builder_is_clean_under_asan_and_ubsan(tmp_path):
    got = run_host(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [3, 50])
    for players in (3, 50):
        same_layout(got[players], built(players, zero=True))
