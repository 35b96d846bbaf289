"""tests/reveal_cs_ref.py, the restatement of the reveal circuit's R1CS, held to the reference's own Groth16 proving key
(tests/golden/groth16-reveal-{head,b-queries,tail}.bin): the counts, the key's fingerprints (a query point is infinity exactly where a
variable is absent from a matrix; equal and opposite B columns are equal and opposite points of b_g2_query), satisfaction at the edge
scalars and points, and THE GATE: a proof made with these matrices and the real key is accepted under the key's own verifying key.
A key is a function of every coefficient of every row, so a layout whose proofs verify under it is the reference's layout."""
import os
import random
import re
import subprocess
import sys

import pytest

import ed_ref as ed
import g16_ref as gr
import reveal_cs_ref as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = rc.Q


@pytest.fixture(scope="module")
def key():
    return gr.load_real_key()


@pytest.fixture(scope="module")
def cols():
    return [rc.columns(M) for M in rc.matrices()]


def edge_cases():
    """(name, sk, e1): random, the edge scalars, e1 = G, e1 = a point of order 8 plus a subgroup point"""
    rng = random.Random("reveal-cs-edges")
    p = ed.mul(rng.randrange(1, ed.L), ed.G)
    mixed = ed.add(ed.order8_point(), ed.mul(rng.randrange(1, ed.L), ed.G))
    assert ed.on_curve(mixed) and ed.classify(mixed) == ed.NOT_IN_SUBGROUP
    low128 = (rng.randrange(ed.L) >> 128 << 128) | ((1 << 128) - 1)
    return [("random", rng.randrange(ed.L), p), ("sk=0", 0, p), ("sk=1", 1, p), ("sk=l-1", ed.L - 1, p), ("low128", low128 % (1 << 256), p),
            ("e1=G", rng.randrange(ed.L), ed.G), ("order8", rng.randrange(ed.L), mixed), ("order8,sk=0", 0, mixed)]


def test_counts():
    A, B, C = rc.matrices()
    assert len(A) == len(B) == len(C) == rc.N_CONSTRAINTS == 4869
    z = rc.witness(5, ed.G)
    assert len(z) == rc.N_VARS == 4869 and rc.N_INPUTS == 7 and gr.domain_of(rc.N_CONSTRAINTS, rc.N_INPUTS) == rc.DOMAIN == 8192
    assert gr.SECTION_LENS == (rc.N_INPUTS, rc.N_VARS, rc.N_VARS, rc.N_VARS, rc.DOMAIN - 1, rc.N_VARS - rc.N_INPUTS)
    roles = rc.roles()
    assert sorted(roles) == list(range(7, rc.N_VARS))
    assert 6 + 256 + 1275 + 3325 == rc.N_VARS - rc.N_INPUTS
    assert [sum(1 for c, _, _ in roles.values() if c == ch) for ch in range(4)] == [6, 256, 1275, 3325]
    assert (rc.OFF_POINTS, rc.OFF_BITS, rc.OFF_FIXED, rc.OFF_VAR) == tuple(min(i for i, r in roles.items() if r[0] == ch) for ch in range(4))
    assert all(all(v % Q for _, v in row) and [c for c, _ in row] == sorted({c for c, _ in row}) for M in (A, B, C) for row in M)


def test_fingerprint_infinities(key, cols):
    ca, cb, cc = cols
    for i in range(rc.N_VARS):
        assert (i not in ca) == (key.a_query[i] is None), i
        assert (i not in cb) == (key.b_g1_query[i] is None) == (key.b_g2_query[i] is None), i
    for i in range(rc.N_INPUTS, rc.N_VARS):
        if i in ca or i in cb or i in cc:
            assert key.l_query[i - rc.N_INPUTS] is not None, i
    assert sum(p is None for p in key.b_g2_query) == 775 == rc.N_VARS - len(cb)


def test_fingerprint_equal_and_opposite_b_columns(key, cols):
    """README: 775 infinities, 256 duplicates and 254 opposite pairs in b_g2_query -- all of them are equal and opposite B columns"""
    cb = cols[1]
    neg2 = lambda p: (p[0], tuple((-c) % gr.P for c in p[1]))
    by_col, by_point = {}, {}
    for i, col in cb.items():
        by_col.setdefault(tuple(sorted(col.items())), []).append(i)
        by_point.setdefault(key.b_g2_query[i], []).append(i)
    dup_cols = sorted(tuple(v) for v in by_col.values() if len(v) > 1)
    dup_points = sorted(tuple(v) for v in by_point.values() if len(v) > 1)
    assert dup_cols == dup_points and len(dup_cols) == 256 and all(len(v) == 2 for v in dup_cols)
    opp_cols = set()
    for k, v in by_col.items():
        other = by_col.get(tuple((r, (-x) % Q) for r, x in k))
        if other:
            opp_cols.add(frozenset((v[0], other[0])))
    opp_points = set()
    for p, v in by_point.items():
        other = by_point.get(neg2(p))
        if other:
            opp_points.add(frozenset((v[0], other[0])))
    assert opp_cols == opp_points and len(opp_cols) == 254
    for pair in opp_cols:
        i, j = sorted(pair)
        assert key.b_g1_query[i] == (key.b_g1_query[j][0], gr.P - key.b_g1_query[j][1])


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: c[0])
def test_the_witness_satisfies_every_constraint(case):
    _, sk, e1 = case
    z = rc.witness(sk, e1)
    assert z == rc.synthesize(sk, e1).z                             # the walk without the combinations gives the same values
    assert len(z) == rc.N_VARS and z[0] == 1 and rc.satisfied(rc.matrices(), z) == []
    assert tuple(z[1:7]) == e1 + ed.mul(sk, e1) + ed.mul(sk, ed.G) == rc.statement(sk, e1)
    assert z[rc.OFF_BITS:rc.OFF_BITS + 256] == [(sk >> i) & 1 for i in range(256)]
    bad = list(z)
    bad[rc.OFF_VAR + 1] = (bad[rc.OFF_VAR + 1] + 1) % Q
    assert rc.satisfied(rc.matrices(), bad) != []


def test_the_gate_a_proof_verifies_under_the_reference_key(key):
    """g16_ref.prove over the real key and the restated matrices, one fresh (sk, e1): accepted by g16_ref.verify under the key's own
    verifying key; rejected once a coordinate of the statement changes"""
    rng = random.Random(os.urandom(16))
    sk, e1 = rng.randrange(1, ed.L), ed.mul(rng.randrange(1, ed.L), ed.G)
    z = rc.witness(sk, e1)
    proof = gr.prove(key, rc.matrices(), rc.N_INPUTS, z, rng.randrange(gr.R), rng.randrange(gr.R))
    assert gr.verify(key, z[:rc.N_INPUTS], proof)
    for k in (1, 4):
        other = list(z[:rc.N_INPUTS])
        other[k] = (other[k] + 1) % Q
        assert not gr.verify(key, other, proof)


def test_the_generated_multiples_are_the_restatement():
    """uzkge_amd/csrc/revealcs_consts.inc: 2^i G as Montgomery words, then d"""
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_revealcs_consts.py"), "--check"]).returncode == 0
    text = open(os.path.join(ROOT, "uzkge_amd", "csrc", "revealcs_consts.inc")).read()
    rows = re.findall(r"\{((?:0x[0-9a-f]{8}u(?:, )?){8})\}", text)
    vals = [sum(int(w, 16) << (32 * i) for i, w in enumerate(re.findall(r"0x([0-9a-f]{8})u", row))) for row in rows]
    assert vals == [(c << 256) % Q for p in rc.fixed_multiples() for c in p] + [(rc.D << 256) % Q]
    assert rc.fixed_multiples()[255] == ed.mul(1 << 255, ed.G)
