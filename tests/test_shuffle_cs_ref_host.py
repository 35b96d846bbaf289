"""tests/shuffle_cs_ref.py, the restatement of zshuffle's circuit, held to the reference's own generated verifier keys.

tests/golden/plonk_52_golden.json and plonk_20_golden.json carry what `gen-params` produced for the two deck sizes: 32 commitments,
k, the root and the root power of every public-input row.  A commitment of an evaluation vector over the reference's Lagrange SRS
is a function of every entry of the vector, and the s vectors are a function of every wire of every row -- so a layout that
reproduces all 32 bit for bit is the reference's layout, with no Rust run.  The witness side is held to the restated
verify_witness for every remainder of the chunks of 3 and of 2."""
import random

import pytest

import oracle_c as oc
import plonk_golden_verifier as gv
import shuffle_cs_ref as cr
import shuffle_ref as sr
from util import affine_of, load_srs

R = cr.R


def golden_key(vk):
    return vk["cm_q"] + vk["cm_s"] + [vk["cm_qb"]] + vk["cm_prk"] + [vk["cm_q_ecc"]] + vk["cm_shuffle_generator"]


def commit(lagrange_wire, vec):
    if not any(vec):
        return None
    return affine_of(oc.msm_pippenger(lagrange_wire, oc.fr_from_ints(vec), 0, 4))


@pytest.mark.parametrize("cards,size", [(52, 14094), (20, 3302)])
def test_the_restated_tables_commit_to_the_golden_verifier_key(cards, size):
    vk, _, _ = gv.load_golden(cards)
    cs = cr.layout(cards)
    assert cs.gates == size == cr.gate_count(cards) and cs.size == vk["cs_size"]
    group = cr.domain(cs.size, vk["root"])
    assert [group[i] for i in cs.public_vars_constraint_indices] == vk["pi_root_powers"]
    assert len(cs.public_vars_constraint_indices) == 8 * cards
    vecs = cr.key_vectors(cs, vk["k"], vk["root"])
    want = golden_key(vk)
    assert len(vecs) == len(want) == 32 == sum(c for _, c in cr.KEY_ORDER)
    wire, _ = load_srs("lagrange-srs-%d.bin" % cs.size)
    for i, (vec, w) in enumerate(zip(vecs, want)):
        assert commit(wire, vec) == w, "commitment %d" % i
    assert all(w is None for w in vk["cm_prk"]) and all(w is not None for j, w in enumerate(want) if not 15 <= j < 19 and j != 7)
    assert want[7] is None                                   # selector 7 is zero everywhere: q_ecc is the indexer's marker


def game(cards, seed, perm=None):
    rng = random.Random(seed)
    pk = sr.e.mul(rng.randrange(1, sr.L), sr.G)
    pts = sr.e.rand_subgroup_points(2 * cards, seed)
    deck = [(pts[2 * i], pts[2 * i + 1]) for i in range(cards)]
    digits = [[rng.randrange(8) for _ in range(sr.ITERATIONS)] for _ in range(cards)]
    if perm is None:
        perm = list(range(cards))
        rng.shuffle(perm)
    return pk, deck, digits, perm


_PK_TABLES = {}


def pk_tables(pk):
    if pk not in _PK_TABLES:
        _PK_TABLES[pk] = sr.tables(pk)
    return _PK_TABLES[pk]


def entries(tables):
    return [[sr.entry(t) for t in row] for row in tables]


@pytest.mark.parametrize("cards", [1, 2, 3, 4, 5, 6, 7, 20])
def test_the_restated_witness_satisfies_the_restated_circuit(cards):
    pk, deck, digits, perm = game(cards, 100 + cards)
    t_pk = pk_tables(pk)
    cs = cr.build_cs(deck, digits, perm, t_pk)
    assert cs.gates == cr.gate_count(cards)
    lay = cr.layout(cards)
    assert cs.wiring == lay.wiring and cs.selectors == lay.selectors and cs.num_vars == lay.num_vars       # the layout is a function of N
    assert cs.public_vars_constraint_indices == lay.public_vars_constraint_indices
    assert cs.boolean_constraint_indices == lay.boolean_constraint_indices
    pi = cr.public_inputs(cs)
    out, _ = sr.shuffle(deck, digits, perm, t_pk)
    flat = lambda d: [v for e1, e2 in d for v in (e2[0], e2[1], e1[0], e1[1])]
    assert pi == flat(deck) + flat(out)                      # verify_shuffle's online inputs: the deck, then the new deck
    assert cr.verify_witness(cs, cs.witness, pi, entries(t_pk)) is None
    ext, wsel = cr.extend_witness(cs), cr.witness_selectors(cs)
    assert len(ext) == 5 and all(len(w) == cs.size for w in ext) and len(wsel) == 3
    assert all(set(v) <= {0, 1} for v in wsel[:2]) and set(wsel[2]) <= {0, 1, R - 1}


@pytest.mark.parametrize("cards", [3, 4])
def test_a_wrong_witness_fails_the_restated_circuit(cards):
    pk, deck, digits, perm = game(cards, 7)
    t_pk = pk_tables(pk)
    cs = cr.build_cs(deck, digits, perm, t_pk)
    pi, ent = cr.public_inputs(cs), entries(t_pk)
    assert cr.verify_witness(cs, cs.witness, pi, ent) is None
    row = cr.remark_rows(cs)[1]
    bad = list(cs.witness)
    bad[cs.wiring[0][row + 40]] = (bad[cs.wiring[0][row + 40]] + 1) % R          # one trace value
    assert "remark equation" in cr.verify_witness(cs, bad, pi, ent)
    # a doubled matrix row: the "permutation" takes card perm[0] twice; every row still sums to one, a column does not
    twice = list(perm)
    twice[1] = twice[0]
    cs2 = cr.build_cs(deck, digits, twice, t_pk)
    msg = cr.verify_witness(cs2, cs2.witness, cr.public_inputs(cs2), ent)
    assert msg is not None and "gate equation" in msg
    assert cr.verify_witness(cs, cs.witness, pi[:-1] + [(pi[-1] + 1) % R], ent) is not None
    # under another key's tables the same trace does not hold
    other = entries(pk_tables(sr.e.mul(5, sr.G)))
    assert "remark equation" in cr.verify_witness(cs, cs.witness, pi, other)


def test_the_bucketed_permutation_is_the_reference_scan():
    cs = cr.layout(2)
    n, flat = cs.size, [v for w in cs.wiring for v in w]
    perm = [0] * (5 * n)
    marked = set()
    for i, value in enumerate(flat):                         # constraint_system/mod.rs:76-90, as written
        if value in marked:
            continue
        prev = i
        for j in range(i + 1, len(flat)):
            if flat[j] == value:
                perm[prev] = j
                prev = j
        perm[prev] = i
        marked.add(value)
    assert perm == cr.compute_permutation(cs)
