"""GPU: a shuffle circuit and a matchmaking circuit alive in one context, their calls interleaved.  The two modules share their
resident layout, their table and gather kernels and the code that hangs a layout on a circuit (uzkge_amd/csrc/cs_common.hpp); the
per-circuit tests cannot see one circuit's resident block, workspace or tag being taken for the other's.  Every result is held to the
restatements (tests/shuffle_cs_ref.py, tests/match_cs_ref.py), and the witnesses after the table calls to the ones before.

3 cards: an odd count, so the last product of a row has a single term; n = 512.  5 players: the smallest size with two cipher
permutations and the extra sigma gate; n = 128."""
import numpy as np
import pytest

import match_cs_ref as mr
import shuffle_cs_ref as cr
import shuffle_ref as sr
import test_gpu_match_cs as tm
import test_gpu_shuffle_cs as ts
from test_match_cs_ref_host import built, match
from test_shuffle_cs_ref_host import commit, entries, game, pk_tables
from util import affine_of

pytestmark = pytest.mark.gpu
CARDS, PLAYERS, K = 3, 5, [1, 7, 13, 17, 23]


def test_two_circuits_interleaved_give_the_restated_results(gpu):
    pk, deck, digits, perm = game(CARDS, 41)
    _, deck2, digits2, perm2 = game(CARDS, 42)
    t_pk = pk_tables(pk)
    decks, dgs, perms = [deck, deck2], [digits, digits2], [perm, perm2]
    ms = [match(PLAYERS, 61), match(PLAYERS, 62)]
    want_s = [ts.expect_witness(d, g, p, t_pk) for d, g, p in zip(decks, dgs, perms)]
    want_m = [tm.expect(m) for m in ms]
    shuffle, matching = ts.make_circuit(CARDS, K), tm.make_circuit(PLAYERS, K)
    key = gpu.RemarkKey(sr.e.points_wire([pk])[0])
    try:
        assert (shuffle.n, matching.n) == (512, 128)

        def witnesses():
            s = ts.run_witness(gpu, shuffle, key, decks, dgs, perms)
            m = tm.run_witness(gpu, matching, ms)
            for lane in range(2):
                for name, g, w in zip(("witness", "wsel", "pi", "e1", "e2"), s, want_s[lane]):
                    assert np.array_equal(g[lane], w), ("shuffle", lane, name)
                for name, g, w in zip(("witness", "pi", "outputs", "commitment"), m, want_m[lane]):
                    assert np.array_equal(g[lane], w), ("matchmaking", lane, name)
            return s, m
        first = witnesses()
        # the game's public-key tables into the shuffle circuit, then both circuits' tables, the matchmaking circuit's first
        cs_s, cs_m = cr.layout(CARDS), built(PLAYERS, zero=True)
        pk_cols = cr.table_columns(cs_s, entries(t_pk))
        lag, _ = ts.bases(shuffle.n)
        assert [affine_of(j) for j in shuffle.set_key(key)] == [commit(lag, c) for c in pk_cols]
        wiring, prm, evals = matching.test_tables()
        assert wiring.reshape(-1).tolist() == [v for w in cs_m.wiring for v in w] and prm.reshape(-1).tolist() == mr.compute_permutation(cs_m)
        want = mr.key_vectors(cs_m, K, ts.root_of(matching.n))
        assert len(want) == evals.shape[0] == 19
        for i, vec in enumerate(want):
            assert np.array_equal(evals[i], ts.wire(vec)), "matchmaking vector %d" % i
        wiring, prm, evals = shuffle.test_tables(key)
        assert wiring.reshape(-1).tolist() == [v for w in cs_s.wiring for v in w] and prm.reshape(-1).tolist() == cr.compute_permutation(cs_s)
        want = ts.slot_vectors(cs_s, K, ts.root_of(shuffle.n), entries(t_pk))
        assert len(want) == evals.shape[0] == 44
        for i, vec in enumerate(want):
            assert np.array_equal(evals[i], ts.wire(vec)), "shuffle vector %d" % i
        second = witnesses()
        for a, b in zip(first[0] + first[1], second[0] + second[1]):
            assert np.array_equal(a, b)
    finally:
        key.release()
        shuffle.release()
        matching.release()
