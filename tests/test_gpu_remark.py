"""GPU: the remask of a shuffle -- uzk_remark_key_create / _tables / uzk_remark_batch and the Python layer over them -- bit for bit
against tests/shuffle_ref.py: the tables of four kinds of key, decks of 1 .. 129 cards (two lanes per card: the wave edge is at 32
cards) with every digit edge, with and without trace and permutation, the chunked trace path beyond 4096 cards, an independent
cross-check through uzk_ed_mul_batch / uzk_ed_sum_batch, the refusals, and a whole game through uzkge_amd/reveal.py."""
import functools
import random

import numpy as np
import pytest

import ed_ref as e
import shuffle_ref as s

pytestmark = pytest.mark.gpu
Q, L, G = e.Q, e.L, e.G
N_MAX = 129
SIZES = [1, 31, 32, 33, 52, 65, 129]


@functools.lru_cache(maxsize=None)
def _pk():
    return e.mul(random.Random("gpu-remark-pk").randrange(1, L), G)


@functools.lru_cache(maxsize=None)
def _deck():
    """129 cards, their digits and the restatement's traces and remasked cards as wire words -- made once, never changed.
    card 0 all digits 0; 1 all digits 7; 2 .. 9 each digit value at iteration 0; 10 .. 17 each at iteration 83; 18 .. 21 e1 = T_G[0][j],
    e2 = T_pk[0][j] with digit +j (the first addition is a doubling); 22 .. 25 the same inputs with digit -j (trace entry 0 is the identity);
    26 e1 = e2 = identity; the rest random."""
    rng = random.Random("gpu-remark-deck")
    pk, t_pk, t_g = _pk(), s.tables(_pk()), s.generator_tables()
    cards = [(e.mul(rng.randrange(1, L), G), e.mul(rng.randrange(1, L), G)) for _ in range(N_MAX)]
    digits = [[rng.randrange(8) for _ in range(84)] for _ in range(N_MAX)]
    digits[0], digits[1] = [0] * 84, [7] * 84
    for v in range(8):
        digits[2 + v][0] = v
        digits[10 + v][83] = v
    for j in range(4):
        cards[18 + j] = cards[22 + j] = (t_g[0][j], t_pk[0][j])
        digits[18 + j][0], digits[22 + j][0] = s.digit_for(j, True), s.digit_for(j, False)
    cards[26] = (e.IDENTITY, e.IDENTITY)
    traces = [s.eval_remark_with_trace(c, d, t_pk) for c, d in zip(cards, digits)]
    for j in range(4):
        assert (traces[18 + j][0][2], traces[18 + j][0][3]) == e.mul(2 * (j + 1), G) and traces[22 + j][0] == (0, 1, 0, 1)
    out = [((t[-1][2], t[-1][3]), (t[-1][0], t[-1][1])) for t in traces]
    return dict(cards=cards, digits=np.array(digits, dtype=np.uint8), e1=e.points_wire([c[0] for c in cards]), e2=e.points_wire([c[1] for c in cards]),
                trace=e.fr_wire([v for t in traces for row in t for v in row]).reshape(N_MAX, 84, 4, 4),
                o1=e.points_wire([o[0] for o in out]), o2=e.points_wire([o[1] for o in out]), out=out)


@pytest.fixture(scope="module")
def key(gpu):
    with gpu.RemarkKey(e.points_wire([_pk()])[0]) as k:
        yield k


def _tables_wire(p):
    return e.fr_wire([v for row in s.table_entries(p) for ent in row for v in ent]).reshape(84, 4, 3, 4)


@pytest.mark.parametrize("kind", ["random", "generator", "identity", "order8"])
def test_tables(gpu, kind):
    p = {"random": _pk(), "generator": G, "identity": e.IDENTITY, "order8": e.order8_point()}[kind]
    with gpu.RemarkKey(e.points_wire([p])[0]) as k:
        tp, tg = k.tables()
        only_pk, none = k.tables(want_gen=False)
    assert none is None and np.array_equal(only_pk, tp)
    assert np.array_equal(tp, _tables_wire(p)) and np.array_equal(tg, _tables_wire(G))
    got = s.tables_unwire(tg)
    for (i, j), want in s.golden_tables().items():                   # the G half is held to the reference's numbers
        assert got[i][j] == want
    if kind == "generator":
        assert np.array_equal(tp, tg)
    if kind == "order8":                                             # the tables collapse to the identity after the first doublings
        t8 = s.tables_unwire(tp)
        assert all(t8[i][j] == (0, 1, 0) for i in range(1, 84) for j in range(4)) and t8[0][0][:2] == p


def _perms(n):
    rng = random.Random("gpu-remark-perm-%d" % n)
    rnd = list(range(n))
    rng.shuffle(rnd)
    return [None, list(range(n)), list(range(n - 1, -1, -1)), rnd]


@pytest.mark.parametrize("n", SIZES)
def test_remask_with_trace_and_permutations(gpu, key, n):
    d = _deck()
    for perm in _perms(n):
        o1, o2, tr = key.remark_batch(d["e1"][:n], d["e2"][:n], d["digits"][:n], perm, want_trace=True)
        idx = list(range(n)) if perm is None else perm
        assert np.array_equal(tr, d["trace"][:n])                    # the trace stays in input order
        assert np.array_equal(o1, d["o1"][idx]) and np.array_equal(o2, d["o2"][idx])
        p1, p2, none = key.remark_batch(d["e1"][:n], d["e2"][:n], d["digits"][:n], perm, want_trace=False)
        assert none is None and np.array_equal(p1, o1) and np.array_equal(p2, o2)      # trace_out = NULL gives the same deck


def test_remask_beyond_one_trace_chunk(gpu, key):
    """4097 cards: a remask with trace runs 4096 cards per launch; the deck is the 129 cards over and over"""
    d, n = _deck(), 4097
    idx = np.arange(n) % N_MAX
    perm = np.arange(n - 1, -1, -1, dtype=np.uint32)
    o1, o2, tr = key.remark_batch(d["e1"][idx], d["e2"][idx], d["digits"][idx], perm, want_trace=True)
    assert np.array_equal(tr, d["trace"][idx])
    assert np.array_equal(o1, d["o1"][idx[perm]]) and np.array_equal(o2, d["o2"][idx[perm]])
    p1, p2, _ = key.remark_batch(d["e1"][idx], d["e2"][idx], d["digits"][idx], perm)
    assert np.array_equal(p1, o1) and np.array_equal(p2, o2)


def test_remask_is_the_equivalent_scalar_by_the_existing_kernels(gpu, key):
    """on subgroup points the output is e1 + (rho mod L) G and e2 + (rho mod L) pk: uzk_ed_mul_batch and uzk_ed_sum_batch say so"""
    d, n = _deck(), 65
    rho = e.scalars_wire([s.remark_scalar([int(v) for v in row]) % L for row in d["digits"][:n]])
    o1, o2, _ = key.remark_batch(d["e1"][:n], d["e2"][:n], d["digits"][:n])
    rg = gpu.ed_mul_batch(e.points_wire([G])[0], rho)
    rpk = gpu.ed_mul_batch(e.points_wire([_pk()])[0], rho)
    assert np.array_equal(gpu.ed_sum_batch(np.stack([d["e1"][:n], rg])), o1)
    assert np.array_equal(gpu.ed_sum_batch(np.stack([d["e2"][:n], rpk])), o2)
    assert not gpu.ed_check_points(np.concatenate([o1, o2])).any()


def test_python_layer_matches(gpu):
    from uzkge_amd import reveal as rv
    d, n = _deck(), 5
    perm = [3, 0, 4, 1, 2]
    with rv.remark_key(_pk()) as k:
        deck, traces = rv.shuffle(k, d["cards"][:n], d["digits"][:n].tolist(), perm, want_trace=True)
        assert rv.shuffle(k, d["cards"][:n], d["digits"][:n].tolist(), perm) == deck
    assert k.handle == 0
    assert deck == [d["out"][i] for i in perm]
    want = s.trace_unwire(d["trace"][:n], n)
    assert traces == want and all(len(t) == 84 for t in traces)


def test_refusals(gpu, key):
    from uzkge_amd import UzkgeError
    d = _deck()
    e1, e2, dg = d["e1"][:3], d["e2"][:3], d["digits"][:3]

    def refused(*args, **kw):
        with pytest.raises(UzkgeError) as err:
            key.remark_batch(*args, **kw)
        assert err.value.kind == "ParameterError", err.value
        return str(err.value)

    eight = dg.copy()
    eight[2, 40] = 8
    assert "digit 40 of card 2" in refused(e1, e2, eight)
    assert "not a permutation" in refused(e1, e2, dg, [0, 1, 1])
    assert "not a permutation" in refused(e1, e2, dg, [0, 1, 3])
    assert "0 cards" in refused(e1[:0], e2[:0], dg[:0])
    bad = e2.copy()
    bad[1, 0:4] = e.raw_wire([Q])[0]
    assert "e2[1]" in refused(e1, bad, dg)
    with pytest.raises(UzkgeError):
        gpu.RemarkKey(bad[1])
    gone = gpu.RemarkKey(e.points_wire([G])[0])
    handle = gone.handle
    gone.release()
    gone.handle = handle
    with pytest.raises(UzkgeError) as err:
        gone.remark_batch(e1, e2, dg)
    assert "unknown remask key" in str(err.value)
    with pytest.raises(UzkgeError):
        gone.tables()
    with pytest.raises(UzkgeError):
        gone.release()
    gone.handle = 0
    o1, _, _ = key.remark_batch(e1, e2, dg)                          # the library is as it was
    assert np.array_equal(o1, d["o1"][:3])


def test_a_game_of_four_players_and_five_cards(gpu):
    """keys -> joint key -> masked deck -> each player's shuffle -> reveals -> unmask, through uzkge_amd/reveal.py only"""
    from uzkge_amd import reveal as rv
    rng = random.Random("gpu-remark-game")
    players, n = 4, 5
    sks = [rng.randrange(1, L) for _ in range(players)]
    pks = rv.keypair_public(sks)
    joint = rv.aggregate_keys(pks)
    cards = rv.keypair_public([rng.randrange(1, L) for _ in range(n)])                   # five distinct subgroup points
    deck, proofs = rv.mask(joint, cards, [1] * n, [rng.randrange(L) for _ in range(n)])
    assert rv.verify_mask(joint, cards, deck, proofs) == [0] * n
    assert all(c[0] == G for c in deck)                              # r = 1: init_masked_cards
    origin = list(range(n))                                          # origin[i]: the card at position i of the current deck
    with rv.remark_key(joint) as key:
        for _ in range(players):
            digits = [[rng.randrange(8) for _ in range(84)] for _ in range(n)]
            perm = list(range(n))
            rng.shuffle(perm)
            new = rv.shuffle(key, deck, digits, perm)
            assert all(a != b for a, b in zip(new, [deck[i] for i in perm]))             # every card re-randomised
            deck, origin = new, [origin[i] for i in perm]
    reveals = []
    for sk, pk in zip(sks, pks):
        cards_k, proofs_k, pk_k = rv.reveal(sk, deck, [rng.randrange(L) for _ in range(n)])
        assert pk_k == pk and rv.verify_reveal([pk] * n, deck, cards_k, proofs_k) == [0] * n
        reveals.append(cards_k)
    assert rv.unmask(deck, reveals) == [cards[i] for i in origin]
    assert sorted(origin) == list(range(n))
