"""GPU: zshuffle's circuit and its witness on the device (uzk_shuffle_circuit_create / _set_key, uzk_shuffle_witness_batch), held to
tests/shuffle_cs_ref.py -- which tests/test_shuffle_cs_ref_host.py holds to the verifier keys the reference generated -- and, for 20
and 52 cards, to those keys directly and to the golden-pinned verifier: a proof made from the device witness over the literal
circuit is accepted under the reference's own 32 commitments plus the game's 12.

The hook returns 44 evaluation vectors, every one the library lays out: the 40 the table kernels compute (9 q, 5 s, qb, q_ecc, 12 + 12
table columns) and the 4 zero q_prk."""
import random

import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
import plonk_batch_ref as br
import plonk_golden_verifier as gv
import plonk_verifier_oracle as pv
import shuffle_cs_ref as cr
import shuffle_ref as sr
from test_shuffle_cs_ref_host import commit, entries, game, golden_key, pk_tables
from util import affine_of, load_srs

pytestmark = pytest.mark.gpu
R = cr.R
e = sr.e


def wire(vec):
    """integers -> [len, 4] Montgomery words, converting every distinct value once"""
    uniq = sorted(set(vec))
    rows, at = oc.fr_from_ints(uniq), {}
    for i, v in enumerate(uniq):
        at[v] = i
    return rows[[at[v] for v in vec]]


_SRS = {}


def bases(n):
    """(n Lagrange bases, the monomial powers): the reference's files where it has them; below 4096 and above 16384 any valid points
    serve -- the layout tests compare vectors, and the restatement's commitments are made over the same points."""
    if n not in _SRS:
        from uzkge_amd import poly_commit as pc
        name = n if n in (4096, 8192, 16384) else 4096 if n < 4096 else 16384
        lag, _ = load_srs("lagrange-srs-%d.bin" % name)
        lag = np.concatenate([lag] * (n // name)) if n > name else lag[:n]
        mono = pc.srs_params_wire(open(gv.os.path.join(gv.GOLDEN, "srs-padding.bin"), "rb").read(), min(n, 16384))
        if n > 16384:
            mono = np.concatenate([mono[:16384], mono[:n - 16384], mono[16384:]])
        _SRS[n] = (np.ascontiguousarray(lag), mono)
    return _SRS[n]


def make_circuit(cards, k=None):
    from uzkge_amd import backend as b
    from uzkge_amd.shuffle_cs import ShuffleCircuit
    n = b.shuffle_cs_info(cards)["n"]
    lag, mono = bases(n)
    k = [1, 2, 3, 4, 5] if k is None else k                 # any five distinct cosets serve the layout tests
    return ShuffleCircuit.create(cards, lag, mono, oc.fr_from_ints(k))


def root_of(n):
    from uzkge_amd import backend as b
    return oc.fr_to_ints(b.domain_group_gen(n).reshape(1, 4))[0]


def slot_vectors(cs, k, root, pk_entries=None):
    """the restatement's vectors in the hook's order: q (9), s (5), qb, q_prk (4), public-key columns (12), generator columns (12), q_ecc"""
    v = cr.key_vectors(cs, k, root)
    pk_cols = cr.table_columns(cs, pk_entries) if pk_entries is not None else v[20:32]
    return v[:19] + pk_cols + v[20:32] + [v[19]]


@pytest.mark.parametrize("cards", [1, 2, 3, 4, 5, 6, 7, 64])
def test_wiring_permutation_and_every_evaluation_vector(gpu, cards):
    k = [1, 7, 13, 17, 23]
    cir = make_circuit(cards, k)
    try:
        cs = cr.layout(cards)
        n = cs.size
        info = gpu.shuffle_cs_info(cards)
        assert (info["size"], info["n"], info["num_vars"], info["pi_count"]) == (cs.gates, n, cs.num_vars, 8 * cards) and cir.info()[:3] == (n, 19, 43)
        assert info["pi_rows"].tolist() == cs.public_vars_constraint_indices
        wiring, perm, evals = cir.test_tables()
        assert wiring.reshape(-1).tolist() == [v for w in cs.wiring for v in w]
        assert perm.reshape(-1).tolist() == cr.compute_permutation(cs)
        want = slot_vectors(cs, k, root_of(n))
        assert len(want) == evals.shape[0] == 44
        for i, vec in enumerate(want):
            assert np.array_equal(evals[i], wire(vec)), "vector %d" % i
        if cards in (3, 64):                                 # with a key: only the public-key columns change
            pk = e.mul(11 + cards, sr.G)
            with gpu.RemarkKey(e.points_wire([pk])[0]) as key:
                _, _, ev2 = cir.test_tables(key)
            want2 = slot_vectors(cs, k, root_of(n), entries(pk_tables(pk)))
            for i in range(19, 31):
                assert np.array_equal(ev2[i], wire(want2[i])), "public-key column %d" % (i - 19)
            assert np.array_equal(ev2[:19], evals[:19]) and np.array_equal(ev2[31:], evals[31:]) and not np.array_equal(ev2[19], evals[19])
    finally:
        cir.release()


@pytest.fixture(scope="module", params=[20, 52])
def literal(request, gpu):
    """the literal circuit of the reference's deck sizes under the reference's k, one game's key, and the golden verifier key"""
    cards = request.param
    vk, _, _ = gv.load_golden(cards)
    cir = make_circuit(cards, vk["k"])
    pk, deck, digits, perm = game(cards, 900 + cards)
    key = gpu.RemarkKey(e.points_wire([pk])[0])
    yield dict(cards=cards, vk=vk, cir=cir, key=key, pk=pk, deck=deck, digits=digits, perm=perm)
    key.release()
    cir.release()


def test_the_key_commitments_are_the_golden_verifier_key(gpu, literal):
    g = literal
    assert root_of(g["cir"].n) == g["vk"]["root"] and g["cir"].n == g["vk"]["cs_size"]
    assert [affine_of(j) for j in g["cir"].commitments] == golden_key(g["vk"])
    cms = g["cir"].set_key(g["key"])
    lag, _ = bases(g["cir"].n)
    cols = cr.table_columns(cr.layout(g["cards"]), entries(pk_tables(g["pk"])))
    assert [affine_of(j) for j in cms] == [commit(lag, c) for c in cols]
    g["cm_pk"] = [affine_of(j) for j in cms]


def decks_wire(decks):
    e1 = np.stack([e.points_wire([c[0] for c in d]) for d in decks])
    e2 = np.stack([e.points_wire([c[1] for c in d]) for d in decks])
    return e1, e2


def expect_witness(deck, digits, perm, t_pk):
    cs = cr.build_cs(deck, digits, perm, t_pk)
    out, _ = sr.shuffle(deck, digits, perm, t_pk)
    return (wire([v for w in cr.extend_witness(cs) for v in w]), wire([v for w in cr.witness_selectors(cs) for v in w]), wire(cr.public_inputs(cs)),
            e.points_wire([c[0] for c in out]), e.points_wire([c[1] for c in out]))


def run_witness(gpu, cir, key, decks, digits, perms):
    e1, e2 = decks_wire(decks)
    w = cir.witness(key, e1, e2, np.array(digits, dtype=np.uint8), None if perms is None else np.array(perms, dtype=np.uint32))
    try:
        n, B = cir.n, len(decks)
        return (gpu.dev_download(w.d_witness, (B, 5 * n, 4)), gpu.dev_download(w.d_wsel, (B, 3 * n, 4)), w.pi_values, w.e1_out, w.e2_out)
    finally:
        w.release()


@pytest.mark.parametrize("cards", [1, 2, 3, 4, 5, 6, 7, 20])
def test_witness_selectors_inputs_and_decks_are_the_restated_ones(gpu, cards):
    pk, deck, _, rnd = game(cards, 500 + cards)
    _, deck2, _, _ = game(cards, 700 + cards)
    t_pk = pk_tables(pk)
    rng = random.Random(cards)
    draw = lambda: [[rng.randrange(8) for _ in range(sr.ITERATIONS)] for _ in range(cards)]
    const = lambda d: [[d] * sr.ITERATIONS for _ in range(cards)]
    ident, rev, shift = list(range(cards)), list(range(cards))[::-1], [(i + 1) % cards for i in range(cards)]
    cir = make_circuit(cards)
    try:
        with gpu.RemarkKey(e.points_wire([pk])[0]) as key:
            cases = [(deck, draw(), ident), (deck, const(0), rev), (deck, const(7), shift), (deck2, draw(), rnd)]
            for deck_i, dg, pm in cases:
                got = run_witness(gpu, cir, key, [deck_i], [dg], [pm])
                for name, g, w in zip(("witness", "wsel", "pi", "e1", "e2"), got, expect_witness(deck_i, dg, pm, t_pk)):
                    assert np.array_equal(g[0], w), name
            # NULL perms: identities
            none = run_witness(gpu, cir, key, [deck], [cases[0][1]], None)
            first = run_witness(gpu, cir, key, [deck], [cases[0][1]], [ident])
            assert all(np.array_equal(a, c) for a, c in zip(none, first))
            # two different decks and permutations in one call; alone, the first gives lane 0
            two = run_witness(gpu, cir, key, [cases[0][0], cases[3][0]], [cases[0][1], cases[3][1]], [cases[0][2], cases[3][2]])
            for lane, (deck_i, dg, pm) in enumerate((cases[0], cases[3])):
                for name, g, w in zip(("witness", "wsel", "pi", "e1", "e2"), two, expect_witness(deck_i, dg, pm, t_pk)):
                    assert np.array_equal(g[lane], w), (lane, name)
            assert all(np.array_equal(a[0], c[0]) for a, c in zip(two, first))
    finally:
        cir.release()


def check_lanes(gpu, cir, key, t_pk, lanes):
    """one call over the lanes [(deck, digits, perm)]: witness, wire selectors, public inputs and both output decks of every lane
    against the restatement"""
    got = run_witness(gpu, cir, key, [l[0] for l in lanes], [l[1] for l in lanes], [l[2] for l in lanes])
    assert all(g.shape[0] == len(lanes) for g in got)
    for lane, (deck, dg, pm) in enumerate(lanes):
        for name, g, w in zip(("witness", "wsel", "pi", "e1", "e2"), got, expect_witness(deck, dg, pm, t_pk)):
            assert np.array_equal(g[lane], w), (lane, name)
    return got


@pytest.mark.parametrize("cards", [64, 63])
def test_witness_at_the_card_bound(gpu, cards):
    """UZK_SHUFFLE_CS_MAX_CARDS and one below: only here the value kernel sums 64 (63) matrix entries of a row and of a column and
    32 products, the last of them ragged at 63 cards (card 62 has no neighbour).  Three lanes in one call: the identity over all-zero
    digits, the reversal of another deck over all-seven digits, a random permutation over random digits; then the second alone."""
    from uzkge_amd import _native as N
    assert N.SHUFFLE_CS_MAX_CARDS == 64
    pk, deck, _, rnd = game(cards, 500 + cards)
    _, deck2, _, _ = game(cards, 700 + cards)
    t_pk = pk_tables(pk)
    rng = random.Random(cards)
    draw = [[rng.randrange(8) for _ in range(sr.ITERATIONS)] for _ in range(cards)]
    const = lambda d: [[d] * sr.ITERATIONS for _ in range(cards)]
    ident, rev = list(range(cards)), list(range(cards))[::-1]
    assert rnd not in (ident, rev) and sorted(rnd) == ident
    cir = make_circuit(cards)
    try:
        cs = cr.layout(cards)
        assert (cir.n, cs.num_vars) == (32768, {64: 39682}.get(cards, cs.num_vars))
        with gpu.RemarkKey(e.points_wire([pk])[0]) as key:
            lanes = [(deck, const(0), ident), (deck2, const(7), rev), (deck, draw, rnd)]
            got = check_lanes(gpu, cir, key, t_pk, lanes)
            alone = run_witness(gpu, cir, key, [deck2], [const(7)], [rev])
            assert all(np.array_equal(a[0], g[1]) for a, g in zip(alone, got))
    finally:
        cir.release()


def test_the_largest_batch_and_the_refusal_of_one_more(gpu):
    """UZK_SHUFFLE_CS_MAX_BATCH decks of 3 cards in one call, every lane its own deck and digits; three cards have six permutations,
    so the lanes go through all of them in turn.  One deck more is refused before anything is written."""
    import itertools
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    cards, batch = 3, N.SHUFFLE_CS_MAX_BATCH
    assert batch == 64
    pk = game(cards, 41)[0]
    t_pk = pk_tables(pk)
    perms = [list(p) for p in itertools.permutations(range(cards))]
    lanes = [game(cards, 3000 + lane)[1:3] + (perms[lane % len(perms)],) for lane in range(batch)]
    assert len({str(l[0]) for l in lanes}) == len({str(l[1]) for l in lanes}) == batch
    cir = make_circuit(cards)
    n, more = cir.n, batch + 1
    d_w, d_s = gpu.dev_alloc(32 * 5 * n * more), gpu.dev_alloc(32 * 3 * n * more)
    try:
        with gpu.RemarkKey(e.points_wire([pk])[0]) as key:
            check_lanes(gpu, cir, key, t_pk, lanes)
            poison_w, poison_s = np.full((more * 5 * n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full((more * 3 * n, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            gpu.dev_upload(d_w, poison_w)
            gpu.dev_upload(d_s, poison_s)
            over = lanes + lanes[:1]
            e1, e2 = decks_wire([l[0] for l in over])
            with pytest.raises(UzkgeError) as err:
                cir.witness_batch(key, e1, e2, np.array([l[1] for l in over], dtype=np.uint8), np.array([l[2] for l in over], dtype=np.uint32), d_w, d_s)
            assert err.value.code == N.UZK_ERR_PARAMETER and "%d decks" % more in str(err.value)
            assert np.array_equal(gpu.dev_download(d_w, poison_w.shape), poison_w) and np.array_equal(gpu.dev_download(d_s, poison_s.shape), poison_s)
    finally:
        gpu.dev_free(d_w)
        gpu.dev_free(d_s)
        cir.release()


def test_refusals_leave_the_outputs_alone(gpu):
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    cards = 3
    pk, deck, digits, perm = game(cards, 41)
    cir, other = make_circuit(cards), make_circuit(4)
    n = cir.n
    d_w, d_s = gpu.dev_alloc(32 * 5 * n), gpu.dev_alloc(32 * 3 * n)
    poison_w, poison_s = np.full((5 * n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full((3 * n, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    gpu.dev_upload(d_w, poison_w)
    gpu.dev_upload(d_s, poison_s)
    e1, e2 = decks_wire([deck])
    dg = np.array([digits], dtype=np.uint8)
    plain = gpu.Circuit(16, bases(4096)[0][:16], bases(4096)[1][:6], np.arange(80, dtype=np.uint32), oc.fr_from_ints([1, 2, 3, 4, 5]), np.zeros(4, dtype=np.uint64),
                        np.zeros(4, dtype=np.uint64), oc.fr_from_ints([1])[0], [None] * 46)
    try:
        with gpu.RemarkKey(e.points_wire([pk])[0]) as key:
            def refused(circuit=cir, k=key, a=e1, c=e2, d=dg, p=np.array([perm], dtype=np.uint32)):
                with pytest.raises(UzkgeError) as err:
                    circuit.witness_batch(k, a, c, d, p, d_w, d_s) if isinstance(circuit, gpu.ShuffleCircuit) else \
                        gpu.ShuffleCircuit.witness_batch(circuit, k, a, c, d, p, d_w, d_s)
                assert err.value.code == N.UZK_ERR_PARAMETER, str(err.value)
                return str(err.value)
            plain.cards = cards                                     # a circuit not made by uzk_shuffle_circuit_create
            assert "no circuit of uzk_shuffle_circuit_create" in refused(circuit=plain)
            assert "decks of 3 cards, the circuit is for 4" in refused(circuit=other)        # a deck size other than the circuit's
            big = e1.copy()
            big[0, 1, 4:] = e.raw_wire([sr.Q])[0]                   # card 1's y = q
            assert "not below q" in refused(a=big)
            assert "not below q" in refused(c=big)
            d8 = dg.copy()
            d8[0, 2, 83] = 8
            assert "digit 83 of card 2" in refused(d=d8)
            assert "not a permutation" in refused(p=np.array([[0, 0, 1]], dtype=np.uint32))
            assert "not a permutation" in refused(p=np.array([[0, 1, 3]], dtype=np.uint32))
            with pytest.raises(UzkgeError):
                cir.set_key(type("K", (), {"handle": 12345})())
        assert "unknown remask key" in refused(k=type("K", (), {"handle": key.handle})())       # released above
        assert np.array_equal(gpu.dev_download(d_w, (5 * n, 4)), poison_w) and np.array_equal(gpu.dev_download(d_s, (3 * n, 4)), poison_s)
        for bad in (0, 65):
            with pytest.raises(UzkgeError):
                gpu.shuffle_cs_info(bad)
    finally:
        gpu.dev_free(d_w)
        gpu.dev_free(d_s)
        plain.release()
        cir.release()
        other.release()


class Transcript:
    """The prover's side of the reference's transcript over integers (tests/test_gpu_plonk_verifier.py holds the same object for the
    stand-in circuits; tests/plonk_golden_verifier.py pins the transcript itself on the reference's golden proof)."""

    def __init__(self, vk, pi, cards):
        from test_gpu_plonk_verifier import _FiatShamir
        import prover_chain as pch
        self.fs = _FiatShamir(vk, pi, cards, pch.eval_plan(True))
        self.beta_gamma, self.alpha, self.zeta, self.after_evaluations, self.ch = self.fs.beta_gamma, self.fs.alpha, self.fs.zeta, self.fs.after_evaluations, self.fs.ch


def evals_of(rows):
    import prover_chain as pch
    v = pv._ints(rows)
    at = {key: i for i, key in enumerate(pch.eval_plan(True))}
    return {"w": [v[at[("c", i, 0)]] for i in range(5)], "s": [v[at[("t", pch.T_S + i, 0)]] for i in range(4)],
            "prk3": v[at[("t", pch.T_QPRK + 2, 0)]], "prk4": v[at[("t", pch.T_QPRK + 3, 0)]], "z_omega": v[at[("c", 9, 1)]],
            "w_omega": [v[at[("c", i, 1)]] for i in range(3)], "q_ecc": v[at[("t", pch.T_QECC, 0)]], "wsel": [v[at[("c", 5 + i, 0)]] for i in range(3)]}


def blinds(seed):
    rng = random.Random(seed)
    fr = lambda *shape: oc.fr_from_ints([rng.randrange(R) for _ in range(int(np.prod(shape)))]).reshape(shape + (4,))
    bl = {"w": fr(5, 3), "wsel": fr(3, 3), "z": fr(3), "t": fr(5)}
    bl["w"][3:, 2] = 0
    bl["wsel"][:, 2] = 0
    return bl


def prove(g, w, vk, seed=5):
    """one proof through uzkge_amd.shuffle_cs.prove_shuffle; returns (PlonkProof as a dict, its 1632 bytes)"""
    from uzkge_amd.shuffle_cs import prove_shuffle
    pi = pv._ints(w.pi_values[0])
    t = Transcript(vk, pi, g["cards"])
    ch = lambda: {"alpha": t.ch["alpha"], "beta": t.ch["beta"], "gamma": t.ch["gamma"], "zeta": t.ch["zeta"], "anemoi_g": 0, "edwards_a": 1}
    o = prove_shuffle(g["cir"], w, 0, t, lambda rows: oc.fr_from_ints(pv.r_scalars(ch(), vk["k"], vk["cs_size"], evals_of(rows), True)), blinds(seed))
    ev = evals_of(o["evals"])
    proof = {"cm_w": [affine_of(j) for j in o["cm_w_wsel"][:5]], "cm_wsel": [affine_of(j) for j in o["cm_w_wsel"][5:8]],
             "cm_t": [affine_of(j) for j in o["cm_t"]], "cm_z": affine_of(o["cm_z"][0]), "prk3": ev["prk3"], "prk4": ev["prk4"], "w": ev["w"],
             "w_omega": ev["w_omega"], "z_omega": ev["z_omega"], "s": ev["s"], "q_ecc": ev["q_ecc"], "wsel": ev["wsel"],
             "open_zeta": affine_of(o["openings"][0]), "open_zeta_omega": affine_of(o["openings"][1])}
    return proof, gv.proof_to_bytes(proof), pi


def test_a_proof_over_the_literal_circuit_is_accepted_under_the_golden_key(gpu, literal):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    from uzkge_amd.poly_commit import PlonkVerifierKey
    g = literal
    cards, cir, key = g["cards"], g["cir"], g["key"]
    g2 = br.load_g2()
    cm_pk = [affine_of(j) for j in cir.set_key(key)]
    vk = dict(g["vk"], cm_shuffle_public_key=cm_pk)          # the reference's own 32 commitments plus this game's 12
    e1, e2 = decks_wire([g["deck"]])
    args = (key, e1, e2, np.array([g["digits"]], dtype=np.uint8), np.array([g["perm"]], dtype=np.uint32))
    w = cir.witness(*args)
    dev = PlonkVerifierKey(vk, br.prefix(cards))
    other = gpu.RemarkKey(e.points_wire([e.mul(77, sr.G)])[0])
    try:
        out, _ = sr.shuffle(g["deck"], g["digits"], g["perm"], pk_tables(g["pk"]))
        flat = lambda d: [v for c1, c2 in d for v in (c2[0], c2[1], c1[0], c1[1])]
        proof, raw, pi = prove(g, w, vk)
        assert pi == flat(g["deck"]) + flat(out) and len(raw) == 1632
        assert proof["q_ecc"] != 0 and proof["prk3"] == 0    # the remark rows are live; the circuit has no anemoi gate
        assert gv.verify(vk, gv.proof_from_bytes(raw), pi, n_cards=cards, g2=g2)
        accepted, status = dev.verify_batch([raw], [pi], None, g2[0], g2[1])
        assert accepted and list(status) == [0]
        # the next game: set_key to another key, a witness and a proof under it -- accepted under that game's 12 commitments,
        # rejected under the old 12
        cm_other = [affine_of(j) for j in cir.set_key(other)]
        w2 = cir.witness(other, *args[1:])
        try:
            _, raw2, pi2 = prove(g, w2, dict(vk, cm_shuffle_public_key=cm_other))
        finally:
            w2.release()
        assert not dev.verify_batch([raw2], [pi2], None, g2[0], g2[1])[0]
        dev.set_public_key(cm_other)
        assert dev.verify_batch([raw2], [pi2], None, g2[0], g2[1])[0]
        dev.set_public_key(cm_pk)
        cir.set_key(key)
        # one element of the device witness overwritten before round 1
        row = cr.remark_rows(cr.layout(cards))[cards // 2] + 17
        gpu.dev_upload(w.d_witness + 32 * (1 * cir.n + row), oc.fr_from_ints([123456789]))
        try:
            _, raw3, pi3 = prove(g, w, vk)
            accepted, _ = dev.verify_batch([raw3], [pi3], None, g2[0], g2[1])
            assert not accepted
        except UzkgeError as err:
            assert err.code == N.UZK_ERR_COMMITMENT
    finally:
        other.release()
        dev.release()
        w.release()
