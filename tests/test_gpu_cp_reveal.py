"""GPU: the Chaum-Pedersen reveal proofs -- uzk_cp_reveal_verify_batch, uzk_cp_reveal_prove_batch and the Python layer over them -- bit
for bit against tests/ed_ref.py: the reference's golden proof, a batch of 65 generated proofs over distinct e1 != G and several keys,
every verdict at lanes 0, 63 and 64, the prover's bytes, and one statement buffer serving this verifier and the Groth16 fold."""
import functools
import random

import numpy as np
import pytest

import ed_ref as e

pytestmark = pytest.mark.gpu
Q, L, G = e.Q, e.L, e.G
M = 65


def _statements_wire(stmts):
    return e.fr_wire([v for st in stmts for v in st]).reshape(len(stmts), 6, 4)


@functools.lru_cache(maxsize=None)
def _batch():
    """65 valid (statement, proof) pairs by the restatement over distinct e1 != G and five keys -- made once, never changed"""
    rng = random.Random("gpu-cp-reveal")
    sks = [rng.randrange(1, L) for _ in range(5)]
    pks = [e.keypair_public(sk) for sk in sks]
    out = []
    for i in range(M):
        e1 = e.mul(rng.randrange(2, L), G)
        sk, omega = sks[i % 5], rng.randrange(L)
        reveal, blob = e.prove(sk, e1, omega)
        out.append(dict(sk=sk, omega=omega, e1=e1, st=(*e1, *reveal, *pks[i % 5]), blob=blob))
    assert len({d["e1"] for d in out}) == M and all(d["e1"] != G for d in out)
    return tuple(out)


def _spoiled(d, code):
    """(statement wire row [6, 4], blob, the restatement's verdict) of entry d bent so that the verdict is `code`"""
    st, blob = list(d["st"]), d["blob"]
    a, b, r = e.parse_proof(blob)
    row = None
    if code == 1:
        blob = e.make_proof(a, (b[0], b[1] + Q), r) if d["omega"] % 2 else blob
        if not d["omega"] % 2:                                       # a statement word that is not below q: raw words on the wire
            row = _statements_wire([st])[0]
            row[3] = e.raw_wire([Q + 1])[0]
            st[3] = Q + 1
    elif code == 2:
        st[2], st[3] = 2, 3
    elif code == 3:
        st[4], st[5] = e.add((st[4], st[5]), e.ORDER2)
    elif code == 4:
        blob = e.make_proof(a, b, (r + 1) % L)
    else:
        e1, reveal, pk = (st[0], st[1]), (st[2], st[3]), (st[4], st[5])
        b_bad = e.mul(d["omega"] + 1, G)
        c = e.challenge(e1, reveal, pk, a, b_bad)
        blob = e.make_proof(a, b_bad, (d["omega"] + c * d["sk"]) % L)
    want = e.verify(tuple(st), blob)
    assert want == code
    return (_statements_wire([st])[0] if row is None else row), blob, want


def test_the_golden_proof_alone(gpu):
    g = e.golden()
    st = e.golden_statement(g)
    verdict, ch = gpu.cp_reveal_verify_batch(_statements_wire([st]), g["proof"], want_challenges=True)
    assert list(verdict) == [0]
    assert e.verify(st, g["proof"], want_challenge=True) == (0, int(sum(int(ch[0, k]) << (64 * k) for k in range(4))))
    bent = list(st)
    bent[2] = (bent[2] + 1) % Q
    assert list(gpu.cp_reveal_verify_batch(_statements_wire([bent]), g["proof"])) == [e.verify(tuple(bent), g["proof"])] != [0]


def test_sixty_five_proofs_are_accepted_with_the_restatements_challenges(gpu):
    batch = _batch()
    verdict, ch = gpu.cp_reveal_verify_batch(_statements_wire([d["st"] for d in batch]), b"".join(d["blob"] for d in batch), want_challenges=True)
    assert not verdict.any()
    want = []
    for d in batch:
        st, (a, b, _) = d["st"], e.parse_proof(d["blob"])
        want.append(e.challenge(st[0:2], st[2:4], st[4:6], a, b))
    assert np.array_equal(ch, e.raw_wire(want))


@pytest.mark.parametrize("turn", range(5))
def test_every_verdict_at_lanes_0_63_64(gpu, turn):
    batch = _batch()
    wire = _statements_wire([d["st"] for d in batch])
    blobs = [d["blob"] for d in batch]
    want = [0] * M
    for slot, lane in enumerate((0, 63, 64)):
        code = (turn + slot) % 5 + 1
        wire[lane], blobs[lane], want[lane] = _spoiled(batch[lane], code)
    assert list(gpu.cp_reveal_verify_batch(wire, b"".join(blobs))) == want          # only those verdicts change


def test_identity_e1_and_an_unreduced_response(gpu):
    sk, omega = 1234567, 7654321
    reveal, blob = e.prove(sk, e.IDENTITY, omega)
    assert reveal == e.IDENTITY
    d = _batch()[7]
    a, b, r = e.parse_proof(d["blob"])
    longer = e.make_proof(a, b, r + L)
    stmts = [(*e.IDENTITY, *reveal, *e.keypair_public(sk)), d["st"]]
    assert [e.verify(stmts[0], blob), e.verify(stmts[1], longer)] == [0, 0]
    assert list(gpu.cp_reveal_verify_batch(_statements_wire(stmts), blob + longer)) == [0, 0]


def _prove(gpu, sk, e1s, omegas):
    reveal, pk, proofs = gpu.cp_reveal_prove_batch(e.scalars_wire([sk])[0], e.points_wire(e1s), e.scalars_wire(omegas))
    return e.points_unwire(reveal), e.points_unwire(pk)[0], [bytes(p) for p in proofs]


def test_prover_matches_the_restatement_byte_for_byte(gpu):
    batch = _batch()
    sk = batch[0]["sk"]
    e1s, omegas = [d["e1"] for d in batch], [d["omega"] for d in batch]
    reveal, pk, proofs = _prove(gpu, sk, e1s, omegas)
    want = [e.prove(sk, p, w) for p, w in zip(e1s, omegas)]
    assert pk == e.keypair_public(sk)
    assert reveal == [r for r, _ in want] and proofs == [blob for _, blob in want]
    stmts = [(*p, *r, *pk) for p, r in zip(e1s, reveal)]
    assert not gpu.cp_reveal_verify_batch(_statements_wire(stmts), b"".join(proofs)).any()
    assert all(e.verify(st, blob) == 0 for st, blob in zip(stmts, proofs))


@pytest.mark.parametrize("sk", (1, L - 1, 0x1234567890ABCDEF))
def test_prover_edge_inputs(gpu, sk):
    e1s = [d["e1"] for d in _batch()[:3]]
    omegas = [0, L - 1, 99]
    reveal, pk, proofs = _prove(gpu, sk, e1s, omegas)
    want = [e.prove(sk, p, w) for p, w in zip(e1s, omegas)]
    assert pk == e.keypair_public(sk) and reveal == [r for r, _ in want] and proofs == [blob for _, blob in want]
    a, b, _ = e.parse_proof(proofs[0])
    assert a == b == e.IDENTITY                                      # omega = 0
    stmts = [(*p, *r, *pk) for p, r in zip(e1s, reveal)]
    assert not gpu.cp_reveal_verify_batch(_statements_wire(stmts), b"".join(proofs)).any()


def test_reveal_verify_unmask_recovers_the_cards(gpu):
    """the Python layer: 4 players, 5 cards"""
    from uzkge_amd import reveal as rv
    rng = random.Random("gpu-cp-game")
    sks = [rng.randrange(1, L) for _ in range(4)]
    pks = rv.keypair_public(sks)
    assert pks == [e.keypair_public(sk) for sk in sks]
    joint = rv.aggregate_keys(pks)
    assert joint == e.aggregate_keys(pks)
    cards = e.rand_subgroup_points(5, "gpu-cp-cards")
    masked = []
    for card in cards:                                               # ElGamal under the joint key: (r G, card + r PK)
        r = rng.randrange(1, L)
        masked.append((e.mul(r, G), e.add(card, e.mul(r, joint))))
    reveals = []
    for sk, pk in zip(sks, pks):
        rcards, proofs, pk_out = rv.reveal(sk, masked, [rng.randrange(L) for _ in cards])
        assert pk_out == pk
        assert rv.verify_reveal([pk] * 5, masked, rcards, proofs) == [0] * 5
        reveals.append(rcards)
    assert rv.unmask(masked, reveals) == cards
    wrong = [reveals[1][0]] + reveals[0][1:]                         # another player's reveal under this player's proof
    assert rv.verify_reveal([pks[0]] * 5, masked, wrong, rv.reveal(sks[0], masked, [5] * 5)[1])[0] != 0


def test_one_statement_buffer_serves_both_verifiers(gpu):
    """three reveal statements made by uzk_ed_mul_batch go, unchanged, to the Chaum-Pedersen verifier and -- as the public signals --
    to the Groth16 fold over a trapdoor key with simulated proofs"""
    import g16_verify_ref as vr
    rng = random.Random("gpu-cp-both")
    sk = rng.randrange(1, L)
    e1s = e.rand_subgroup_points(3, "gpu-cp-both")
    e1w = e.points_wire(e1s)
    rvw = gpu.ed_mul_batch(e1w, e.scalars_wire([sk] * 3))
    pkw = gpu.ed_mul_batch(e.points_wire([G])[0], e.scalars_wire([sk] * 3))
    buf = np.ascontiguousarray(np.concatenate([e1w, rvw, pkw], axis=1).reshape(3, 6, 4))
    publics = [e.fr_unwire(buf[i]) for i in range(3)]
    assert publics == [[*e1s[i], *e.mul(sk, e1s[i]), *e.keypair_public(sk)] for i in range(3)]
    # the Chaum-Pedersen side
    omegas = [rng.randrange(L) for _ in range(3)]
    _, _, proofs = gpu.cp_reveal_prove_batch(e.scalars_wire([sk])[0], e1w, e.scalars_wire(omegas))
    assert not gpu.cp_reveal_verify_batch(buf, proofs).any()
    # the Groth16 side
    key, trap = vr.trapdoor_vk(7, "cp-both")
    g16 = [vr.simulate(trap, rng.randrange(1, vr.R), rng.randrange(1, vr.R), pub) for pub in publics]
    blobs = [vr.make_blob(p) for p in g16]
    weights = [rng.randrange(1, 1 << 128) for _ in range(3)]
    dk = gpu.Groth16VerifierKey(*vr.key_wire(key))
    try:
        got = dk.fold(b"".join(blobs), buf, vr.weights_wire(weights))
        want = vr.fold(key, blobs, publics, weights)
        assert list(got[5]) == want["status"] == [0, 0, 0]
        assert np.array_equal(got[0], vr.a_wire(want["a"])) and np.array_equal(got[1], vr.b_wire(want["b"]))
        assert tuple(vr.jac_point(got[k]) for k in (2, 3, 4)) == (want["alpha"], want["x"], want["c"])
        assert vr.accepts(key, want)
        accepted, status = dk.verify_batch(b"".join(blobs), buf, vr.weights_wire(weights))
        assert accepted and not status.any()
    finally:
        dk.release()
