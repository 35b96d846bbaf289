"""GPU: the zk-friendly reveal proofs -- uzk_cp_reveal_prove0_batch, uzk_cp_reveal_verify0_batch and reveal0 / verify_reveal0 of the
Python layer -- bit for bit against tests/anemoi_ref.py composed with tests/ed_ref.py: 65 generated proofs, the two transcripts
rejecting each other's proofs, every verdict at lanes 0, 63 and 64, the identity as (0, 0) in the hash, and a challenge whose hash
lies in the top slice [7 L, r) of the field."""
import functools
import random

import numpy as np
import pytest

import anemoi_ref as a
import ed_ref as e

pytestmark = pytest.mark.gpu
Q, L, G = e.Q, e.L, e.G
M = 65
# A transcript whose hash is >= 7 L (r / L = 7.9995.., so about one hash in eight is): found once on the CPU by walking omega upwards
# from 1000 over this secret and this e1 -- test_a_challenge_from_the_top_slice_of_the_field checks that it still is one.
TOP_SK, TOP_E1_SCALAR, TOP_OMEGA = 0x1234567890ABCDEF1234567, 0xC0FFEE, 1009


def _statements_wire(stmts):
    return e.fr_wire([v for st in stmts for v in st]).reshape(len(stmts), 6, 4)


@functools.lru_cache(maxsize=None)
def _batch():
    """65 valid (statement, proof) pairs of the zk-friendly prover by the restatement, over distinct e1 and ONE key (a prover's batch)
    -- made once, never changed"""
    rng = random.Random("gpu-cp-reveal0")
    sk = rng.randrange(1, L)
    pk = e.keypair_public(sk)
    out = []
    for i in range(M):
        e1 = e.mul(rng.randrange(2, L), G)
        omega = rng.randrange(L)
        reveal, blob = a.prove0(sk, e1, omega)
        out.append(dict(sk=sk, omega=omega, e1=e1, st=(*e1, *reveal, *pk), blob=blob))
    assert len({d["e1"] for d in out}) == M
    return tuple(out)


def _prove0(gpu, sk, e1s, omegas):
    reveal, pk, proofs = gpu.cp_reveal_prove_batch(e.scalars_wire([sk])[0], e.points_wire(e1s), e.scalars_wire(omegas), anemoi=True)
    return e.points_unwire(reveal), e.points_unwire(pk)[0], [bytes(p) for p in proofs]


def test_sixty_five_proofs_byte_for_byte_and_each_transcript_rejects_the_others(gpu):
    batch = _batch()
    sk = batch[0]["sk"]
    e1s, omegas = [d["e1"] for d in batch], [d["omega"] for d in batch]
    reveal, pk, proofs = _prove0(gpu, sk, e1s, omegas)
    assert pk == e.keypair_public(sk) and reveal == [d["st"][2:4] for d in batch]
    assert proofs == [d["blob"] for d in batch]
    wire = _statements_wire([d["st"] for d in batch])
    verdict, ch = gpu.cp_reveal_verify_batch(wire, b"".join(proofs), want_challenges=True, anemoi=True)
    assert not verdict.any()
    want = []
    for d in batch:
        st, (pa, pb, _) = d["st"], e.parse_proof(d["blob"])
        want.append(a.cp0_challenge(st[0:2], G, st[2:4], st[4:6], pa, pb))
    assert np.array_equal(ch, e.raw_wire(want))
    # the Keccak verifier rejects them at an equation, and the zk-friendly verifier rejects Keccak proofs
    keccak = list(gpu.cp_reveal_verify_batch(wire, b"".join(proofs)))
    assert all(v in (4, 5) for v in keccak) and keccak[:3] == [e.verify(d["st"], d["blob"]) for d in batch[:3]]
    _, _, other = gpu.cp_reveal_prove_batch(e.scalars_wire([sk])[0], e.points_wire(e1s), e.scalars_wire(omegas))
    assert not gpu.cp_reveal_verify_batch(wire, other).any()
    back = list(gpu.cp_reveal_verify_batch(wire, other, anemoi=True))
    assert all(v in (4, 5) for v in back) and back[:3] == [a.verify0(d["st"], bytes(other[i])) for i, d in enumerate(batch[:3])]


def _spoiled(d, code):
    """(statement wire row [6, 4], blob, the restatement's verdict) of entry d bent so that the verdict is `code`"""
    st, blob = list(d["st"]), d["blob"]
    pa, pb, r = e.parse_proof(blob)
    row = None
    if code == 1:
        blob = e.make_proof(pa, (pb[0], pb[1] + Q), r) if d["omega"] % 2 else blob
        if not d["omega"] % 2:                                       # a statement word that is not below q: raw words on the wire
            row = _statements_wire([st])[0]
            row[3] = e.raw_wire([Q + 1])[0]
            st[3] = Q + 1
    elif code == 2:
        st[2], st[3] = 2, 3
    elif code == 3:
        st[4], st[5] = e.add((st[4], st[5]), e.ORDER2)
    elif code == 4:
        blob = e.make_proof(pa, pb, (r + 1) % L)
    else:
        e1, reveal, pk = (st[0], st[1]), (st[2], st[3]), (st[4], st[5])
        b_bad = e.mul(d["omega"] + 1, G)
        c = a.cp0_challenge(e1, G, reveal, pk, pa, b_bad)
        blob = e.make_proof(pa, b_bad, (d["omega"] + c * d["sk"]) % L)
    want = a.verify0(tuple(st), blob)
    assert want == code
    return (_statements_wire([st])[0] if row is None else row), blob, want


@pytest.mark.parametrize("turn", range(5))
def test_every_verdict_at_lanes_0_63_64(gpu, turn):
    batch = _batch()
    wire = _statements_wire([d["st"] for d in batch])
    blobs = [d["blob"] for d in batch]
    want = [0] * M
    for slot, lane in enumerate((0, 63, 64)):
        code = (turn + slot) % 5 + 1
        wire[lane], blobs[lane], want[lane] = _spoiled(batch[lane], code)
    assert list(gpu.cp_reveal_verify_batch(wire, b"".join(blobs), anemoi=True)) == want      # only those verdicts change


def test_identity_e1_enters_the_hash_as_zero_zero(gpu):
    """documented, not verified against the reference's arkworks fork: xy() of the identity is None upstream, so (0, 0) is hashed"""
    sk, omega = 1234567, 7654321
    reveal, blob = a.prove0(sk, e.IDENTITY, omega)
    pa, pb, _ = e.parse_proof(blob)
    assert reveal == pa == e.IDENTITY
    st = (*e.IDENTITY, *reveal, *e.keypair_public(sk))
    got_reveal, _, proofs = _prove0(gpu, sk, [e.IDENTITY], [omega])
    assert got_reveal == [e.IDENTITY] and proofs == [blob]
    verdict, ch = gpu.cp_reveal_verify_batch(_statements_wire([st]), blob, want_challenges=True, anemoi=True)
    c = a.eval_variable_length_hash([0, 0, *G, 0, 0, *st[4:6], 0, 0, *pb]) % L
    assert list(verdict) == [0] == [a.verify0(st, blob)] and np.array_equal(ch, e.raw_wire([c]))
    assert c != a.eval_variable_length_hash([0, 1, *G, 0, 1, *st[4:6], 0, 1, *pb]) % L


def test_a_challenge_from_the_top_slice_of_the_field(gpu):
    """floor(r / L) = 7: a hash in [7 L, r) is what the last of the reduction's subtractions is for"""
    assert TOP_OMEGA is not None
    e1 = e.mul(TOP_E1_SCALAR, G)
    reveal, blob = a.prove0(TOP_SK, e1, TOP_OMEGA)
    pk = e.keypair_public(TOP_SK)
    pa, pb, _ = e.parse_proof(blob)
    h = a.eval_variable_length_hash([*e1, *G, *reveal, *pk, *pa, *pb])
    assert 7 * L <= h < a.R
    _, _, proofs = _prove0(gpu, TOP_SK, [e1], [TOP_OMEGA])
    assert proofs == [blob]
    st = (*e1, *reveal, *pk)
    verdict, ch = gpu.cp_reveal_verify_batch(_statements_wire([st]), blob, want_challenges=True, anemoi=True)
    assert list(verdict) == [0] and np.array_equal(ch, e.raw_wire([h - 7 * L]))


def test_reveal0_verify_reveal0_unmask_recover_the_cards(gpu):
    """the Python layer: 4 players, 5 cards"""
    from uzkge_amd import reveal as rv
    rng = random.Random("gpu-cp0-game")
    sks = [rng.randrange(1, L) for _ in range(4)]
    pks = rv.keypair_public(sks)
    joint = rv.aggregate_keys(pks)
    cards = e.rand_subgroup_points(5, "gpu-cp0-cards")
    masked = []
    for card in cards:                                               # ElGamal under the joint key: (r G, card + r PK)
        r = rng.randrange(1, L)
        masked.append((e.mul(r, G), e.add(card, e.mul(r, joint))))
    reveals = []
    for sk, pk in zip(sks, pks):
        omegas = [rng.randrange(L) for _ in cards]
        rcards, proofs, pk_out = rv.reveal0(sk, masked, omegas)
        assert pk_out == pk
        assert proofs[0] == a.prove0(sk, masked[0][0], omegas[0])[1]
        assert rv.verify_reveal0([pk] * 5, masked, rcards, proofs) == [0] * 5
        assert all(v in (4, 5) for v in rv.verify_reveal([pk] * 5, masked, rcards, proofs))
        reveals.append(rcards)
    assert rv.unmask(masked, reveals) == cards
    wrong = [reveals[1][0]] + reveals[0][1:]                         # another player's reveal under this player's proof
    assert rv.verify_reveal0([pks[0]] * 5, masked, wrong, rv.reveal0(sks[0], masked, [5] * 5)[1])[0] != 0
