"""GPU: masking a card -- uzk_cp_mask_prove_batch, uzk_cp_mask_verify_batch and the Python layer over them -- bit for bit against
tests/shuffle_ref.py: the prover's bytes for 1, 63, 64 and 65 cards with the edge draws (r = 1, the shape of init_masked_cards;
r and omega at 0 and L - 1; the identity as a card), every verdict at lanes 0, 63 and 64 beside accepted neighbours, the challenges,
and the label: a "Revealing" proof over the same numbers is no mask proof."""
import functools
import random

import numpy as np
import pytest

import ed_ref as e
import shuffle_ref as s

pytestmark = pytest.mark.gpu
Q, L, G = e.Q, e.L, e.G
M = 65


@functools.lru_cache(maxsize=None)
def _pk():
    return e.mul(random.Random("gpu-cp-mask-pk").randrange(1, L), G)


@functools.lru_cache(maxsize=None)
def _batch():
    """65 masked cards with their proofs by the restatement -- made once, never changed.  Entry 1: r = 1; 2: r = 0; 3: r = L - 1;
    4: omega = 0; 5: omega = L - 1; 6: the identity as the card."""
    rng = random.Random("gpu-cp-mask")
    pk, out = _pk(), []
    for i in range(M):
        card, r, omega = e.mul(rng.randrange(1, L), G), rng.randrange(1, L), rng.randrange(L)
        r = {1: 1, 2: 0, 3: L - 1}.get(i, r)
        omega = {4: 0, 5: L - 1}.get(i, omega)
        card = e.IDENTITY if i == 6 else card
        masked, blob = s.mask(pk, card, r, omega)
        out.append(dict(card=card, r=r, omega=omega, masked=masked, blob=blob))
    assert out[1]["masked"] == (G, e.add(out[1]["card"], pk)) and out[2]["masked"] == (e.IDENTITY, out[2]["card"])
    return tuple(out)


def _wire(batch):
    pw = e.points_wire
    return pw([d["card"] for d in batch]), pw([d["masked"][0] for d in batch]), pw([d["masked"][1] for d in batch])


def _int(words):
    return sum(int(words[k]) << (64 * k) for k in range(4))


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_prover_bytes(gpu, m):
    batch = _batch()[:m]
    cards, e1, e2 = _wire(batch)
    g1, g2, proofs = gpu.cp_mask_prove_batch(e.points_wire([_pk()])[0], cards, e.scalars_wire([d["r"] for d in batch]), e.scalars_wire([d["omega"] for d in batch]))
    assert np.array_equal(g1, e1) and np.array_equal(g2, e2)
    assert [bytes(p) for p in proofs] == [d["blob"] for d in batch]
    verdict, ch = gpu.cp_mask_verify_batch(e.points_wire([_pk()])[0], cards, g1, g2, proofs, want_challenges=True)
    assert not verdict.any()
    want = []
    for d in batch:
        a, b, _ = e.parse_proof(d["blob"])
        want.append(s.mask_challenge(_pk(), d["masked"][0], e.sub(d["masked"][1], d["card"]), a, b))
    assert np.array_equal(ch, e.raw_wire(want))


def test_one_card_with_r_one(gpu):
    """init_masked_cards: e1 = G, e2 = card + pk"""
    from uzkge_amd import reveal as rv
    d = _batch()[1]
    masked, proofs = rv.mask(_pk(), [d["card"]], [1], [d["omega"]])
    assert masked == [(G, e.add(d["card"], _pk()))] and proofs == [d["blob"]]
    assert rv.verify_mask(_pk(), [d["card"]], masked, proofs) == [0] == [s.verify_mask(_pk(), d["card"], masked[0], proofs[0])]


def _spoiled(d, code):
    """(pk, card, e1, e2 as wire rows, blob, the restatement's verdict) of entry d bent so that the verdict is `code`"""
    pk, card, (e1, e2), blob = _pk(), d["card"], d["masked"], d["blob"]
    a, b, r = e.parse_proof(blob)
    raw_e2 = None
    if code == 1:
        if d["omega"] % 2:
            blob = e.make_proof(a, (b[0], b[1] + Q), r)
        else:                                                        # a statement word that is not below q: raw words on the wire
            e2 = (e2[0], Q + 1)
            raw_e2 = np.concatenate([e.fr_wire([e2[0]])[0], e.raw_wire([Q + 1])[0]])
    elif code == 2:
        card = (2, 3)
    elif code == 3:
        e1 = e.add(e1, e.ORDER2)
    elif code == 4:
        blob = e.make_proof(a, b, (r + 1) % L)
    else:
        b_bad = e.mul(d["omega"] + 1, pk)
        c = s.mask_challenge(pk, e1, e.sub(e2, card), a, b_bad)
        blob = e.make_proof(a, b_bad, (d["omega"] + c * d["r"]) % L)
    want = s.verify_mask(pk, card, (e1, e2), blob)
    assert want == code
    rows = e.points_wire([card, e1, (e2[0], 0) if raw_e2 is not None else e2])
    if raw_e2 is not None:
        rows[2] = raw_e2
    return rows, blob, want


@pytest.mark.parametrize("turn", range(5))
def test_every_verdict_at_lanes_0_63_64(gpu, turn):
    batch = _batch()
    cards, e1, e2 = _wire(batch)
    blobs = [d["blob"] for d in batch]
    want = [0] * M
    for slot, lane in enumerate((0, 63, 64)):
        code = (turn + slot) % 5 + 1
        rows, blobs[lane], want[lane] = _spoiled(batch[lane], code)
        cards[lane], e1[lane], e2[lane] = rows
    assert list(gpu.cp_mask_verify_batch(e.points_wire([_pk()])[0], cards, e1, e2, b"".join(blobs))) == want     # only those verdicts change


def test_a_bad_key_fails_every_proof(gpu):
    batch = _batch()[:3]
    cards, e1, e2 = _wire(batch)
    blobs = b"".join(d["blob"] for d in batch)
    low = e.add(_pk(), e.ORDER2)
    assert list(gpu.cp_mask_verify_batch(e.points_wire([low])[0], cards, e1, e2, blobs)) == [3, 3, 3]
    assert s.verify_mask(low, batch[0]["card"], batch[0]["masked"], batch[0]["blob"]) == 3
    not_canonical = np.concatenate([e.raw_wire([Q])[0], e.fr_wire([1])[0]])
    assert list(gpu.cp_mask_verify_batch(not_canonical, cards, e1, e2, blobs)) == [1, 1, 1]
    other = e.mul(5, _pk())
    got = list(gpu.cp_mask_verify_batch(e.points_wire([other])[0], cards, e1, e2, blobs))
    assert got == [s.verify_mask(other, d["card"], d["masked"], d["blob"]) for d in batch] and 0 not in got


def test_a_reveal_proof_over_the_same_numbers_is_no_mask_proof(gpu):
    """the DL proof of (G, pk; e1, e2 - card) under the label "Revealing": the reveal verifier takes its points in another order, so
    the proof is built here from the restatement's transcript with the label swapped"""
    d, pk = _batch()[9], _pk()
    e1, e2 = d["masked"]
    a, b = e.mul(d["omega"], G), e.mul(d["omega"], pk)
    t = s.mask_transcript_bytes(pk, e1, e.sub(e2, d["card"]), a, b)
    t = e._pad32(b"Revealing") + t[32:]
    c = e.reduce_digest(int.from_bytes(e.keccak256(t), "big"))
    blob = e.make_proof(a, b, (d["omega"] + c * d["r"]) % L)
    cards, w1, w2 = _wire([d, d])
    verdict, ch = gpu.cp_mask_verify_batch(e.points_wire([pk])[0], cards, w1, w2, blob + d["blob"], want_challenges=True)
    assert list(verdict) == [4, 0] == [s.verify_mask(pk, d["card"], d["masked"], blob), 0]
    assert _int(ch[0]) == _int(ch[1]) != c                            # the challenge is the mask transcript's whatever the response


def test_refusals(gpu):
    from uzkge_amd import UzkgeError
    batch = _batch()[:2]
    cards, e1, e2 = _wire(batch)
    pk = e.points_wire([_pk()])[0]
    sc = e.scalars_wire([1, 2])
    bad = cards.copy()
    bad[1, 4:8] = e.raw_wire([Q])[0]
    with pytest.raises(UzkgeError) as err:
        gpu.cp_mask_prove_batch(pk, bad, sc, sc)
    assert "cards[1]" in str(err.value)
    with pytest.raises(UzkgeError):
        gpu.cp_mask_prove_batch(pk, cards[:0], sc[:0], sc[:0])
    with pytest.raises(UzkgeError):
        gpu.cp_mask_verify_batch(pk, cards[:0], e1[:0], e2[:0], b"")
