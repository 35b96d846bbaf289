"""The Baby Jubjub side of a zshuffle game over arrays of cards, with the reference's names: the plain reveal path
(shuffle/src/reveal.rs, keygen.rs; RevealVerifier.sol), masking (shuffle/src/mask.rs) and the remask of a shuffle
(uzkge/src/shuffle/remark.rs).  Every function is one call of the Baby Jubjub layer of the C ABI (include/uzkge_gpu.h, uzk_ed_* /
uzk_cp_* / uzk_remark_*).

Points are affine integer pairs (x, y) below q, the identity is (0, 1); a masked card is (e1, e2); secrets and omegas are integers below
the subgroup order L; a proof is the 160 bytes of ChaumPedersenDLProof::to_uncompress.  The library draws no randomness: the caller
supplies one omega per card, as it supplies the fold weights of the batch verifiers."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import _native as N
from . import backend as b

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
GENERATOR = (0x2B8CFD91B905CAE31D41E7DEDF4A927EE3BC429AAD7E344D59D2810D82876C32, 0x2AAA6C24A758209E90ACED1F10277B762A7C1115DBC0E16AC276FC2C671A861F)
_R = (1 << 256) % Q
_R_INV = pow(_R, -1, Q)
_MASK = (1 << 64) - 1

Point = Tuple[int, int]


def _words(v: int) -> List[int]:
    return [(v >> (64 * k)) & _MASK for k in range(4)]


def points_to_wire(points: Sequence[Point]) -> np.ndarray:
    """[n, 8]: x then y, Montgomery words"""
    out = np.zeros((len(points), 8), dtype=np.uint64)
    for i, (x, y) in enumerate(points):
        if not (0 <= x < Q and 0 <= y < Q):
            raise ValueError("point %d: a coordinate is not below q" % i)
        out[i] = _words(x * _R % Q) + _words(y * _R % Q)
    return out


def points_from_wire(wire: np.ndarray) -> List[Point]:
    w = np.asarray(wire, dtype=np.uint64).reshape(-1, 2, 4)
    val = lambda r: sum(int(r[k]) << (64 * k) for k in range(4)) * _R_INV % Q
    return [(val(p[0]), val(p[1])) for p in w]


def scalars_to_wire(scalars: Sequence[int]) -> np.ndarray:
    """[n, 4]: plain 256-bit integers, little-endian words"""
    out = np.zeros((len(scalars), 4), dtype=np.uint64)
    for i, s in enumerate(scalars):
        if not 0 <= s < (1 << 256):
            raise ValueError("scalar %d does not fit 256 bits" % i)
        out[i] = _words(s)
    return out


def statements_to_wire(pks: Sequence[Point], e1s: Sequence[Point], reveal_cards: Sequence[Point]) -> np.ndarray:
    """[m, 6, 4]: e1, reveal, pk -- also the public signals of the Groth16 reveal proof of the same statement"""
    rows = [p for e1, rv, pk in zip(e1s, reveal_cards, pks) for p in (e1, rv, pk)]
    return points_to_wire(rows).reshape(len(e1s), 6, 4)


def _decoded(who: str, raw: bytes, check_subgroup: bool) -> List[Point]:
    from . import codec
    wire, status = codec.ed_decompress(raw, check_subgroup)
    bad = np.flatnonzero(status)
    if bad.size:
        raise ValueError("%s: point %d: status %d (1 not a canonical encoding, 2 not on the curve, 3 outside the prime-order subgroup)"
                         % (who, int(bad[0]), int(status[bad[0]])))
    return points_from_wire(wire)


def points_from_hex(strings: Sequence[str], check_subgroup: bool = True) -> List[Point]:
    """The SDK's point strings (shuffle/src/utils.rs hex_to_point: the hex of ark-serialize's 32 compressed bytes, with or without
    "0x") decoded on the device in one call (uzk_ed_decompress_batch).  check_subgroup: what Validate::Yes adds to the curve check."""
    raw = b"".join(bytes.fromhex(s[2:] if s.startswith("0x") else s) for s in strings)
    if len(raw) != 32 * len(strings):
        raise ValueError("a point string is 32 bytes")
    return _decoded("points_from_hex", raw, check_subgroup) if strings else []


def points_to_hex(points: Sequence[Point], with_start: bool = True) -> List[str]:
    """point_to_hex of every point (uzk_ed_compress_batch)"""
    from . import codec
    if not len(points):
        return []
    enc, _ = codec.ed_compress(points_to_wire(points))              # points_to_wire refuses what status 1 would report
    return [("0x" if with_start else "") + bytes(row).hex() for row in enc]


def points_from_y(ys: Sequence[int], greatest: bool = True) -> List[Point]:
    """index_to_point over a table of the caller's: the point with y = ys[i] and the larger (greatest) or smaller of its two x
    (get_point_from_y_unchecked(y, greatest)), all in one call.  Neither the curve's cofactor nor the table is checked beyond the
    curve equation: a y with no point is refused."""
    if any(not 0 <= y < Q for y in ys):
        raise ValueError("a y coordinate is not below q")
    # y = +-1 has x = 0 alone: no sign to choose, and the strict decoder takes no sign bit on it
    raw = b"".join((y | (int(bool(greatest) and y not in (1, Q - 1)) << 255)).to_bytes(32, "little") for y in ys)
    return _decoded("points_from_y", raw, False) if len(ys) else []


def keypair_public(sks: Sequence[int]) -> List[Point]:
    """pk = sk G for every secret"""
    return points_from_wire(b.ed_mul_batch(points_to_wire([GENERATOR])[0], scalars_to_wire(sks)))


def aggregate_keys(pks: Sequence[Point]) -> Point:
    """the joint key: the sum of the players' keys (RevealVerifier.aggregateKeys)"""
    return points_from_wire(b.ed_sum_batch(points_to_wire(pks).reshape(len(pks), 1, 8)))[0]


def reveal(sk: int, masked_cards: Sequence[Tuple[Point, Point]], omegas: Sequence[int]):
    """One player's reveals of the masked cards (e1, e2): (reveal cards, proofs, pk).  omegas: one fresh uniform integer below L per
    card, drawn by the caller and never reused."""
    if len(omegas) != len(masked_cards):
        raise ValueError("one omega per card")
    rv, pk, proofs = b.cp_reveal_prove_batch(scalars_to_wire([sk])[0], points_to_wire([c[0] for c in masked_cards]), scalars_to_wire(omegas))
    return points_from_wire(rv), [bytes(p) for p in proofs], points_from_wire(pk)[0]


def verify_reveal(pks: Sequence[Point], masked_cards: Sequence[Tuple[Point, Point]], reveal_cards: Sequence[Point], proofs: Sequence[bytes]) -> List[int]:
    """The verdict of every (pk, masked card, reveal card, proof): 0 accepted, else the first failing check (uzk_cp_reveal_verify_batch)."""
    if not len(pks) == len(masked_cards) == len(reveal_cards) == len(proofs):
        raise ValueError("one key, one masked card and one proof per reveal card")
    if any(len(p) != N.CP_PROOF_BYTES for p in proofs):
        raise ValueError("a proof is %d bytes" % N.CP_PROOF_BYTES)
    st = statements_to_wire(pks, [c[0] for c in masked_cards], reveal_cards)
    return [int(v) for v in b.cp_reveal_verify_batch(st, b"".join(proofs))]


def reveal0(sk: int, masked_cards: Sequence[Tuple[Point, Point]], omegas: Sequence[int]):
    """The zk-friendly reveal (reveal.rs reveal0 over dl.rs prove0): `reveal` with the Anemoi-Jive hash of the twelve coordinates as
    the challenge in place of the Keccak transcript; the same blob."""
    if len(omegas) != len(masked_cards):
        raise ValueError("one omega per card")
    rv, pk, proofs = b.cp_reveal_prove_batch(scalars_to_wire([sk])[0], points_to_wire([c[0] for c in masked_cards]), scalars_to_wire(omegas), anemoi=True)
    return points_from_wire(rv), [bytes(p) for p in proofs], points_from_wire(pk)[0]


def verify_reveal0(pks: Sequence[Point], masked_cards: Sequence[Tuple[Point, Point]], reveal_cards: Sequence[Point], proofs: Sequence[bytes]) -> List[int]:
    """`verify_reveal` for the proofs of reveal0 (uzk_cp_reveal_verify0_batch): the same verdict codes."""
    if not len(pks) == len(masked_cards) == len(reveal_cards) == len(proofs):
        raise ValueError("one key, one masked card and one proof per reveal card")
    if any(len(p) != N.CP_PROOF_BYTES for p in proofs):
        raise ValueError("a proof is %d bytes" % N.CP_PROOF_BYTES)
    st = statements_to_wire(pks, [c[0] for c in masked_cards], reveal_cards)
    return [int(v) for v in b.cp_reveal_verify_batch(st, b"".join(proofs), anemoi=True)]


def reveal_with_snark(sk: int, masked_cards: Sequence[Tuple[Point, Point]], circuit, r: Sequence[int], s: Sequence[int], finish: str = "host"):
    """One player's reveals with a Groth16 proof each (sdk.rs reveal_card_with_snark; RevealVerifier.sol): (reveal cards, proofs, pk).
    circuit: a reveal_cs.RevealCircuit; r, s: one pair of fresh uniform integers below the scalar field's order per card, drawn by the
    caller.  A proof is the 256-byte blob Groth16VerifierKey.verify_batch takes, with the public inputs e1.x e1.y reveal.x reveal.y
    pk.x pk.y of its card.  finish="device": the proofs are finished and encoded on the device; the same blobs."""
    if len(r) != len(masked_cards) or len(s) != len(masked_cards):
        raise ValueError("one pair of blinds per card")
    statements, proofs = circuit.prove(sk, [c[0] for c in masked_cards], r, s, finish=finish)
    return [(st[2], st[3]) for st in statements], proofs, (statements[0][4], statements[0][5])


def unmask(masked_cards: Sequence[Tuple[Point, Point]], reveal_cards: Sequence[Sequence[Point]]) -> List[Point]:
    """card_j = e2_j minus every player's reveal of card j; reveal_cards[k][j] is player k's reveal of card j"""
    n = len(masked_cards)
    if any(len(row) != n for row in reveal_cards):
        raise ValueError("every player reveals every card")
    rows = np.stack([points_to_wire(row) for row in reveal_cards])
    return points_from_wire(b.ed_unmask_batch(points_to_wire([c[1] for c in masked_cards]), rows))


def remark_key(pk: Point) -> b.RemarkKey:
    """the remask tables of the joint key, built once per game; a context manager"""
    return b.RemarkKey(points_to_wire([pk])[0])


def mask(pk: Point, cards: Sequence[Point], rs: Sequence[int], omegas: Sequence[int]):
    """(masked cards (e1, e2), proofs) of the cards under the joint key: e1 = r G, e2 = card + r pk with a "Masking" proof each.  rs and
    omegas: one integer below L per card, drawn by the caller (init_masked_cards uses r = 1)."""
    if not len(cards) == len(rs) == len(omegas):
        raise ValueError("one r and one omega per card")
    e1, e2, proofs = b.cp_mask_prove_batch(points_to_wire([pk])[0], points_to_wire(cards), scalars_to_wire(rs), scalars_to_wire(omegas))
    return list(zip(points_from_wire(e1), points_from_wire(e2))), [bytes(p) for p in proofs]


def verify_mask(pk: Point, cards: Sequence[Point], masked_cards: Sequence[Tuple[Point, Point]], proofs: Sequence[bytes]) -> List[int]:
    """The verdict of every (card, masked card, proof) under the joint key: 0 accepted, else the first failing check
    (uzk_cp_mask_verify_batch)."""
    if not len(cards) == len(masked_cards) == len(proofs):
        raise ValueError("one masked card and one proof per card")
    if any(len(p) != N.CP_PROOF_BYTES for p in proofs):
        raise ValueError("a proof is %d bytes" % N.CP_PROOF_BYTES)
    wire = points_to_wire
    return [int(v) for v in b.cp_mask_verify_batch(wire([pk])[0], wire(cards), wire([c[0] for c in masked_cards]), wire([c[1] for c in masked_cards]),
                                                   b"".join(proofs))]


def remark_scalar(digits: Sequence[int]) -> int:
    """rho = sum_i +-(j_i + 1) 16^i of one card's 84 digits (bits 0, 1: j; bit 2 set: +): the remasked card is (e1 + rho G, e2 + rho pk)"""
    if len(digits) != N.REMARK_ITERATIONS:
        raise ValueError("%d digits per card" % N.REMARK_ITERATIONS)
    if any(not 0 <= d <= 7 for d in digits):
        raise ValueError("a digit is three bits")
    return sum((1 if d & 4 else -1) * ((d & 3) + 1) << (4 * i) for i, d in enumerate(digits))


def shuffle(remark_key: b.RemarkKey, masked_cards: Sequence[Tuple[Point, Point]], digits: Sequence[Sequence[int]], perm: Sequence[int] = None,
            want_trace: bool = False):
    """One player's shuffle: every card remasked by its 84 digits, then out[i] = remasked[perm[i]].  Returns the new deck, and with
    want_trace also the traces in INPUT card order: per card 84 entries (c2.x, c2.y, c1.x, c1.y), the intermediate values of
    eval_remark_with_trace.  digits and perm come from the caller."""
    if len(digits) != len(masked_cards):
        raise ValueError("84 digits per card")
    e1, e2, tr = remark_key.remark_batch(points_to_wire([c[0] for c in masked_cards]), points_to_wire([c[1] for c in masked_cards]),
                                         np.asarray(digits, dtype=np.uint8), perm, want_trace)
    deck = list(zip(points_from_wire(e1), points_from_wire(e2)))
    if not want_trace:
        return deck
    flat = points_from_wire(tr)                                       # (c2.x, c2.y), (c1.x, c1.y) alternating
    per = N.REMARK_ITERATIONS
    return deck, [[flat[2 * (k * per + i)] + flat[2 * (k * per + i) + 1] for i in range(per)] for k in range(len(masked_cards))]
