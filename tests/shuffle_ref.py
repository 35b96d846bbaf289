"""CPU restatement, on Python integers, of the two steps of a zshuffle game that sit on Baby Jubjub beside the reveal path of
tests/ed_ref.py: masking a card with its Chaum-Pedersen "Masking" proof (shuffle/src/mask.rs) and the remask of a shuffle with its
trace (uzkge/src/shuffle/remark.rs: crate_generators / crate_public_keys, eval_remark, eval_remark_with_trace).

  tables     T_P[i][j] = (j + 1) 16^i P for i < 84, j < 4, built as the reference builds them: a segment by three additions, then four
             doublings to the next i (4 16^83 has 335 bits: no 256-bit scalar multiplication produces the entries).  The unified law
             makes the definition hold on the whole curve.  An entry is (x, y, d x y)
  digit      one byte per (card, iteration): bit 0 = bits[0], bit 1 = bits[1], bit 2 = bits[2]; j = bit0 + 2 bit1; bit 2 set adds
             T[i][j], clear adds -T[i][j]; bits 3 .. 7 must be zero
  step i     c1 += +-T_G[i][j], c2 += +-T_pk[i][j]; trace entry i = [c2.x, c2.y, c1.x, c1.y] in affine (the identity is (0, 1)); the
             remasked card is entry 83
  rho        sum_i +-(j_i + 1) 16^i, up to 336 bits: remask = (e1 + rho G, e2 + rho pk)
  shuffle    out[i] = remasked[perm[i]] (the row convention of Permutation: matrix[i][perm[i]] = 1)
  mask       e1 = r G, e2 = card + r pk; transcript keccak256(pad32("Masking") | pad32("DL") | G, pk, e1, e2 - card, a, b): 448 bytes;
             a = omega G, b = omega pk, c = digest mod L, r' = omega + c r mod L; the blob is ed_ref's 160 bytes
  verify     0 accepted; 1 .. 3 as classify over pk, card, e1, e2, a, b; 4 r' G != a + c e1; 5 r' pk != b + c (e2 - card)"""
import json
import os

import numpy as np

import ed_ref as e
from plonk_golden_verifier import keccak256

Q, L, D, G = e.Q, e.L, e.D, e.G
ITERATIONS = 84
TABLES_JSON = os.path.join(e.GOLDEN, "remark_tables_golden.json")
TABLES_SHA256 = "d79030a9b14b15adc8c9b99ea34776b750ef2db1f30cf83389a4dd89be1bb6ad"


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def tables_projective(p):
    out, g = [], e.proj(p)
    for _ in range(ITERATIONS):
        seg, row = g, []
        for _ in range(4):
            row.append(seg)
            seg = e.padd(seg, g)
        for _ in range(4):
            g = e.padd(g, g)
        out.append(row)
    return out


def tables(p):
    """[84][4] affine points"""
    return [[e.affine(t) for t in row] for row in tables_projective(p)]


def entry(pt):
    """what the circuit stores of a table point: x, y, d x y"""
    return (pt[0], pt[1], D * pt[0] % Q * pt[1] % Q)


def table_entries(p):
    return [[entry(t) for t in row] for row in tables(p)]


_GEN = None


def generator_tables():
    global _GEN
    if _GEN is None:
        _GEN = tables(G)
    return _GEN


# ---- digits -----------------------------------------------------------------------------------------------------------------------
def digit_of_bits(bits):
    return int(bits[0]) | int(bits[1]) << 1 | int(bits[2]) << 2


def signed_digit(d):
    """the multiple of 16^i a digit adds: +-(j + 1)"""
    if not 0 <= d <= 7:
        raise ValueError("a digit is three bits")
    return (1 if d & 4 else -1) * ((d & 3) + 1)


def digit_for(j, positive):
    return j | (4 if positive else 0)


def remark_scalar(digits):
    assert len(digits) == ITERATIONS
    return sum(signed_digit(d) << (4 * i) for i, d in enumerate(digits))


# ---- the remask -------------------------------------------------------------------------------------------------------------------
def eval_remark_with_trace(card, digits, t_pk, t_gen=None):
    """card = (e1, e2); t_pk / t_gen: tables().  Returns the 84 trace entries [c2.x, c2.y, c1.x, c1.y]."""
    t_gen = t_gen or generator_tables()
    assert len(digits) == ITERATIONS
    c1, c2 = e.proj(card[0]), e.proj(card[1])
    trace = []
    for i, d in enumerate(digits):
        s, j = signed_digit(d), d & 3
        tg, tp = t_gen[i][j], t_pk[i][j]
        c1 = e.padd(c1, e.proj(tg if s > 0 else e.neg(tg)))
        c2 = e.padd(c2, e.proj(tp if s > 0 else e.neg(tp)))
        a1, a2 = e.affine(c1), e.affine(c2)
        trace.append((a2[0], a2[1], a1[0], a1[1]))
    return trace


def eval_remark(card, digits, t_pk, t_gen=None):
    last = eval_remark_with_trace(card, digits, t_pk, t_gen)[-1]
    return ((last[2], last[3]), (last[0], last[1]))


def signed_mul(k, p):
    """k P for any integer k, on the whole curve"""
    return e.mul(k, p) if k >= 0 else e.neg(e.mul(-k, p))


def remark_by_scalar(card, digits, pk):
    rho = remark_scalar(digits)
    return (e.add(card[0], signed_mul(rho, G)), e.add(card[1], signed_mul(rho, pk)))


def shuffle(cards, digits, perm, t_pk):
    """(the deck in output order, the traces in input order)"""
    traces = [eval_remark_with_trace(c, d, t_pk) for c, d in zip(cards, digits)]
    remasked = [((t[-1][2], t[-1][3]), (t[-1][0], t[-1][1])) for t in traces]
    perm = list(range(len(cards))) if perm is None else perm
    assert sorted(perm) == list(range(len(cards)))
    return [remasked[perm[i]] for i in range(len(cards))], traces


# ---- the mask ---------------------------------------------------------------------------------------------------------------------
def mask_transcript_bytes(pk, e1, diff, a, b):
    out = e._pad32(b"Masking") + e._pad32(b"DL")
    for p in (G, pk, e1, diff, a, b):
        out += e._w(p[0]) + e._w(p[1])
    assert len(out) == 448
    return out


def mask_challenge(pk, e1, diff, a, b):
    return e.reduce_digest(int.from_bytes(keccak256(mask_transcript_bytes(pk, e1, diff, a, b)), "big"))


def mask(pk, card, r, omega):
    """((e1, e2), proof blob) for the caller's draws r and omega"""
    e1, rpk = e.mul(r, G), e.mul(r, pk)
    e2 = e.add(card, rpk)
    a, b = e.mul(omega, G), e.mul(omega, pk)
    c = mask_challenge(pk, e1, e.sub(e2, card), a, b)
    return (e1, e2), e.make_proof(a, b, (omega + c * r) % L)


def verify_mask(pk, card, masked, blob, want_challenge=False):
    a, b, r = e.parse_proof(blob)
    e1, e2 = masked
    pts = (pk, card, e1, e2, a, b)
    if any(v >= Q for p in pts for v in p):
        st = e.NOT_CANONICAL
    elif not all(e.on_curve(p) for p in pts):
        st = e.OFF_CURVE
    else:
        st = max(e.classify(p) for p in pts)
    c = None
    if st == e.OK:
        diff = e.sub(e2, card)
        c = mask_challenge(pk, e1, diff, a, b)
        if not e.peq(e.pmul(r, G), e.padd(e.proj(a), e.pmul(c, e1))):
            st = e.EQ1_FAILS
        elif not e.peq(e.pmul(r, pk), e.padd(e.proj(b), e.pmul(c, diff))):
            st = e.EQ2_FAILS
    return (st, c) if want_challenge else st


# ---- the fixture and the wire -----------------------------------------------------------------------------------------------------
def golden_tables():
    """{(i, j): (x, y, dxy)} of the reference's preprocessed generator entries"""
    g = json.load(open(TABLES_JSON))
    return {(int(t["i"]), int(t["j"])): (int(t["x"]), int(t["y"]), int(t["dxy"])) for t in g["generators"]}


def tables_unwire(a):
    """[84, 4, 3, 4] words -> [84][4] of (x, y, dxy)"""
    v = e.fr_unwire(np.asarray(a, dtype=np.uint64).reshape(-1, 4))
    return [[tuple(v[(4 * i + j) * 3:(4 * i + j) * 3 + 3]) for j in range(4)] for i in range(ITERATIONS)]


def trace_unwire(a, n):
    """[n, 84, 4, 4] words -> [n][84] of (c2.x, c2.y, c1.x, c1.y)"""
    v = e.fr_unwire(np.asarray(a, dtype=np.uint64).reshape(-1, 4))
    return [[tuple(v[(k * ITERATIONS + i) * 4:(k * ITERATIONS + i) * 4 + 4]) for i in range(ITERATIONS)] for k in range(n)]
