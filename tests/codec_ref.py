"""The point codec on Python integers: ark-serialize's compressed G1, G2 and Baby Jubjub points in both directions, with the strictness
rules of include/uzkge_gpu.h ("the point codec").  Decoders return (status, point): 0 accepted (point None = infinity for G1 / G2),
1 not a canonical encoding, 2 no point, 3 outside the prime-order subgroup (only when asked; never for G1).  Encoders return the bytes.

G1 points are (x, y), G2 points ((x0, x1), (y0, y1)), Baby Jubjub points (x, y); integers below the modulus."""
import json
import os

import ed_ref
import g2_ref
from g2_ref import P, R

Q = ed_ref.Q
OK, NOT_CANONICAL, NO_POINT, NOT_IN_SUBGROUP = 0, 1, 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
CARD_MAPS_JSON = os.path.join(HERE, "golden", "card_maps_golden.json")
CARD_MAPS_SHA256 = "9dadf3a765935dc07dd65813ec4f5b6eb34944596378117fdd0221e0e7e3b03e"
KEY_PARTS = ("groth16-reveal-head.bin", "groth16-reveal-b-queries.bin", "groth16-reveal-tail.bin")
SECTIONS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
G2_SECTIONS = ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query")


def _flags(b):
    """(infinity bit, sign bit, the integer under the two flag bits) of an encoding's last 32 bytes"""
    v = int.from_bytes(b[-32:], "little")
    return bool(v >> 254 & 1), bool(v >> 255), v & ((1 << 254) - 1)


def g1_decompress(b):
    assert len(b) == 32
    inf, sign, x = _flags(b)
    if inf:
        return (OK, None) if not sign and x == 0 else (NOT_CANONICAL, None)
    if x >= P:
        return NOT_CANONICAL, None
    y = g2_ref.fq_sqrt((x * x * x + 3) % P)
    if y is None:
        return NO_POINT, None
    if y == 0 and sign:
        return NOT_CANONICAL, None
    if (y > (-y) % P) != sign:
        y = (-y) % P
    return OK, (x, y)


def _g2_mul_is_inf(k, q):
    """[k] q = O by double-and-add over g2_ref's Jacobian arithmetic (None = infinity; a doubling of a point with y = 0 leaves z = 0)"""
    acc = None
    for bit in bin(k)[2:]:
        acc = g2_ref.jac_dbl(acc)
        if acc is not None and acc[2] == (0, 0):
            acc = None
        if bit == "1":
            acc = g2_ref.jac_madd(acc, q)
    return acc is None or acc[2] == (0, 0)


def g2_decompress(b, check_subgroup=False):
    assert len(b) == 64
    inf, sign, x1 = _flags(b)
    x0 = int.from_bytes(b[:32], "little")
    if inf:
        return (OK, None) if not sign and x0 == 0 and x1 == 0 else (NOT_CANONICAL, None)
    if x0 >= P or x1 >= P:
        return NOT_CANONICAL, None
    x = (x0, x1)
    y = g2_ref.f2_sqrt(g2_ref.f2_add(g2_ref.f2_mul(g2_ref.f2_sqr(x), x), g2_ref.B2))
    if y is None:
        return NO_POINT, None
    if y == (0, 0) and sign:
        return NOT_CANONICAL, None
    if g2_ref.f2_gt(y, g2_ref.f2_neg(y)) != sign:
        y = g2_ref.f2_neg(y)
    if check_subgroup and not _g2_mul_is_inf(R, (x, y)):
        return NOT_IN_SUBGROUP, None
    return OK, (x, y)


def ed_decompress(b, check_subgroup=False):
    assert len(b) == 32
    v = int.from_bytes(b, "little")
    sign, y = bool(v >> 255), v & ((1 << 255) - 1)
    if y >= Q:
        return NOT_CANONICAL, None
    x = ed_ref._sqrt((1 - y * y) * pow(1 - ed_ref.D * y * y, -1, Q) % Q)
    if x is None:
        return NO_POINT, None
    if x == 0 and sign:
        return NOT_CANONICAL, None
    if (x > (-x) % Q) != sign:
        x = (-x) % Q
    if check_subgroup and ed_ref.classify((x, y)) != ed_ref.OK:
        return NOT_IN_SUBGROUP, None
    return OK, (x, y)


def g1_compress(p):
    if p is None:
        return (1 << 254).to_bytes(32, "little")
    x, y = p
    return (x | (int(y > (-y) % P) << 255)).to_bytes(32, "little")


def g2_compress(q):
    if q is None:
        return bytes(32) + (1 << 254).to_bytes(32, "little")
    x, y = q
    return x[0].to_bytes(32, "little") + (x[1] | (int(g2_ref.f2_gt(y, g2_ref.f2_neg(y))) << 255)).to_bytes(32, "little")


def ed_compress(p):
    x, y = p
    return (y | (int(x > (-x) % Q) << 255)).to_bytes(32, "little")


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------
def key_bytes():
    """the reference's groth16_pk.bin, 1 041 488 bytes, from its three parts under tests/golden"""
    return b"".join(open(os.path.join(HERE, "golden", name), "rb").read() for name in KEY_PARTS)


def key_layout(data):
    """section -> (offset, count) by the walk of RevealCircuit.parse_key_bytes: the host test compares uzk_g16_pk_layout with it"""
    out, pos = {}, 0
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1", "a_query", "b_g1_query", "b_g2_query", "h_query",
                 "l_query"):
        width = 64 if name in G2_SECTIONS else 32
        count = 1
        if name == "gamma_abc_g1" or name.endswith("_query"):
            count = int.from_bytes(data[pos:pos + 8], "little")
            pos += 8
        out[name] = (pos, count)
        pos += width * count
    assert pos == len(data)
    return out


def section_encodings(data, layout, name):
    off, count = layout[name][:2]
    width = 64 if name in G2_SECTIONS else 32
    return [data[off + width * i:off + width * (i + 1)] for i in range(count)]


def card_ys():
    return [int(y, 16) for y in json.load(open(CARD_MAPS_JSON))["y"]]


def g2_outside_subgroup():
    """a point of the twist that [r] does not kill: the twist has r (2 p - r) points, so almost every point of it is one"""
    x0 = 1
    while True:
        x0 += 1
        x = (x0, 1)
        y = g2_ref.f2_sqrt(g2_ref.f2_add(g2_ref.f2_mul(g2_ref.f2_sqr(x), x), g2_ref.B2))
        if y is not None and not _g2_mul_is_inf(R, (x, y)):
            return (x, y)
