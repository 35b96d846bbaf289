"""CPU restatement, on Python integers, of the Baby Jubjub layer of include/uzkge_gpu.h (uzk_ed_* / uzk_cp_reveal_*): the twisted
Edwards curve over BN254's scalar field that zshuffle's cards live on (ark_ed_on_bn254), point classification, the Chaum-Pedersen
DL proof of a reveal (shuffle/src/reveal.rs, uzkge/src/chaum_pedersen/dl.rs) with its Keccak transcript, unmask and key aggregation.

  curve      x^2 + y^2 = 1 + d x^2 y^2 over F_q (q = BN254's r), a = 1, d = 168696 / 168700: d is a non-square, the unified addition
             law is complete.  Identity (0, 1), cofactor 8, prime subgroup order L (251 bits)
  classify   0 ok; 1 a coordinate >= q; 2 off the curve; 3 [L] P != identity          (the first that applies)
  transcript keccak256(pad32("Revealing") | pad32("DL") | x, y of e1, G, reveal, pk, a, b as 32-byte big-endian words): 448 bytes;
             c = the digest as a big-endian integer mod L
  proof      160 bytes, big-endian a.x a.y b.x b.y r (ChaumPedersenDLProof::to_uncompress)
  verify     0 accepted; 1 .. 3 as classify over the statement's and the proof's points; 4 r e1 != a + c reveal; 5 r G != b + c pk

Points are affine integer pairs; arithmetic runs on projective triples (X, Y, Z) so that a multiplication costs no inversion per step."""
import hashlib
import json
import os
import random

import numpy as np

from plonk_golden_verifier import keccak256

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
D = 168696 * pow(168700, -1, Q) % Q
G = (0x2B8CFD91B905CAE31D41E7DEDF4A927EE3BC429AAD7E344D59D2810D82876C32, 0x2AAA6C24A758209E90ACED1F10277B762A7C1115DBC0E16AC276FC2C671A861F)
IDENTITY = (0, 1)
ORDER2 = (0, Q - 1)
ORDER4 = ((1, 0), (Q - 1, 0))
PROOF_BYTES = 160
OK, NOT_CANONICAL, OFF_CURVE, NOT_IN_SUBGROUP, EQ1_FAILS, EQ2_FAILS = 0, 1, 2, 3, 4, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_JSON = os.path.join(GOLDEN, "chaum_pedersen_reveal_golden.json")
GOLDEN_SHA256 = "53127311d60ee71ce7a9fc3c876e93a4d6de6e38e0885853e27e6fb5c803921d"
R_MONT = (1 << 256) % Q


# ---- the group law --------------------------------------------------------------------------------------------------------------
def padd(p, q):
    """the unified projective addition (add-2008-bbjlp with a = 1): complete, also the doubling"""
    x1, y1, z1 = p
    x2, y2, z2 = q
    a = z1 * z2 % Q
    b = a * a % Q
    c = x1 * x2 % Q
    d = y1 * y2 % Q
    e = D * c % Q * d % Q
    f = (b - e) % Q
    g = (b + e) % Q
    x3 = a * f % Q * ((x1 + y1) * (x2 + y2) - c - d) % Q
    y3 = a * g % Q * (d - c) % Q
    z3 = f * g % Q
    return (x3, y3, z3)


def proj(p):
    return (p[0] % Q, p[1] % Q, 1)


def affine(p):
    zi = pow(p[2], -1, Q)
    return (p[0] * zi % Q, p[1] * zi % Q)


def add(p, q):
    return affine(padd(proj(p), proj(q)))


def neg(p):
    return ((-p[0]) % Q, p[1] % Q)


def sub(p, q):
    return add(p, neg(q))


def pmul(k, p):
    """k P for any integer k >= 0 (not reduced), projective"""
    acc, base = (0, 1, 1), proj(p)
    for i in range(k.bit_length() - 1, -1, -1):
        acc = padd(acc, acc)
        if (k >> i) & 1:
            acc = padd(acc, base)
    return acc


def mul(k, p):
    return affine(pmul(k, p))


def psum(points):
    acc = (0, 1, 1)
    for p in points:
        acc = padd(acc, proj(p))
    return affine(acc)


# the textbook affine law with separate formulas, for the comparison with the unified one (tests only: an inversion per call)
def affine_add_distinct(p, q):
    x1, y1 = p
    x2, y2 = q
    t = D * x1 * x2 % Q * y1 % Q * y2 % Q
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, Q) % Q, (y1 * y2 - x1 * x2) * pow(1 - t, -1, Q) % Q)


def affine_double(p):
    """the dedicated doubling: 2 x y / (x^2 + y^2), (y^2 - x^2) / (2 - x^2 - y^2)  (the curve equation replaces d x^2 y^2)"""
    x, y = p
    s = (x * x + y * y) % Q
    return (2 * x * y * pow(s, -1, Q) % Q, (y * y - x * x) * pow(2 - s, -1, Q) % Q)


def on_curve(p):
    x, y = p
    return (x * x + y * y - 1 - D * x * x % Q * y * y) % Q == 0


def classify(p):
    x, y = p
    if x >= Q or y >= Q:
        return NOT_CANONICAL
    if not on_curve(p):
        return OFF_CURVE
    t = pmul(L, p)
    return OK if t[0] == 0 and t[1] == t[2] else NOT_IN_SUBGROUP


def order8_point():
    """a point of order exactly 8: [L] of a curve point outside every smaller subgroup"""
    x = 1
    while True:
        x += 1
        # y^2 = (1 - x^2) / (1 - d x^2)
        y2 = (1 - x * x) * pow(1 - D * x * x, -1, Q) % Q
        y = _sqrt(y2)
        if y is None:
            continue
        t = mul(L, (x, y))
        if mul(4, t) != IDENTITY:
            return t


def _sqrt(a):
    """Tonelli-Shanks in F_q (q - 1 = 2^28 * odd)"""
    if a == 0:
        return 0
    if pow(a, (Q - 1) // 2, Q) != 1:
        return None
    s, t = 0, Q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 5
    while pow(z, (Q - 1) // 2, Q) == 1:
        z += 1
    m, c, u, r = s, pow(z, t, Q), pow(a, t, Q), pow(a, (t + 1) // 2, Q)
    while u != 1:
        i, v = 0, u
        while v != 1:
            v, i = v * v % Q, i + 1
        b = pow(c, 1 << (m - i - 1), Q)
        m, c, u, r = i, b * b % Q, u * b * b % Q, r * b % Q
    return r


def rand_subgroup_points(n, seed):
    rng = random.Random(seed)
    return [mul(rng.randrange(1, L), G) for _ in range(n)]


# ---- the transcript and the proof -------------------------------------------------------------------------------------------------
def _pad32(msg):
    return bytes(32 - len(msg)) + msg


def _w(v):
    return int(v).to_bytes(32, "big")


def transcript_bytes(e1, reveal, pk, a, b):
    out = _pad32(b"Revealing") + _pad32(b"DL")
    for p in (e1, G, reveal, pk, a, b):
        out += _w(p[0]) + _w(p[1])
    assert len(out) == 448
    return out


def reduce_digest(v):
    """a 256-bit integer mod L (floor(2^256 / L) = 42)"""
    return v % L


def challenge(e1, reveal, pk, a, b):
    return reduce_digest(int.from_bytes(keccak256(transcript_bytes(e1, reveal, pk, a, b)), "big"))


def make_proof(a, b, r):
    return _w(a[0]) + _w(a[1]) + _w(b[0]) + _w(b[1]) + _w(r)


def parse_proof(blob):
    assert len(blob) == PROOF_BYTES
    w = [int.from_bytes(blob[32 * k:32 * k + 32], "big") for k in range(5)]
    return (w[0], w[1]), (w[2], w[3]), w[4]


def keypair_public(sk):
    return mul(sk, G)


def prove(sk, e1, omega):
    """(reveal card, proof blob) of one masked card's e1 under the secret sk with the caller's draw omega"""
    reveal, pk = mul(sk, e1), mul(sk, G)
    a, b = mul(omega, e1), mul(omega, G)
    c = challenge(e1, reveal, pk, a, b)
    return reveal, make_proof(a, b, (omega + c * sk) % L)


def verify(statement, blob, want_challenge=False):
    """statement = (e1.x, e1.y, reveal.x, reveal.y, pk.x, pk.y): the verdict byte (and the challenge, where one is defined)"""
    a, b, r = parse_proof(blob)
    e1, reveal, pk = (statement[0], statement[1]), (statement[2], statement[3]), (statement[4], statement[5])
    pts = (e1, reveal, pk, a, b)
    # the first rule that applies over ALL points: a coordinate >= q anywhere comes before a point off the curve elsewhere
    if any(v >= Q for p in pts for v in p):
        st = NOT_CANONICAL
    elif not all(on_curve(p) for p in pts):
        st = OFF_CURVE
    else:
        st = max(classify(p) for p in pts)                        # 0 or 3
    c = None
    if st == OK:
        c = challenge(e1, reveal, pk, a, b)
        if not peq(pmul(r, e1), padd(proj(a), pmul(c, reveal))):
            st = EQ1_FAILS
        elif not peq(pmul(r, G), padd(proj(b), pmul(c, pk))):
            st = EQ2_FAILS
    return (st, c) if want_challenge else st


def peq(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % Q == 0 and (p[1] * q[2] - q[1] * p[2]) % Q == 0


def unmask(e2, reveals):
    return sub(e2, psum(reveals))


def aggregate_keys(pks):
    return psum(pks)


# ---- the golden cases ----------------------------------------------------------------------------------------------------------
def sha256_of(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def golden():
    g = json.load(open(GOLDEN_JSON))
    ints = lambda xs: [int(v, 16) for v in xs]
    pt = lambda d: (int(d["x"], 16), int(d["y"], 16))
    agg, rev, unm = g["aggregate_keys"], g["reveal_verify"], g["unmask_verify"]
    return {
        "keys": [pt(k) for k in agg["keys"]], "keys_sum": pt(agg["sum"]),
        "pk": pt(rev["pk"]), "masked": ints(rev["masked"]), "reveal": pt(rev["reveal"]), "proof": bytes.fromhex(rev["proof"]),
        "unmask_masked": ints(unm["masked"]), "unmask_reveals": [pt(k) for k in unm["reveals"]], "unmask_y": int(unm["y"], 16),
    }


def golden_statement(g=None):
    """the golden reveal case as a statement: a masked card is e2.x, e2.y, e1.x, e1.y"""
    g = g or golden()
    m = g["masked"]
    return (m[2], m[3], g["reveal"][0], g["reveal"][1], g["pk"][0], g["pk"][1])


# ---- the wire -------------------------------------------------------------------------------------------------------------------
def fr_wire(vals):
    """integers below q -> n x 4 uint64 Montgomery words (the element encoding of every Fr argument of the C ABI)"""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = int(v) % Q * R_MONT % Q
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def fr_unwire(a):
    inv = pow(R_MONT, -1, Q)
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(a[i, k]) << (64 * k) for k in range(4)) * inv % Q for i in range(a.shape[0])]


def raw_wire(vals):
    """integers below 2^256 taken as they are -> n x 4 uint64 words (what a non-canonical element looks like on the wire)"""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def points_wire(points):
    """n points -> n x 8 words, x then y"""
    return fr_wire([c for p in points for c in p]).reshape(len(points), 8)


def points_unwire(a):
    v = fr_unwire(np.asarray(a).reshape(-1, 4))
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def scalars_wire(ks):
    """256-bit integers, little-endian 64-bit words, NOT Montgomery"""
    return raw_wire(ks)
