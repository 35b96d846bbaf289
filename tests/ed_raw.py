"""Host side of uzk_test_ed_raw_kat (include/uzkge_gpu_test.h), Python integers only: raw limb representatives of the coordinates of a
Baby Jubjub point in the form ed29.hpp keeps them in, the extended-coordinate law of ed29.hpp restated on residues, and the way back
from raw output limbs to residues and to the affine point (held to ed_ref.add by tests/test_ed_raw_host.py).

A coordinate with residue c in the 2^261-form is ANY limb vector of value c 2^261 mod Q + k Q; ed::C = Lz<Fr29, 1, 2> takes k = 0, 1.
The limb shapes are those lz29_contract.gen_type has for K = 1: the normalized digits, and the carry-step restatement of the same value
(g2_raw.carry_step).  A given value has the second shape only where a digit is below 2^6, so the tests also build points AROUND limbs:
any nonzero Z residue carries a point (X = x Z, Y = y Z, T = x y Z), and any X limb vector carries one with Z = X / x, so gen_type's
extreme vectors and shaped()'s carry-step vectors sit in a coordinate as they are."""
import numpy as np

import ed_ref as er
import lz29_contract as lc
from g2_raw import carry_step
from lz29_contract import B, limbs, value

Q = er.Q
FORM = 261
C = (1, 2)                                  # (K, V) of ed::C
PT_WORDS, REC_WORDS, OUT_WORDS = 36, 72, 37
MONT = (1 << 256) % Q
OPS = dict(add=0, neg=1, is_identity=2, eq_affine=3, on_curve=4, to_affine=5, inv=6)


# ---- representatives ----------------------------------------------------------------------------------------------------------------
def rep_value(c, k):
    return c * pow(2, FORM, Q) % Q + k * Q


def residue(l):
    return value(l) * pow(2, -FORM, Q) % Q


def rep_limbs(c, k, slack=False):
    l = limbs(rep_value(c, k))
    return carry_step(l) if slack else l


def shaped(rng):
    """A limb vector of ed::C drawn limb by limb: every low limb either a plain digit or, with probability 1 / 2, in the carry-step
    range [2^29, 2^29 + 2^6); the top limb anywhere the value bound allows.  Its residue is whatever it is."""
    low = [int(B + rng.integers(0, 64)) if rng.integers(0, 2) else int(rng.integers(0, B)) for _ in range(8)]
    top_max = (C[1] * Q - 1 - value(low + [0])) >> 232
    l = low + [int(rng.integers(0, top_max + 1))]
    assert lc.in_type(l, *C, Q)
    return l


def extreme_vectors(rng):
    """gen_type's extreme vectors of ed::C: (a) every low limb at 2^29 + 2^6 - 1 with the largest top limb, (b) the top limb alone,
    (c) 2 M - 1"""
    return lc.gen_type(*C, Q, rng, n_random=0)[:3]


# ---- the extended law on residues (ed29.hpp; a point is (X, Y, Z, T)) ---------------------------------------------------------------------
def ext_of(pt, z=1):
    """an affine point under the representative z: (x z, y z, z, x y z)"""
    x, y = pt
    return (x * z % Q, y * z % Q, z % Q, x * y % Q * z % Q)


def ext_affine(p):
    zi = pow(p[2], -1, Q)
    return (p[0] * zi % Q, p[1] * zi % Q)


def ext_consistent(p):
    """T Z = X Y: what the next addition's C = d T1 T2 relies on"""
    return (p[3] * p[2] - p[0] * p[1]) % Q == 0


def ext_add(p, q):
    """the unified addition of ed29.hpp: X3 = E F, Y3 = G H, T3 = E H, Z3 = F G"""
    a = p[0] * q[0] % Q
    b = p[1] * q[1] % Q
    c = er.D * p[3] % Q * q[3] % Q
    d = p[2] * q[2] % Q
    e = ((p[0] + p[1]) * (q[0] + q[1]) - a - b) % Q
    f, g, h = (d - c) % Q, (d + c) % Q, (b - a) % Q
    return (e * f % Q, g * h % Q, f * g % Q, e * h % Q)


def ext_neg(p):
    return ((-p[0]) % Q, p[1], p[2], (-p[3]) % Q)


def around_z(pt, zl):
    """(the point's residues, override) with the limb vector zl as its Z, as it is (its residue must not be 0)"""
    z = residue(zl)
    assert z != 0
    return ext_of(pt, z), {2: list(zl)}


def around_x(pt, xl):
    """the same with xl as X: Z = X / x (x and the residue of xl must not be 0)"""
    xr = residue(xl)
    assert pt[0] != 0 and xr != 0
    p = ext_of(pt, xr * pow(pt[0], -1, Q) % Q)
    assert p[0] == xr
    return p, {0: list(xl)}


# ---- raw records -------------------------------------------------------------------------------------------------------------------
def raw_point(p, ks=0, slack=False, override=None):
    """36 words of a point given by residues (X, Y, Z, T): coordinate i is representative ks[i] (an int: the same everywhere), normalized
    or carry-step; override = {i: limbs} puts a limb vector in as it is (its residue must be the coordinate's)"""
    ks = [ks] * 4 if isinstance(ks, int) else list(ks)
    sl = [slack] * 4 if isinstance(slack, bool) else list(slack)
    out = np.zeros(PT_WORDS, dtype=np.uint32)
    for i in range(4):
        l = (override or {}).get(i)
        if l is None:
            l = rep_limbs(p[i], ks[i], sl[i])
        else:
            assert residue(l) == p[i]
        out[9 * i:9 * i + 9] = l
    return out


def record(a, b=None):
    r = np.zeros(REC_WORDS, dtype=np.uint32)
    r[0:PT_WORDS] = a
    if b is not None:
        r[PT_WORDS:] = b
    return r


def coords(row):
    return [[int(v) for v in row[9 * t:9 * t + 9]] for t in range(4)]


def residues(row):
    return tuple(residue(l) for l in coords(row))


def check_types(row, what="", count=4):
    for t, l in enumerate(coords(row)[:count]):
        lc.check_type(l, *C, Q, what=f"{what} coordinate {t}")


def check_point(row, want, what=""):
    """a raw output point: every coordinate inside ed::C AND exactly the residues of the restated law"""
    check_types(row, what)
    got = residues(row)
    assert got == tuple(want), f"{what}: residues differ from the reference in coordinates {[i for i in range(4) if got[i] != want[i]]}"


def check_coord(l, want, what=""):
    lc.check_type(l, *C, Q, what=what)
    assert residue(l) == want, f"{what}: residue differs from the reference"


def _words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def wire_affine(pt):
    """what op 5 returns for the affine point: the canonical Montgomery (2^256) words of x and y, eight each and the ninth 0; z, t and
    the flag zero"""
    out = np.zeros(OUT_WORDS, dtype=np.uint32)
    out[0:8] = _words(pt[0] * MONT % Q)
    out[9:17] = _words(pt[1] * MONT % Q)
    return out
