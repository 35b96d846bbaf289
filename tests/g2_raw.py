"""Host side of uzk_test_g2_raw_kat (include/uzkge_gpu_test.h), Python integers only: raw limb representatives of the coordinates of a
G2 point in the forms g2_29.hpp keeps them in, the XYZZ formulas of g2_29.hpp restated on residues, and the way back from raw output
limbs to residues and to the affine point (held to oracle/bn254_pairing.py's g2_add by tests/test_g2_raw_host.py).

A coordinate is an Fq2 element (c0, c1); a component with residue c in the 2^f-form is ANY limb vector of value c 2^f + k M.  The
types bound k: X, Y of the accumulator and all four coordinates of a full point (g2::CoA = E2<1, 16>, 2^261-form) take k = 0 .. 15,
ZZ and ZZZ of the accumulator (g2::CoZ = E2<1, 2>, 2^266-form) k = 0 .. 1.  The limb shapes are those lz29_contract.gen_type has for
K = 1: the normalized digits, and the carry-step restatement of the same value (a low limb in [2^29, 2^29 + 2^6), one borrowed from
the limb above).  A given value has the second shape only where a digit is below 2^6, so the tests also build points AROUND shaped
limbs: ZZ is taken from gen_type's extreme vectors as they are and the rest of the point follows from its square root."""
import numpy as np

import g2_ref as g
import lz29_contract as lc
from lz29_contract import B, limbs, value

P = g.P
PT_WORDS, REC_WORDS = 73, 147
F261, F266 = 261, 266
FORMS_P = (F261, F261, F261, F261)          # G2P: x, y, zz, zzz
FORMS_ACC = (F261, F261, F266, F266)        # G2Acc
KMAX_P = (15, 15, 15, 15)
KMAX_ACC = (15, 15, 1, 1)
TYPES_P = ((1, 16),) * 4                    # what lc.check_type holds each output coordinate to
TYPES_ACC = ((1, 16), (1, 16), (1, 2), (1, 2))


# ---- representatives ----------------------------------------------------------------------------------------------------------------
def rep_value(c, form, k):
    """the value of the k-th representative of residue c in the 2^form-form"""
    return c * pow(2, form, P) % P + k * P


def residue(l, form):
    return value(l) * pow(2, -form, P) % P


def carry_step(l):
    """The same value with every low limb that allows it raised by 2^29 (one borrowed from the limb above): low limbs stay below
    2^29 + 2^6, the K = 1 bound.  Identity where no digit is below 2^6."""
    l = list(l)
    for i in range(8):
        if l[i] < 64 and l[i + 1] >= 1:
            l[i] += B
            l[i + 1] -= 1
    return l


def rep_limbs(c, form, k, slack=False):
    l = limbs(rep_value(c, form, k))
    return carry_step(l) if slack else l


# ---- XYZZ on residues (the formulas of g2_29.hpp; a point is (X, Y, ZZ, ZZZ) of Fq2 tuples, None = infinity) ---------------------------
def xyzz_of(pt, z=(1, 0)):
    """an affine point under the representative z: (x z^2, y z^3, z^2, z^3)"""
    if pt is None:
        return None
    zz = g.f2_sqr(z)
    zzz = g.f2_mul(zz, z)
    return (g.f2_mul(pt[0], zz), g.f2_mul(pt[1], zzz), zz, zzz)


def xyzz_affine(p):
    if p is None or p[2] == (0, 0):
        return None
    return (g.f2_mul(p[0], g.f2_inv(p[2])), g.f2_mul(p[1], g.f2_inv(p[3])))


def xyzz_consistent(p):
    """ZZ^3 = ZZZ^2: what the next addition's U, S products rely on"""
    return p is None or g.f2_mul(g.f2_sqr(p[2]), p[2]) == g.f2_sqr(p[3])


def xyzz_dbl(p):
    """dbl-2008-s-1 (g2p_dbl)"""
    if p is None:
        return None
    X, Y, ZZ, ZZZ = p
    U = g.f2_add(Y, Y)
    V = g.f2_sqr(U)
    W = g.f2_mul(U, V)
    S = g.f2_mul(X, V)
    X2 = g.f2_sqr(X)
    M3 = g.f2_add(g.f2_add(X2, X2), X2)
    X3 = g.f2_sub(g.f2_sqr(M3), g.f2_add(S, S))
    Y3 = g.f2_sub(g.f2_mul(M3, g.f2_sub(S, X3)), g.f2_mul(W, Y))
    return (X3, Y3, g.f2_mul(V, ZZ), g.f2_mul(W, ZZZ))


def xyzz_add(a, b):
    """add-2008-s, complete (g2p_add)"""
    if b is None:
        return a
    if a is None:
        return b
    U1, U2 = g.f2_mul(a[0], b[2]), g.f2_mul(b[0], a[2])
    S1, S2 = g.f2_mul(a[1], b[3]), g.f2_mul(b[1], a[3])
    Pd, Rd = g.f2_sub(U2, U1), g.f2_sub(S2, S1)
    if Pd == (0, 0):
        return xyzz_dbl(a) if Rd == (0, 0) else None
    PP = g.f2_sqr(Pd)
    PPP, Q = g.f2_mul(Pd, PP), g.f2_mul(U1, PP)
    X3 = g.f2_sub(g.f2_sqr(Rd), g.f2_add(PPP, g.f2_add(Q, Q)))
    Y3 = g.f2_sub(g.f2_mul(Rd, g.f2_sub(Q, X3)), g.f2_mul(S1, PPP))
    return (X3, Y3, g.f2_mul(g.f2_mul(a[2], b[2]), PP), g.f2_mul(g.f2_mul(a[3], b[3]), PPP))


def xyzz_madd(a, q, negate=False):
    """madd-2008-s, complete (g2acc_madd): accumulator a, affine q (None = infinity); the doubling branch restarts from 2 q"""
    if q is None:
        return a
    if negate:
        q = g.g2_neg(q)
    if a is None:
        return (q[0], q[1], (1, 0), (1, 0))
    return xyzz_dbl(xyzz_of(q)) if _same(a, q) else xyzz_add(a, xyzz_of(q))


def _same(a, q):
    return g.f2_mul(q[0], a[2]) == a[0] and g.f2_mul(q[1], a[3]) == a[1]


# ---- raw records -------------------------------------------------------------------------------------------------------------------
def raw_point(p, forms=FORMS_P, ks=0, slack=False, override=None):
    """73 words of a point given by residues (X, Y, ZZ, ZZZ) or None: component j of coordinate i is representative ks[2 i + j] (an
    int: the same everywhere) in forms[i], normalized or carry-step; override = {(i, j): limbs} puts limb vectors in as they are."""
    out = np.zeros(PT_WORDS, dtype=np.uint32)
    if p is None:
        out[72] = 1
        return out
    ks = [ks] * 8 if isinstance(ks, int) else list(ks)
    sl = [slack] * 8 if isinstance(slack, bool) else list(slack)
    for i in range(4):
        for j in range(2):
            l = (override or {}).get((i, j))
            if l is None:
                l = rep_limbs(p[i][j], forms[i], ks[2 * i + j], sl[2 * i + j])
            else:
                assert residue(l, forms[i]) == p[i][j]
            out[18 * i + 9 * j:18 * i + 9 * j + 9] = l
    return out


def _words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def wire_point(q):
    """73 words holding an affine point as g2acc_madd takes it: the canonical Montgomery (2^256) words of x and y, eight per
    component; infinity = zeros"""
    out = np.zeros(PT_WORDS, dtype=np.uint32)
    if q is not None:
        for i in range(2):
            for j in range(2):
                out[18 * i + 9 * j:18 * i + 9 * j + 8] = _words(q[i][j] * g.MONT % P)
    return out


def wire_words(p):
    """what op 3 returns for a point of residues: eight canonical words per component, the ninth 0; infinity = zeros, flag set"""
    out = np.zeros(PT_WORDS, dtype=np.uint32)
    if p is None:
        out[72] = 1
        return out
    for i in range(4):
        for j in range(2):
            out[18 * i + 9 * j:18 * i + 9 * j + 8] = _words(p[i][j] * g.MONT % P)
    return out


def record(a, b=None, flag=0):
    r = np.zeros(REC_WORDS, dtype=np.uint32)
    r[0:73] = a
    if b is not None:
        r[73:146] = b
    r[146] = flag
    return r


def coords(row):
    """a 73-word point -> (eight limb lists: x.c0, x.c1, y.c0, ..., infinity flag)"""
    return [[int(v) for v in row[9 * t:9 * t + 9]] for t in range(8)], int(row[72])


def residues(row, forms=FORMS_P):
    """a raw 73-word point -> residues (X, Y, ZZ, ZZZ), None at infinity"""
    cs, inf = coords(row)
    if inf:
        return None
    return tuple((residue(cs[2 * i], forms[i]), residue(cs[2 * i + 1], forms[i])) for i in range(4))


def check_types(row, types, what=""):
    cs, inf = coords(row)
    for t, l in enumerate(cs):
        lc.check_type(l, *types[t // 2], P, what=f"{what} coordinate {t // 2} component {t % 2}")


def shaped_zz(rng, acc=False):
    """Points around shaped limbs: (z, {(2, 0): limbs, (2, 1): limbs}) for every pair of gen_type's extreme vectors -- (a) all low limbs
    at 2^29 + 2^6 - 1 with the largest top limb, (b) the top limb alone, (c) V M - 1 -- of ZZ's type whose residue is a square in Fq2;
    z is its root, so that a point built on z carries exactly these limbs as its ZZ."""
    form, v = (F266, 2) if acc else (F261, 16)
    ext = lc.gen_type(1, v, P, rng, n_random=4)
    out = []
    for la in ext[:3] + ext[3:5]:
        for lb in ext[:3] + ext[5:7]:
            zz = (residue(la, form), residue(lb, form))
            z = g.f2_sqrt(zz)
            if z is not None and zz != (0, 0):
                out.append((z, {(2, 0): la, (2, 1): lb}))
    return out
