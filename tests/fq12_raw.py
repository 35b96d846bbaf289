"""Host side of uzk_test_fq12_raw_kat and uzk_test_miller_step_raw (include/uzkge_gpu_test.h), Python integers only: raw limb
representatives of the components of an Fq12 element and of the operands of a Miller step, the way back from raw output limbs to
residues, and the checks every raw output is held to.  Expected values are NOT restated here: they come from tests/pairing_ref.py (the
device's algorithm on integers) and oracle/bn254_pairing.py.

A coefficient of Fq12 is an Fq2 element (c0, c1); a component with residue c in the 2^261-form is ANY limb vector of value
c 2^261 mod P + k P.  The types bound k: q12::El = E2<1, 2> takes k = 0, 1; xP and -yP of a Miller step (Lz<Fq29, 1, 4>) k = 0 .. 3.
The limb shapes are those lz29_contract.gen_type has for K = 1: the normalized digits, and the carry-step restatement of the same value
(a low limb in [2^29, 2^29 + 2^6), one borrowed from the limb above; g2_raw.carry_step).  A given value has the second shape only where
a digit is below 2^6, so where an operation takes ANY residue the tests also go the other way: shaped() draws limb vectors with
carry-step limbs and the residue follows from them."""
import numpy as np

import lz29_contract as lc
import pairing_ref as pr
from g2_raw import carry_step
from lz29_contract import B, limbs, value

P = pr.P
FORM = 261
EL, BASE = (1, 2), (1, 4)                   # (K, V) of q12::El's members and of q12::Base
EL_WORDS, REC_WORDS = 108, 216              # an element; a record of uzk_test_fq12_raw_kat
STEP_IN_WORDS, STEP_OUT_WORDS = 108, 126    # uzk_test_miller_step_raw
MONT = (1 << 256) % P
OPS = dict(mul=0, sqr=1, sparse=2, conj=3, frob1=4, frob2=5, frob3=6, inv=7, cyc=8, easy=9, hard=10, xi_mul=11, to_wire=12)


# ---- representatives ----------------------------------------------------------------------------------------------------------------
def rep_value(c, k):
    """the value of the k-th representative of residue c"""
    return c * pow(2, FORM, P) % P + k * P


def residue(l):
    return value(l) * pow(2, -FORM, P) % P


def rep_limbs(c, k, slack=False):
    l = limbs(rep_value(c, k))
    return carry_step(l) if slack else l


def shaped(rng, v=2):
    """A limb vector of Lz<Fq29, 1, v> drawn limb by limb: every low limb either a plain digit or, with probability 1 / 2, in the
    carry-step range [2^29, 2^29 + 2^6); the top limb anywhere the value bound allows.  Its residue is whatever it is."""
    low = [int(B + rng.integers(0, 64)) if rng.integers(0, 2) else int(rng.integers(0, B)) for _ in range(8)]
    top_max = (v * P - 1 - value(low + [0])) >> 232
    l = low + [int(rng.integers(0, top_max + 1))]
    assert lc.in_type(l, 1, v, P)
    return l


def _list(x, n, kind):
    return [x] * n if isinstance(x, kind) else list(x)


# ---- Fq12 elements --------------------------------------------------------------------------------------------------------------------
def raw_f12(a, ks=0, slack=False, override=None):
    """108 words of an element given by residues (six Fq2 pairs): component j of coefficient i is representative ks[2 i + j] (an int: the
    same everywhere), normalized or carry-step; override = {(i, j): limbs} puts limb vectors in as they are (their residue must be a's)"""
    ks, sl = _list(ks, 12, int), _list(slack, 12, bool)
    out = np.zeros(EL_WORDS, dtype=np.uint32)
    for i in range(6):
        for j in range(2):
            l = (override or {}).get((i, j))
            if l is None:
                l = rep_limbs(a[i][j], ks[2 * i + j], sl[2 * i + j])
            else:
                assert residue(l) == a[i][j]
            out[18 * i + 9 * j:18 * i + 9 * j + 9] = l
    return out


def f12_of_limbs(vectors):
    """twelve limb vectors (c0, c1 of coefficient 0, ...) -> (the element's residues, its 108 words as they are)"""
    assert len(vectors) == 12
    a = [(residue(vectors[2 * i]), residue(vectors[2 * i + 1])) for i in range(6)]
    return a, np.asarray([x for l in vectors for x in l], dtype=np.uint32)


def record(a, b=None):
    r = np.zeros(REC_WORDS, dtype=np.uint32)
    r[0:EL_WORDS] = a
    if b is not None:
        r[EL_WORDS:] = b
    return r


def components(row):
    """raw words -> limb lists of nine, in order"""
    assert len(row) % 9 == 0
    return [[int(v) for v in row[9 * t:9 * t + 9]] for t in range(len(row) // 9)]


def residues(row):
    """raw words of Fq2 values (18 each) -> their residues, a list of pairs"""
    cs = components(row)
    return [(residue(cs[2 * i]), residue(cs[2 * i + 1])) for i in range(len(cs) // 2)]


def check_types(row, kv=EL, what=""):
    for t, l in enumerate(components(row)):
        lc.check_type(l, kv[0], kv[1], P, what=f"{what} coefficient {t // 2} component {t % 2}")


def check(row, want, what=""):
    """a raw output of Fq2 values: every component inside El AND exactly the residues of the reference"""
    check_types(row, EL, what)
    got = residues(row)
    assert got == [tuple(c) for c in want], f"{what}: residues differ from the reference in coefficients {[i for i, (g, w) in enumerate(zip(got, want)) if g != tuple(w)]}"


def _words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def wire_words(a):
    """what op 12 returns for an element of residues: eight canonical Montgomery (2^256) words per component, the ninth 0"""
    out = np.zeros(9 * 2 * len(a), dtype=np.uint32)
    for i, c in enumerate(a):
        for j in range(2):
            out[18 * i + 9 * j:18 * i + 9 * j + 8] = _words(c[j] * MONT % P)
    return out


def extreme_vectors(rng, v=2):
    """gen_type's extreme vectors of Lz<Fq29, 1, v>: (a) every low limb at 2^29 + 2^6 - 1 with the largest top limb, (b) the top limb
    alone, (c) v M - 1"""
    return lc.gen_type(1, v, P, rng, n_random=0)[:3]


# ---- Miller steps ---------------------------------------------------------------------------------------------------------------------
def raw_e2(c, ks=0, slack=False):
    ks, sl = _list(ks, 2, int), _list(slack, 2, bool)
    return rep_limbs(c[0], ks[0], sl[0]) + rep_limbs(c[1], ks[1], sl[1])


def step_record(t, q, xp, nyp, ks=0, slack=False, kb=(0, 0)):
    """108 words: T = (x, y, z) and Q = (qx, qy) of Fq2 residues, component m of the ten at representative ks[m] (El: 0 or 1) and shape
    slack[m]; xP and -yP (residues) at representatives kb (Base: 0 .. 3)"""
    ks, sl = _list(ks, 10, int), _list(slack, 10, bool)
    out = []
    for i, c in enumerate(list(t) + list(q)):
        out += raw_e2(c, ks[2 * i:2 * i + 2], sl[2 * i:2 * i + 2])
    out += rep_limbs(xp, kb[0]) + rep_limbs(nyp, kb[1])
    r = np.asarray(out, dtype=np.uint32)
    assert r.shape == (STEP_IN_WORDS,)
    return r


def step_inputs_in_type(row):
    cs = components(row)
    return all(lc.in_type(l, *EL, P) for l in cs[:10]) and all(lc.in_type(l, *BASE, P) for l in cs[10:])


def check_step(row, t3, line, what=""):
    """a 126-word output: T3 and the line's three coefficients inside El with the reference's residues, the lanes' differences zero"""
    assert not row[108:].any(), f"{what}: the lanes of the group disagree"
    check(row[:108], list(t3) + list(line), what)
