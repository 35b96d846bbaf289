"""The G2 group law of g2_29.hpp on RAW limbs at the edges of the bounds it carries across loop iterations (uzk_test_g2_raw_kat: nothing
re-limbed or reduced on the way in, nothing canonicalised on the way out).  Accumulator X, Y and every coordinate of a full point at
their smallest and largest representatives below 16 M (k = 0 .. 15), the accumulator's ZZ, ZZZ below 2 M in the 2^266-form, in
normalized and in carry-step limbs.  Every raw output coordinate must lie in the type the code assigns it AND hold the residue of the
XYZZ formulas on integers (tests/g2_raw.py); the affine result is compared with the oracle's g2_add.  The doubling and cancellation
branches hang on q2::is_zero of a difference that is a large multiple of M here, never 0 or M as with canonical inputs."""
import zlib

import numpy as np
import pytest

import bn254_pairing as bp
import g2_raw as gr
import g2_ref as g
import lz29_contract as lc
from lz29_contract import limbs

pytestmark = pytest.mark.gpu
P = g.P


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@pytest.fixture(scope="module")
def fin():
    """distinct finite points of the fixture's b_g2_query column, no two of them opposite"""
    seen, out = set(), []
    for q in g.load_fixture()[1]:
        if q is not None and q not in seen and g.g2_neg(q) not in seen:
            seen.add(q)
            out.append(q)
    return out[:64]


def _z(rng):
    return (int(rng.integers(1, 1 << 62)) * (P >> 62) % P, int(rng.integers(0, 1 << 62)) * (P >> 63) % P)


def _ks(rng, kmax, mode):
    if mode == "min":
        return [0] * 8
    if mode == "max":
        return [kmax[t // 2] for t in range(8)]
    return [int(rng.integers(0, kmax[t // 2] + 1)) for t in range(8)]


def _slack(rng, mode):
    return [False] * 8 if mode in ("min", "max") else [bool(rng.integers(0, 2)) for _ in range(8)]


def _run(gpu, op, recs):
    assert 0 < len(recs) < 1000
    return gpu.g2_raw_op(op, np.stack(recs))


def _check(row, want, forms, types, what):
    """the raw output: in its types, the residues of the integer formulas, consistent, and the oracle's affine point"""
    gr.check_types(row, types, what)
    got = gr.residues(row, forms)
    assert got == want, what
    assert gr.xyzz_consistent(got), what


MODES = ["min", "max"] + ["mix"] * 208


@pytest.mark.parametrize("op", ["add", "dbl", "madd", "msub"])
def test_generic_additions_at_every_representative(gpu, fin, op):
    """P + Q (full), 2 P, P + Q and P - Q (mixed): every coordinate of every operand at its smallest representative, at its largest
    (k = 15, k = 1 for the accumulator's ZZ, ZZZ), and 208 random mixes of k and of the two limb shapes; then points built around
    gen_type's extreme limb vectors as ZZ"""
    rng = _rng("generic", op)
    acc = op in ("madd", "msub")
    forms, kmax, types = (gr.FORMS_ACC, gr.KMAX_ACC, gr.TYPES_ACC) if acc else (gr.FORMS_P, gr.KMAX_P, gr.TYPES_P)
    cases = [(m, None) for m in MODES] + [("max", s) for s in gr.shaped_zz(rng, acc)] + [("mix", s) for s in gr.shaped_zz(rng, acc)]
    recs, want, aff = [], [], []
    for i, (mode, shaped) in enumerate(cases):
        p, q = fin[i % 31], fin[31 + i % 29]
        za, ov = shaped if shaped else (_z(rng), None)
        a = gr.xyzz_of(p, za)
        ra = gr.raw_point(a, forms, _ks(rng, kmax, mode), _slack(rng, mode), ov)
        if op == "add":
            b = gr.xyzz_of(q, _z(rng))
            recs.append(gr.record(ra, gr.raw_point(b, forms, _ks(rng, kmax, mode), _slack(rng, mode))))
            want.append(gr.xyzz_add(a, b))
            aff.append(bp.g2_add(p, q))
        elif op == "dbl":
            recs.append(gr.record(ra))
            want.append(gr.xyzz_dbl(a))
            aff.append(bp.g2_add(p, p))
        else:
            recs.append(gr.record(ra, gr.wire_point(q), int(op == "msub")))
            want.append(gr.xyzz_madd(a, q, op == "msub"))
            aff.append(bp.g2_add(p, bp.g2_neg(q) if op == "msub" else q))
    out = _run(gpu, {"add": 0, "dbl": 1, "madd": 2, "msub": 2}[op], recs)
    for i, row in enumerate(out):
        _check(row, want[i], forms, types, f"{op} case {i} ({cases[i][0]})")
        assert gr.xyzz_affine(want[i]) == aff[i] and aff[i] is not None


def _same_point_cases(rng, fin, forms, kmax):
    """(a residues, raw a, point) with the accumulator side's X and Y at every k = 0 .. 15 (both components, then one component at k
    and the other random), under a random z, ZZ / ZZZ at random representatives"""
    out = []
    for k in range(16):
        for both in (True, False):
            p = fin[(2 * k + both) % len(fin)]
            a = gr.xyzz_of(p, _z(rng))
            ks = _ks(rng, kmax, "mix")
            ks[0] = ks[2] = k
            if both:
                ks[1] = ks[3] = k
            out.append((a, gr.raw_point(a, forms, ks, _slack(rng, "mix")), p))
    return out


def test_full_addition_of_one_point_under_different_representatives(gpu, fin):
    """g2p_add(P, P) with another z and other representatives on the right: the doubling branch (is_zero of U2 - U1, S2 - S1, both
    large multiples of M) gives 2 P; with -P instead the flag is set, and storing that result gives zero words"""
    rng = _rng("same-full")
    cases = _same_point_cases(rng, fin, gr.FORMS_P, gr.KMAX_P)
    recs, want = [], []
    for a, ra, p in cases:
        for other in (p, g.g2_neg(p)):
            mode = ("min", "max", "mix")[len(recs) % 3]
            b = gr.xyzz_of(other, _z(rng))
            recs.append(gr.record(ra, gr.raw_point(b, gr.FORMS_P, _ks(rng, gr.KMAX_P, mode), _slack(rng, mode))))
            want.append((gr.xyzz_add(a, b), bp.g2_add(p, other)))
    out = _run(gpu, 0, recs)
    for i, row in enumerate(out):
        res, aff = want[i]
        if i % 2 == 0:
            assert res is not None and gr.coords(row)[1] == 0, f"case {i}: the doubling branch was not taken (result at infinity)"
            _check(row, res, gr.FORMS_P, gr.TYPES_P, f"P + P case {i}")
            assert gr.xyzz_affine(res) == aff
        else:
            assert res is None and aff is None and gr.coords(row)[1] == 1, f"case {i}: P + (-P) is not flagged infinite"
            gr.check_types(row, gr.TYPES_P, f"P - P case {i}")
    stored = _run(gpu, 3, [gr.record(row) for row in out[1::2]])
    assert all(r[72] == 1 and not r[:72].any() for r in stored)


def test_mixed_addition_of_the_accumulators_own_point(gpu, fin):
    """g2acc_madd(acc = P, P): X and Y of the accumulator at c + k M for every k, so U2 - X is about (k + 1) M: the doubling branch
    restarts from 2 P of the wire point; -P (by the wire point or by the negate flag) cancels to infinity"""
    rng = _rng("same-mixed")
    cases = _same_point_cases(rng, fin, gr.FORMS_ACC, gr.KMAX_ACC)
    recs, want = [], []
    for a, ra, p in cases:
        for q, neg in ((p, 0), (g.g2_neg(p), 1), (g.g2_neg(p), 0), (p, 1)):
            recs.append(gr.record(ra, gr.wire_point(q), neg))
            want.append((gr.xyzz_madd(a, q, bool(neg)), bp.g2_add(p, bp.g2_neg(q) if neg else q)))
    out = _run(gpu, 2, recs)
    for i, row in enumerate(out):
        res, aff = want[i]
        if i % 4 < 2:
            assert res is not None and gr.coords(row)[1] == 0, f"case {i}: the doubling branch was not taken (bucket at infinity)"
            _check(row, res, gr.FORMS_ACC, gr.TYPES_ACC, f"acc + own point case {i}")
            assert gr.xyzz_affine(res) == aff
        else:
            assert res is None and aff is None and gr.coords(row)[1] == 1, f"case {i}: acc - own point is not flagged infinite"
            gr.check_types(row, gr.TYPES_ACC, f"acc - own point case {i}")
    stored = _run(gpu, 3, [gr.record(row, None, 1) for row in out[2::4]])
    assert all(r[72] == 1 and not r[:72].any() for r in stored)


def test_infinity_on_either_side_and_on_both(gpu, fin):
    rng = _rng("inf")
    inf = gr.raw_point(None)
    for mode in ("min", "max", "mix"):
        p, q = fin[3], fin[4]
        a, b = gr.xyzz_of(p, _z(rng)), gr.xyzz_of(q, _z(rng))
        ra = gr.raw_point(a, gr.FORMS_P, _ks(rng, gr.KMAX_P, mode), _slack(rng, mode))
        rb = gr.raw_point(b, gr.FORMS_P, _ks(rng, gr.KMAX_P, mode), _slack(rng, mode))
        out = _run(gpu, 0, [gr.record(inf, rb), gr.record(ra, inf), gr.record(inf, inf)])
        assert np.array_equal(out[0], rb) and np.array_equal(out[1], ra) and out[2][72] == 1       # the other operand, limb for limb
        out = _run(gpu, 1, [gr.record(inf)])
        assert out[0][72] == 1
        rc = gr.raw_point(a, gr.FORMS_ACC, _ks(rng, gr.KMAX_ACC, mode), _slack(rng, mode))
        out = _run(gpu, 2, [gr.record(inf, gr.wire_point(q), 0), gr.record(inf, gr.wire_point(q), 1), gr.record(rc, gr.wire_point(None), 0),
                            gr.record(rc, gr.wire_point(None), 1), gr.record(inf, gr.wire_point(None), 0)])
        _check(out[0], (q[0], q[1], (1, 0), (1, 0)), gr.FORMS_ACC, gr.TYPES_ACC, "inf + q")
        _check(out[1], (q[0], g.f2_neg(q[1]), (1, 0), (1, 0)), gr.FORMS_ACC, gr.TYPES_ACC, "inf - q")
        assert np.array_equal(out[2], rc) and np.array_equal(out[3], rc) and out[4][72] == 1


def test_stores_of_extreme_representatives_are_canonical(gpu, fin):
    """g2p_store (to_wire at V = 16) and g2acc_store (to_wire, to_wire_266) on the smallest, the largest and mixed representatives, and
    on points around gen_type's extreme ZZ limbs: the canonical words of the residues"""
    rng = _rng("store")
    for acc in (False, True):
        forms, kmax = (gr.FORMS_ACC, gr.KMAX_ACC) if acc else (gr.FORMS_P, gr.KMAX_P)
        cases = [(m, None) for m in ["min", "max"] + ["mix"] * 30] + [("max", s) for s in gr.shaped_zz(rng, acc)]
        recs, want = [], []
        for i, (mode, shaped) in enumerate(cases):
            z, ov = shaped if shaped else (_z(rng), None)
            a = gr.xyzz_of(fin[i % len(fin)], z)
            recs.append(gr.record(gr.raw_point(a, forms, _ks(rng, kmax, mode), _slack(rng, mode), ov), None, int(acc)))
            want.append(gr.wire_words(a))
        recs.append(gr.record(gr.raw_point(None), None, int(acc)))
        want.append(gr.wire_words(None))
        out = _run(gpu, 3, recs)
        for i, row in enumerate(out):
            assert np.array_equal(row, want[i]), (acc, i)


def _borrowed(l):
    """the same value with 2^29 borrowed into every low limb that has a limb above to borrow from: limbs below 2^30, far outside the
    K = 1 bound but well inside reduce()'s own contract (limbs < 2^32 - 2^3), which is all q2::is_zero relies on"""
    l = list(l)
    for i in range(8):
        if l[i + 1] >= 1:
            l[i] += lc.B
            l[i + 1] -= 1
    return l


def _shapes(v):
    out = [limbs(v)]
    for s in (gr.carry_step(out[0]), _borrowed(out[0])):
        if s not in out:
            out.append(s)
    return out


def test_is_zero_is_exact_below_32M(gpu):
    """q2::is_zero on E2<1, 32>: true exactly for (k M, k' M), k, k' = 0 .. 31; false for k M +- 1 in either component and when only one
    component is a multiple of M.  Shapes: normalized limbs; the carry-step restatement within the K = 1 bound, which no k M or
    k M +- 1 below 32 M has for BN254's q (it needs a digit below 2^6; asserted below), so the un-normalized form of these exact values
    is the one with 2^29 borrowed into every low limb; and the free component in gen_type's extreme shapes (every low limb at
    2^29 + 2^6 - 1)."""
    rng = _rng("is_zero")
    ext = [l for l in lc.gen_type(1, 32, P, rng, n_random=12) if lc.value(l) % P != 0]
    assert max(ext[0][:8]) == lc.B + 63
    cases = []
    for k in range(32):
        for k2 in (k, 31 - k, 0):
            for la in _shapes(k * P):
                for lb in _shapes(k2 * P):
                    cases.append((la, lb, 1))
        for d in (-1, 1):
            v = k * P + d
            if not 0 <= v < 32 * P:
                continue
            for lv in _shapes(v):
                for other in (k * P, 0, 31 * P):
                    cases.append((lv, limbs(other), 0))
                    cases.append((limbs(other), lv, 0))
                cases.append((lv, lv, 0))
        for e in ext[:4] + [ext[4 + k % (len(ext) - 4)]]:
            cases.append((limbs(k * P), e, 0))
            cases.append((e, limbs(k * P), 0))
    assert all(gr.carry_step(limbs(k * P + d)) == limbs(k * P + d) for k in range(32) for d in (-1, 0, 1) if k * P + d >= 0)
    assert all(len(_shapes(k * P)) == 2 for k in range(1, 32))
    for lo in range(0, len(cases), 512):
        part = cases[lo:lo + 512]
        recs = []
        for la, lb, _ in part:
            row = np.zeros(gr.PT_WORDS, dtype=np.uint32)
            row[0:9], row[9:18] = la, lb
            assert all(max(x[:8]) < 1 << 30 and lc.value(x) < 32 * P for x in (la, lb))
            recs.append(gr.record(row))
        out = _run(gpu, 4, recs)
        for (la, lb, want), row in zip(part, out):
            assert int(row[72]) == want, (lc.value(la) / P, lc.value(lb) / P, want)
            assert not row[:72].any()
