"""The Baby Jubjub group law of ed29.hpp on RAW limbs at the edges of the type it carries across the 256 iterations of a scalar
multiplication (uzk_test_ed_raw_kat: nothing re-limbed or reduced on the way in, nothing canonicalised on the way out).  Every
coordinate of an operand is a member of ed::C = Lz<Fr29, 1, 2>: the representative c or c + M, in normalized or carry-step limbs; and
points are built AROUND limb vectors (lz29_contract.gen_type's extreme vectors, ed_raw.shaped's carry-step vectors) standing as their Z
or their X as they are.  Every raw output coordinate must lie in C (K = 1, V = 2) AND hold exactly the residue of the extended law
restated on integers (tests/ed_raw.py); T Z = X Y; the affine result is ed_ref.add's.  The predicates hang on Fr::is_zero of a
canonicalised difference of products, which is a multiple of M here, never 0 itself as with canonical inputs."""
import zlib

import numpy as np
import pytest

import ed_raw as ew
import ed_ref as er
import lz29_contract as lc

pytestmark = pytest.mark.gpu
Q = ew.Q
MODES = ["min", "max"] + ["mix"] * 200


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _fr(rng):
    return int.from_bytes(rng.bytes(40), "little") % Q


def _z(rng):
    return _fr(rng) or 1


@pytest.fixture(scope="module")
def pts():
    return er.rand_subgroup_points(40, "ed-raw-gpu")


@pytest.fixture(scope="module")
def edge():
    """the identity and the points of order 2, 4, 4, 8, 8"""
    o8 = er.order8_point()
    return [er.IDENTITY, er.ORDER2, er.ORDER4[0], er.ORDER4[1], o8, er.neg(o8)]


def _point(rng, pt, mode, around=None):
    """(residues, 36 words) of pt under a random Z: every coordinate at k = 0, at k = 1, or at a random k and shape each -- a mix also
    takes a shaped limb vector as Z every other time; around = (builder, limbs) puts that vector in as Z or X instead"""
    if around is None and mode == "mix" and rng.integers(0, 2):
        around = (ew.around_z, ew.shaped(rng))
        while ew.residue(around[1]) == 0:
            around = (ew.around_z, ew.shaped(rng))
    p, ov = around[0](pt, around[1]) if around else (ew.ext_of(pt, _z(rng)), None)
    if mode == "min":
        return p, ew.raw_point(p, 0, False, ov)
    if mode == "max":
        return p, ew.raw_point(p, 1, False, ov)
    return p, ew.raw_point(p, [int(rng.integers(0, 2)) for _ in range(4)], [bool(rng.integers(0, 2)) for _ in range(4)], ov)


def _run(gpu, op, recs):
    assert 0 < len(recs) < 1000
    out = gpu.ed_raw_op(ew.OPS[op], np.stack(recs))
    assert out.shape == (len(recs), ew.OUT_WORDS)
    return out


def _check_sum(row, a, b, pa, pb, what):
    """the raw sum: in its type, the residues of the restated law, consistent, and the reference's affine point"""
    want = ew.ext_add(a, b)
    ew.check_point(row, want, what)
    assert row[36] == 0 and want[2] != 0 and ew.ext_consistent(want), what
    assert ew.ext_affine(ew.residues(row)) == er.add(pa, pb), what


def test_addition_at_every_representative(gpu, pts):
    """add on subgroup points under random Z: every coordinate of both operands at k = 0, at k = 1, 200 mixes of k and limb shape (half
    of them around a carry-step Z); then gen_type's extreme vectors as the Z and as the X of either operand, the other coordinates at
    k = 1 and mixed"""
    rng = _rng("add")
    cases = [(m, None, None) for m in MODES]
    for v in ew.extreme_vectors(rng):
        for build in (ew.around_z, ew.around_x):
            for mode in ("max", "mix"):
                cases += [(mode, (build, v), None), (mode, None, (build, v))]
    recs, args = [], []
    for i, (mode, ar_a, ar_b) in enumerate(cases):
        pa, pb = pts[i % 19], pts[19 + i % 17]
        a, ra = _point(rng, pa, mode, ar_a)
        b, rb = _point(rng, pb, mode, ar_b)
        recs.append(ew.record(ra, rb))
        args.append((a, b, pa, pb))
    out = _run(gpu, "add", recs)
    for i, row in enumerate(out):
        _check_sum(row, *args[i], f"add case {i} ({cases[i][0]})")


def test_addition_special_cases(gpu, pts, edge):
    """the unified law has no branch: P + P with another Z and other representatives on the right, P + (-P), the identity on either
    side, and the points of order 2, 4 and 8 with themselves, their negatives, each other and subgroup points"""
    rng = _rng("add-special")
    pairs = []
    for i in range(6):
        p = pts[i]
        pairs += [(p, p), (p, er.neg(p)), (er.IDENTITY, p), (p, er.IDENTITY)]
    pairs.append((er.IDENTITY, er.IDENTITY))
    for e in edge[1:]:
        pairs += [(e, e), (e, er.neg(e)), (e, pts[7]), (pts[8], e), (e, er.IDENTITY)] + [(e, o) for o in edge[1:] if o != e]
    recs, args = [], []
    for pa, pb in pairs:
        for mode in ("min", "max", "mix", "mix"):
            a, ra = _point(rng, pa, mode)
            b, rb = _point(rng, pb, mode)
            recs.append(ew.record(ra, rb))
            args.append((a, b, pa, pb))
    out = _run(gpu, "add", recs)
    for i, row in enumerate(out):
        _check_sum(row, *args[i], f"special case {i}: {pairs[i // 4]}")
    # the sums that are the identity are recognised as such from their raw limbs
    ident = [i for i, (_, _, pa, pb) in enumerate(args) if er.add(pa, pb) == er.IDENTITY]
    assert len(ident) >= 4 * 12
    flags = _run(gpu, "is_identity", [ew.record(out[i][:36]) for i in ident])
    assert all(r[36] == 1 for r in flags)


def test_negation_at_every_representative(gpu, pts, edge):
    rng = _rng("neg")
    cases = [(m, None) for m in ["min", "max"] + ["mix"] * 60]
    cases += [(mode, (build, v)) for v in ew.extreme_vectors(rng) for build in (ew.around_z, ew.around_x) for mode in ("max", "mix")]
    recs, want = [], []
    for i, (mode, ar) in enumerate(cases):
        pt = (pts + edge)[i % 46] if ar is None else pts[i % 40]
        a, ra = _point(rng, pt, mode, ar)
        recs.append(ew.record(ra))
        want.append((ew.ext_neg(a), er.neg(pt)))
    out = _run(gpu, "neg", recs)
    for i, row in enumerate(out):
        ew.check_point(row, want[i][0], f"neg case {i}")
        assert ew.ext_consistent(ew.residues(row)) and ew.ext_affine(ew.residues(row)) == want[i][1]


def _all_reps(c):
    """every member of C with residue c: k = 0, 1, each in both shapes where the second exists"""
    out = []
    for k in range(2):
        for slack in (False, True):
            l = ew.rep_limbs(c, k, slack)
            if l not in out:
                out.append(l)
    return out


def _off_by_one(rng, l):
    """a member of C next to l: the value one up or one down (the residue moves by 2^-261)"""
    v = lc.value(l)
    v += 1 if v == 0 or (v + 1 < 2 * Q and rng.integers(0, 2)) else -1
    return lc.limbs(v)


def _flags(gpu, op, cases):
    """cases = [(a words, b words or None, expected flag)]"""
    out = _run(gpu, op, [ew.record(a, b) for a, b, _ in cases])
    for i, (row, (_, _, want)) in enumerate(zip(out, cases)):
        assert int(row[36]) == want, f"{op} case {i}: flag {int(row[36])}, expected {want}"
        assert not row[:36].any()


def _put(row, i, l):
    r = row.copy()
    r[9 * i:9 * i + 9] = l
    return r


def test_is_identity_on_every_representative(gpu, pts):
    """(0 : Z : Z : 0): true for X at each representative of 0, Y and Z at every pair of theirs, both shapes, Z random or a shaped
    vector; false with X or Y one off, with X a multiple of M and Y != Z, with Y = Z and X not a multiple of M, and on other points"""
    rng = _rng("is_identity")
    cases = []
    for t in range(24):
        zl = ew.shaped(rng) if t % 2 else ew.rep_limbs(_z(rng), t % 4 // 2, True)
        z = ew.residue(zl)
        for xl in _all_reps(0):
            for yl in _all_reps(z):
                row = np.asarray(xl + yl + list(zl) + ew.rep_limbs(0, t % 2), dtype=np.uint32)
                assert ew.ext_affine(ew.residues(row)) == er.IDENTITY
                cases.append((row, None, 1))
                cases.append((_put(row, 0, _off_by_one(rng, xl)), None, 0))
                cases.append((_put(row, 1, _off_by_one(rng, yl)), None, 0))
                cases.append((_put(row, 1, ew.rep_limbs(_z(rng), t % 2)), None, 0))               # X a multiple of M, Y != Z
                cases.append((_put(row, 0, ew.rep_limbs(_z(rng), t % 2)), None, 0))               # Y = Z, X not
    for i, mode in enumerate(["min", "max"] + ["mix"] * 20):
        cases.append((_point(rng, pts[i], mode)[1], None, 0))
    assert all(lc.in_type(l, *ew.C, Q) for a, _, _ in cases for l in ew.coords(a))
    for lo in range(0, len(cases), 900):
        _flags(gpu, "is_identity", cases[lo:lo + 900])


def test_eq_affine_on_every_representative(gpu, pts, edge):
    """X = ax Z and Y = ay Z without an inversion: true for the point's own affine coordinates at every representative and shape of
    theirs and of the point's; false with ax, ay, X or Y one off and against (x, -y) and (-x, y), where one of the two differences is a
    multiple of M and the other is not"""
    rng = _rng("eq_affine")
    cases = []
    for i, mode in enumerate(["min", "max"] + ["mix"] * 40):
        pt = (pts + edge)[i]
        _, ra = _point(rng, pt, mode)
        for xl in _all_reps(pt[0]):
            for yl in _all_reps(pt[1]):
                b = np.asarray(xl + yl + [0] * 18, dtype=np.uint32)
                cases.append((ra, b, 1))
        xl, yl = ew.rep_limbs(pt[0], i % 2), ew.rep_limbs(pt[1], 1 - i % 2)
        b = np.asarray(xl + yl + [0] * 18, dtype=np.uint32)
        cases.append((ra, _put(b, 0, _off_by_one(rng, xl)), 0))
        cases.append((ra, _put(b, 1, _off_by_one(rng, yl)), 0))
        cases.append((_put(ra, 0, _off_by_one(rng, ew.coords(ra)[0])), b, 0))
        cases.append((_put(ra, 1, _off_by_one(rng, ew.coords(ra)[1])), b, 0))
        if pt[1] != 0:
            cases.append((ra, _put(b, 1, ew.rep_limbs(Q - pt[1], i % 2)), 0))
        if pt[0] != 0:
            cases.append((ra, _put(b, 0, ew.rep_limbs(Q - pt[0], i % 2)), 0))
    assert sum(c[2] for c in cases) >= 4 * 42
    for lo in range(0, len(cases), 900):
        _flags(gpu, "eq_affine", cases[lo:lo + 900])


def test_on_curve_on_every_representative(gpu, pts, edge):
    """x^2 + y^2 = 1 + d x^2 y^2 on affine coordinates at every representative and shape; false with either coordinate one off in
    value, or one off in residue"""
    rng = _rng("on_curve")
    cases = []
    for i, pt in enumerate(pts + edge):
        for xl in _all_reps(pt[0]):
            for yl in _all_reps(pt[1]):
                row = np.asarray(xl + yl + [0] * 18, dtype=np.uint32)
                cases.append((row, None, 1))
                cases.append((_put(row, i % 2, _off_by_one(rng, (xl, yl)[i % 2])), None, 0))
        bad = ((pt[0] + 1) % Q, pt[1]) if i % 2 else (pt[0], (pt[1] + 1) % Q)
        assert er.on_curve(pt) and not er.on_curve(bad)
        cases.append((np.asarray(ew.rep_limbs(bad[0], i % 2) + ew.rep_limbs(bad[1], 1 - i % 2) + [0] * 18, dtype=np.uint32), None, 0))
    _flags(gpu, "on_curve", cases)


def test_to_affine_and_inverse(gpu, pts, edge):
    """to_affine: the canonical wire words of ed_ref.affine's point from every representative, shape and extreme Z or X.  inv: the raw
    inverse inside C with the residue of the reference, of ordinary values, of the extreme vectors, and of each representative of 0
    (whose inverse is a representative of 0)."""
    rng = _rng("to_affine")
    cases = [(m, None) for m in ["min", "max"] + ["mix"] * 44]
    cases += [(mode, (build, v)) for v in ew.extreme_vectors(rng) for build in (ew.around_z, ew.around_x) for mode in ("max", "mix")]
    recs, want = [], []
    for i, (mode, ar) in enumerate(cases):
        pt = (pts + edge)[i % 46] if ar is None else pts[i % 40]
        a, ra = _point(rng, pt, mode, ar)
        assert er.affine(a[:3]) == pt
        recs.append(ew.record(ra))
        want.append(ew.wire_affine(pt))
    out = _run(gpu, "to_affine", recs)
    for i, row in enumerate(out):
        assert np.array_equal(row, want[i]), f"to_affine case {i}"
    vs = ew.extreme_vectors(rng) + [ew.shaped(rng) for _ in range(20)] + _all_reps(0) + _all_reps(1) + _all_reps(Q - 1) + _all_reps(2)
    out = _run(gpu, "inv", [ew.record(np.asarray(list(l) + [0] * 27, dtype=np.uint32)) for l in vs])
    for i, (l, row) in enumerate(zip(vs, out)):
        ew.check_coord(ew.coords(row)[0], pow(ew.residue(l), Q - 2, Q), f"inv case {i}")
        assert not row[9:].any()
