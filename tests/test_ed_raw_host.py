"""CPU checks of tests/ed_raw.py, the host side of the raw-limb Baby Jubjub known answers: representatives round-trip through the raw
record, every generated input lies in its type, the extended law restated on residues agrees with ed_ref.add (random, edge and
doubling cases), points built around given limbs carry them, the checkers REJECT outputs that are the right residue outside the type
or a wrong residue inside it, and the hook checks its arguments before the device."""
import ctypes
import random

import numpy as np
import pytest

import ed_raw as ew
import ed_ref as er
import lz29_contract as lc

Q = ew.Q


@pytest.fixture(scope="module")
def pts():
    return er.rand_subgroup_points(12, "ed-raw-host")


def _edge_points():
    o8 = er.order8_point()
    return [er.IDENTITY, er.ORDER2, er.ORDER4[0], er.ORDER4[1], o8, er.neg(o8)]


def test_representatives_round_trip_and_lie_in_their_type(pts):
    rng = random.Random(1)
    for pt in pts[:4] + _edge_points():
        p = ew.ext_of(pt, rng.randrange(1, Q))
        assert ew.ext_affine(p) == pt and ew.ext_consistent(p)
        for ks in (0, 1, [rng.randrange(2) for _ in range(4)]):
            for slack in (False, True):
                row = ew.raw_point(p, ks, slack)
                ew.check_types(row)
                assert ew.residues(row) == p and ew.ext_affine(ew.residues(row)) == pt
                kk = [ks] * 4 if isinstance(ks, int) else ks
                assert [lc.value(c) // Q for c in ew.coords(row)] == kk                # exactly the representative asked for
    with pytest.raises(AssertionError):                                              # k = 2 leaves ed::C
        ew.check_types(ew.raw_point(p, [0, 0, 2, 0]))


def test_the_extended_law_agrees_with_the_reference(pts):
    rng = random.Random(2)
    z = lambda: rng.randrange(1, Q)
    edge = _edge_points()
    assert er.mul(2, edge[1]) == er.IDENTITY and er.mul(2, edge[2]) == edge[1] and er.mul(4, edge[4]) == edge[1]   # orders 2, 4, 8
    cases = [(pts[i], pts[i + 1]) for i in range(0, 8, 2)]
    cases += [(p, p) for p in pts[:3]] + [(p, er.neg(p)) for p in pts[:3]]            # doubling under two Z, cancellation
    cases += [(e, p) for e in edge for p in (pts[0], e, er.neg(e), edge[4])] + [(pts[1], e) for e in edge]
    for a, b in cases:
        s = ew.ext_add(ew.ext_of(a, z()), ew.ext_of(b, z()))
        assert s[2] != 0 and ew.ext_consistent(s) and ew.ext_affine(s) == er.add(a, b)
        n = ew.ext_neg(ew.ext_of(a, z()))
        assert ew.ext_consistent(n) and ew.ext_affine(n) == er.neg(a)
    assert ew.ext_affine(ew.ext_add(ew.ext_of(pts[0], z()), ew.ext_of(pts[0], z()))) == er.affine_double(pts[0])


def test_points_around_given_limbs_carry_them(pts):
    rng = np.random.default_rng(3)
    vs = ew.extreme_vectors(rng) + [ew.shaped(rng) for _ in range(24)]
    assert max(vs[0][:8]) == min(vs[0][:8]) == lc.B + 63 and not any(vs[1][:8]) and lc.value(vs[2]) == 2 * Q - 1
    assert sum(x >= lc.B for l in vs[3:] for x in l[:8]) > 50 and any(lc.value(l) >= Q for l in vs[3:])
    for i, l in enumerate(vs):
        assert lc.in_type(l, *ew.C, Q)
        pt = pts[i % len(pts)]
        for build, at in ((ew.around_z, 2), (ew.around_x, 0)):
            p, ov = build(pt, l)
            row = ew.raw_point(p, 1, False, ov)
            ew.check_types(row)
            assert ew.coords(row)[at] == l and ew.ext_affine(ew.residues(row)) == pt and ew.ext_consistent(ew.residues(row))


def test_record_layout(pts):
    p, q = ew.ext_of(pts[0], 3), ew.ext_of(pts[1], 5)
    r = ew.record(ew.raw_point(p), ew.raw_point(q, 1))
    assert r.shape == (ew.REC_WORDS,) and r.dtype == np.uint32 and ew.residues(r[:36]) == p and ew.residues(r[36:]) == q
    assert not ew.record(ew.raw_point(p))[36:].any()
    w = ew.wire_affine(pts[0])
    ref = er.points_wire([pts[0]])[0].view(np.uint32)                                 # x then y, eight 32-bit words each
    assert w.shape == (ew.OUT_WORDS,) and np.array_equal(np.concatenate([w[0:8], w[9:17]]), ref) and w[8] == 0 and not w[17:].any()


def _over_limb(rng, i):
    """a limb vector of value below M whose low limb i is exactly 2^29 + 2^6 -- the first value outside K = 1 -- the others plain digits"""
    l = [rng.randrange(lc.B) for _ in range(8)] + [rng.randrange(1 << 20)]
    l[i] = lc.B + 64
    assert lc.value(l) < Q and not lc.in_type(l, *ew.C, Q)
    return l


def test_the_checker_accepts_a_correct_output_and_rejects_wrong_ones(pts):
    rng = random.Random(4)
    want = ew.ext_add(ew.ext_of(pts[2], rng.randrange(1, Q)), ew.ext_of(pts[3], rng.randrange(1, Q)))
    row = ew.raw_point(want, [rng.randrange(2) for _ in range(4)])
    ew.check_point(row, want)
    for i in range(4):
        # the right residue, raised by M beyond 2 M
        bad = row.copy()
        bad[9 * i:9 * i + 9] = lc.limbs(ew.rep_value(want[i], 2))
        assert ew.residues(bad) == want
        with pytest.raises(AssertionError, match="outside Lz<1, 2>"):
            ew.check_point(bad, want)
        # the right residue, a value below M, one low limb at 2^29 + 2^6: the reference is made to hold this vector's residue
        over = _over_limb(rng, 2 * i)
        want2 = tuple(ew.residue(over) if j == i else want[j] for j in range(4))
        ew.check_point(ew.raw_point(want2), want2)
        bad = ew.raw_point(want2, 0, False, {i: over})
        assert ew.residues(bad) == want2
        with pytest.raises(AssertionError, match="outside Lz<1, 2>"):
            ew.check_point(bad, want2)
        with pytest.raises(AssertionError, match="outside Lz<1, 2>"):
            ew.check_coord(over, ew.residue(over))
        # inside the type, the residue off by one
        bad = row.copy()
        bad[9 * i:9 * i + 9] = ew.rep_limbs((want[i] + 1) % Q, 1)
        ew.check_types(bad)
        with pytest.raises(AssertionError, match="residues differ"):
            ew.check_point(bad, want)
        with pytest.raises(AssertionError, match="residue differs"):
            ew.check_coord(ew.coords(bad)[i], want[i])


def test_the_hook_checks_its_arguments_before_the_device():
    from uzkge_amd import _native as N, backend as b
    p = np.zeros(72, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p)
    E = N.UZK_ERR_PARAMETER
    fn = N.lib.uzk_test_ed_raw_kat
    assert fn(0, None, p, 1) == E and fn(0, p, None, 1) == E
    assert fn(7, p, p, 1) == E and fn(-1, p, p, 1) == E
    if b.device_count() == 0:
        assert fn(0, p, p, 1) == N.UZK_ERR_DEVICE
