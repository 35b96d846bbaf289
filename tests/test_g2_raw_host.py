"""CPU checks of tests/g2_raw.py, the host side of the raw-limb G2 known answers: representatives round-trip through the raw record,
every one of them lies in its type, the XYZZ formulas restated on residues agree with the reference (g2_ref's Jacobian additions and
the oracle's affine g2_add), and the record builders are laid out as include/uzkge_gpu_test.h states."""
import random

import numpy as np
import pytest

import bn254_pairing as bp
import g2_raw as gr
import g2_ref as g
import lz29_contract as lc


@pytest.fixture(scope="module")
def fin():
    seen, out = set(), []
    for q in g.load_fixture()[1]:
        if q is not None and q not in seen and g.g2_neg(q) not in seen:
            seen.add(q)
            out.append(q)
    return out[:24]


def _z(rng):
    return (rng.randrange(1, g.P), rng.randrange(g.P))


def test_representatives_round_trip_and_lie_in_their_types(fin):
    rng = random.Random(1)
    for q in fin[:6]:
        p = gr.xyzz_of(q, _z(rng))
        assert gr.xyzz_affine(p) == q and gr.xyzz_consistent(p)
        for forms, kmax, types in ((gr.FORMS_P, gr.KMAX_P, gr.TYPES_P), (gr.FORMS_ACC, gr.KMAX_ACC, gr.TYPES_ACC)):
            for ks in (0, [kmax[t // 2] for t in range(8)], [rng.randrange(kmax[t // 2] + 1) for t in range(8)]):
                for slack in (False, True):
                    row = gr.raw_point(p, forms, ks, slack)
                    gr.check_types(row, types)
                    assert gr.residues(row, forms) == p and gr.xyzz_affine(gr.residues(row, forms)) == q
                    kk = [ks] * 8 if isinstance(ks, int) else ks
                    cs, inf = gr.coords(row)
                    assert inf == 0 and [lc.value(c) // g.P for c in cs] == kk                 # exactly the representative asked for
    assert gr.residues(gr.raw_point(None)) is None and gr.raw_point(None)[72] == 1
    # one more than the largest representative leaves the type: the k ranges are the types' own
    with pytest.raises(AssertionError):
        gr.check_types(gr.raw_point(p, gr.FORMS_P, 16), gr.TYPES_P)
    with pytest.raises(AssertionError):
        gr.check_types(gr.raw_point(p, gr.FORMS_ACC, [0, 0, 0, 0, 2, 0, 0, 0]), gr.TYPES_ACC)


def test_carry_step_keeps_the_value_and_the_limb_bound():
    l = lc.limbs(5 + (7 << 29) + (3 << 58) + (123456 << 232))
    r = gr.carry_step(l)
    assert r != l and lc.value(r) == lc.value(l) and all(x < lc.B + 64 for x in r[:8]) and max(r[:8]) >= lc.B
    full = lc.limbs((1 << 232) - 1)
    assert gr.carry_step(full) == full


def test_shaped_zz_points_carry_the_extreme_limbs(fin):
    rng = np.random.default_rng(3)
    for acc in (False, True):
        forms, types = (gr.FORMS_ACC, gr.TYPES_ACC) if acc else (gr.FORMS_P, gr.TYPES_P)
        shaped = gr.shaped_zz(rng, acc)
        assert len(shaped) >= 4
        assert any(max(ov[(2, 0)][:8]) == lc.B + 63 for _, ov in shaped)                       # gen_type's shape (a) is among them
        for z, ov in shaped:
            p = gr.xyzz_of(fin[0], z)
            row = gr.raw_point(p, forms, 0, False, ov)
            gr.check_types(row, types)
            assert gr.coords(row)[0][4] == ov[(2, 0)] and gr.coords(row)[0][5] == ov[(2, 1)]
            assert gr.xyzz_affine(gr.residues(row, forms)) == fin[0]


def test_xyzz_formulas_agree_with_the_reference(fin):
    rng = random.Random(2)
    for i in range(0, 12, 2):
        p, q = fin[i], fin[i + 1]
        a, b = gr.xyzz_of(p, _z(rng)), gr.xyzz_of(q, _z(rng))
        s = gr.xyzz_add(a, b)
        assert gr.xyzz_consistent(s) and gr.xyzz_affine(s) == bp.g2_add(p, q) == g.jac_to_affine(g.jac_madd((p[0], p[1], (1, 0)), q))
        d = gr.xyzz_dbl(a)
        assert gr.xyzz_consistent(d) and gr.xyzz_affine(d) == bp.g2_add(p, p)
        assert gr.xyzz_affine(gr.xyzz_add(a, gr.xyzz_of(p, _z(rng)))) == bp.g2_add(p, p)        # same point, another z: doubling
        assert gr.xyzz_add(a, gr.xyzz_of(g.g2_neg(p), _z(rng))) is None
        assert gr.xyzz_add(a, None) == a and gr.xyzz_add(None, b) == b and gr.xyzz_add(None, None) is None and gr.xyzz_dbl(None) is None
        for neg in (False, True):
            want = bp.g2_add(p, bp.g2_neg(q) if neg else q)
            m = gr.xyzz_madd(a, q, neg)
            assert gr.xyzz_consistent(m) and gr.xyzz_affine(m) == want
        assert gr.xyzz_affine(gr.xyzz_madd(a, p)) == bp.g2_add(p, p) and gr.xyzz_madd(a, p, True) is None
        assert gr.xyzz_affine(gr.xyzz_madd(a, g.g2_neg(p), True)) == bp.g2_add(p, p) and gr.xyzz_madd(a, g.g2_neg(p)) is None
        assert gr.xyzz_madd(None, q, True) == (q[0], g.f2_neg(q[1]), (1, 0), (1, 0)) and gr.xyzz_madd(a, None) == a


def test_record_layout(fin):
    q = fin[0]
    w = gr.wire_point(q)
    ref = g.points_to_wire([q])[0].view(np.uint32)                   # 16 u64 = x.c0, x.c1, y.c0, y.c1 of eight 32-bit words each
    got = np.concatenate([w[0:8], w[9:17], w[18:26], w[27:35]])
    assert np.array_equal(got, ref) and not w[35:].any() and w[8] == w[17] == 0
    assert not gr.wire_point(None).any()
    p = gr.xyzz_of(q, (3, 5))
    ww = gr.wire_words(p)
    assert np.array_equal(np.concatenate([ww[0:8], ww[9:17]]), g.fq2_to_wire(p[0]).view(np.uint32)) and ww[72] == 0
    assert gr.wire_words(None)[72] == 1 and not gr.wire_words(None)[:72].any()
    r = gr.record(gr.raw_point(p), w, 1)
    assert r.shape == (gr.REC_WORDS,) and np.array_equal(r[73:146], w) and r[146] == 1 and r.dtype == np.uint32
