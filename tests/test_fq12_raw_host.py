"""CPU checks of tests/fq12_raw.py, the host side of the raw-limb Fq12 and Miller-step known answers: representatives round-trip
through the raw records, every generated input lies in its type, the records are laid out as include/uzkge_gpu_test.h states, the
checkers REJECT outputs that are the right residue outside the type or a wrong residue inside it, and the hooks check their arguments
before the device."""
import ctypes
import random

import numpy as np
import pytest

import bn254_pairing as bp
import fq12_raw as fr
import g2_ref as g2
import lz29_contract as lc
import pairing_cases as pc
import pairing_ref as pr

P = fr.P


def test_representatives_round_trip_and_lie_in_their_type():
    rng = random.Random(1)
    for a in [pc.rand_f12(rng) for _ in range(4)] + pc.edge_f12():
        for ks in (0, 1, [rng.randrange(2) for _ in range(12)]):
            for slack in (False, True):
                row = fr.raw_f12(a, ks, slack)
                fr.check_types(row)
                assert fr.residues(row) == a
                kk = [ks] * 12 if isinstance(ks, int) else ks
                assert [lc.value(c) // P for c in fr.components(row)] == kk          # exactly the representative asked for
    with pytest.raises(AssertionError):                                              # k = 2 leaves El: the k range is the type's own
        fr.check_types(fr.raw_f12(a, [0] * 7 + [2] + [0] * 4))
    for k in range(4):
        assert lc.in_type(fr.rep_limbs(12345, k), *fr.BASE, P) and fr.residue(fr.rep_limbs(12345, k)) == 12345
    assert not lc.in_type(fr.rep_limbs(12345, 4), *fr.BASE, P)


def test_shaped_and_extreme_vectors_lie_in_their_type_and_carry_the_shapes():
    rng = np.random.default_rng(2)
    vs = [fr.shaped(rng) for _ in range(48)]
    assert all(lc.in_type(l, *fr.EL, P) for l in vs)
    assert sum(x >= lc.B for l in vs for x in l[:8]) > 100 and any(lc.value(l) >= P for l in vs) and any(lc.value(l) < P for l in vs)
    ext = fr.extreme_vectors(rng)
    assert len(ext) == 3 and max(ext[0][:8]) == min(ext[0][:8]) == lc.B + 63 and not any(ext[1][:8]) and lc.value(ext[2]) == 2 * P - 1
    a, row = fr.f12_of_limbs(ext + ext + ext + [fr.shaped(rng) for _ in range(3)])
    fr.check_types(row)
    assert fr.residues(row) == a and fr.components(row)[0] == ext[0]
    assert np.array_equal(fr.raw_f12(a, override={(i, j): fr.components(row)[2 * i + j] for i in range(6) for j in range(2)}), row)


def test_record_layout():
    rng = random.Random(3)
    a, b = pc.rand_f12(rng), pc.rand_f12(rng)
    r = fr.record(fr.raw_f12(a), fr.raw_f12(b, 1))
    assert r.shape == (fr.REC_WORDS,) and r.dtype == np.uint32 and fr.residues(r[:108]) == a and fr.residues(r[108:]) == b
    assert not fr.record(fr.raw_f12(a))[108:].any()
    ww = fr.wire_words(a)
    ref = pc.gt_to_wire([a])[0].view(np.uint32).reshape(6, 2, 8)                       # uzk_gt's layout: 8 words a component
    assert np.array_equal(ww.reshape(6, 2, 9)[:, :, :8], ref) and not ww.reshape(6, 2, 9)[:, :, 8].any()
    assert np.array_equal(g2.fq2_to_wire(a[0]).view(np.uint32), np.concatenate([ww[0:8], ww[9:17]]))


def _step_case(rng):
    q = pc.h_multiples(3)[2]
    t = (q[0], q[1], (1, 0))
    for _ in range(3):
        t, _co = pr.dbl_step(t)
    s = (rng.randrange(1, P), rng.randrange(P))
    t = tuple(bp.f2_mul(c, s) for c in t)
    return t, q, 1, P - 2                                                            # P = the generator (1, 2): xP = 1, -yP = p - 2


def test_step_records_lie_in_their_types_and_round_trip():
    rng = random.Random(4)
    t, q, xp, nyp = _step_case(rng)
    for ks in (0, 1, [rng.randrange(2) for _ in range(10)]):
        for kb in ((0, 0), (3, 3), (1, 2)):
            row = fr.step_record(t, q, xp, nyp, ks, True, kb)
            assert fr.step_inputs_in_type(row)
            assert fr.residues(row[:90]) == list(t) + list(q)
            assert [fr.residue(l) for l in fr.components(row[90:])] == [xp, nyp]
            assert [lc.value(l) // P for l in fr.components(row[90:])] == list(kb)
    assert not fr.step_inputs_in_type(fr.step_record(t, q, xp, nyp, 0, False, (4, 0)))
    assert not fr.step_inputs_in_type(fr.step_record(t, q, xp, nyp, 2, False, (0, 0)))


def _model_outputs(rng):
    """correct raw outputs as the hooks would give them: an Fq12 product and a Miller step, every component a member of El"""
    a, b = pc.rand_f12(rng), pc.rand_f12(rng)
    want = pr.f12_mul(a, b)
    assert want == bp.f12_mul(a, b)
    t, q, xp, nyp = _step_case(rng)
    t3, co = pr.add_step(t, q)
    line = pr.line_at(co, (xp, (-nyp) % P))
    step = np.concatenate([fr.raw_f12(list(t3) + list(line), [rng.randrange(2) for _ in range(12)]), np.zeros(18, dtype=np.uint32)])
    return (fr.raw_f12(want, [rng.randrange(2) for _ in range(12)]), want), (step, t3, line)


def _over_limb(rng, i):
    """a limb vector of value below M whose low limb i is exactly 2^29 + 2^6 -- the first value outside K = 1 -- the others plain digits"""
    l = [rng.randrange(lc.B) for _ in range(8)] + [rng.randrange(1 << 20)]
    l[i] = lc.B + 64
    assert lc.value(l) < P and not lc.in_type(l, *fr.EL, P)
    return l


def _reject_three_ways(rng, check, row, want, comp):
    """`row` passes `check` against `want` (a list of Fq2 residues); component `comp` of it is then made wrong in the three ways a
    kernel's slip would show, and each must fail"""
    lo, c = 9 * comp, want[comp // 2][comp % 2]
    check(row, want)
    # the right residue, raised by M beyond 2 M
    bad = row.copy()
    bad[lo:lo + 9] = lc.limbs(fr.rep_value(c, 2))
    assert fr.residues(bad[:108]) == want
    with pytest.raises(AssertionError, match="outside Lz<1, 2>"):
        check(bad, want)
    # the right residue, a value below M, one low limb at 2^29 + 2^6: the reference is made to hold this vector's residue
    over = _over_limb(rng, comp % 8)
    want2 = [tuple(x) for x in want]
    want2[comp // 2] = tuple(fr.residue(over) if j == comp % 2 else want2[comp // 2][j] for j in range(2))
    good = row.copy()
    good[lo:lo + 9] = fr.rep_limbs(fr.residue(over), 0)
    check(good, want2)
    bad = good.copy()
    bad[lo:lo + 9] = over
    assert fr.residues(bad[:108]) == want2
    with pytest.raises(AssertionError, match="outside Lz<1, 2>"):
        check(bad, want2)
    # inside the type, the residue off by one
    bad = row.copy()
    bad[lo:lo + 9] = fr.rep_limbs((c + 1) % P, lc.value(fr.components(row)[comp]) // P)
    fr.check_types(bad[:108])
    with pytest.raises(AssertionError, match="residues differ"):
        check(bad, want)


def test_the_checkers_accept_correct_outputs_and_reject_wrong_ones():
    rng = random.Random(5)
    (row, want), (step, t3, line) = _model_outputs(rng)
    for comp in (0, 5, 11):
        _reject_three_ways(rng, fr.check, row, [tuple(c) for c in want], comp)
    step_want = [tuple(c) for c in list(t3) + list(line)]
    for comp in (1, 4, 6, 9, 10):                                                    # T3's coordinates and each of l0, l1, l3
        _reject_three_ways(rng, lambda r, w: fr.check_step(r, w[:3], w[3:]), step, step_want, comp)
    bad = step.copy()
    bad[125] = 1
    with pytest.raises(AssertionError, match="lanes of the group disagree"):
        fr.check_step(bad, t3, line)


def test_the_hooks_check_their_arguments_before_the_device():
    from uzkge_amd import _native as N, backend as b
    p = np.zeros(216, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p)
    E = N.UZK_ERR_PARAMETER
    for fn, top in ((N.lib.uzk_test_fq12_raw_kat, 12), (N.lib.uzk_test_miller_step_raw, 1)):
        assert fn(0, None, p, 1) == E and fn(0, p, None, 1) == E
        assert fn(top + 1, p, p, 1) == E and fn(-1, p, p, 1) == E
        assert fn(0, p, p, (1 << 20) + 1) == E
        if b.device_count() == 0:
            assert fn(0, p, p, 1) == N.UZK_ERR_DEVICE
