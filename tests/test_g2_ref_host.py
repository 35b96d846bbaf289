"""CPU side of the G2 MSM: the Groth16 fixture and its decompression, the Python reference (tests/g2_ref.py) against the naive oracle
sum and the frozen vectors, the library's host-side G2 code (uzk_g2_fold, uzk_g2_to_affine) against the reference, and the argument
checks of the new entry points, which come before anything touches a device."""
import ctypes
import hashlib
import os
import random
import struct

import numpy as np
import pytest

import bn254_pairing as bp
import bn254_py as opy
import g2_cases as gc
import g2_ref as g


@pytest.fixture(scope="module")
def cols():
    return g.load_fixture()


@pytest.fixture(scope="module")
def vec(golden_dir):
    return np.load(os.path.join(golden_dir, "vectors_g2.npz"))


def test_fixture_bytes_and_lengths():
    data = open(g.FIXTURE, "rb").read()
    assert len(data) == 467440 and hashlib.sha256(data).hexdigest() == g.FIXTURE_SHA256
    assert struct.unpack_from("<Q", data, 0)[0] == 4869 and struct.unpack_from("<Q", data, 8 + 32 * 4869)[0] == 4869
    readme = open(os.path.join(os.path.dirname(g.FIXTURE), "README_g2.md")).read()
    assert g.FIXTURE_SHA256 + "  groth16-reveal-b-queries.bin" in readme


def test_every_point_is_on_its_curve_and_the_column_is_degenerate(cols):
    g1, g2 = cols
    assert len(g1) == len(g2) == 4869
    assert all(p is None or (p[1] * p[1] - p[0] ** 3 - 3) % g.P == 0 for p in g1)
    assert all(g.g2_on_curve(q) for q in g2) and all(bp.g2_is_on_curve(q) for q in g2 if q is not None)
    fin = [q for q in g2 if q is not None]
    assert len(g2) - len(fin) == 775
    assert len(set(fin)) == 3838 and len(fin) - len(set(fin)) == 256
    dup, opp = gc.pair_classes(g2)
    assert len(dup) == 256 and len(opp) == 254
    assert sum(1 for q in set(fin) if g.g2_neg(q) in set(fin)) == 508
    off, n = gc.INF_RANGE
    assert all(q is None for q in g2[off:off + n])


def test_a_finite_point_has_order_r(cols):
    q = next(q for q in cols[1] if q is not None)
    assert bp.g2_mul(q, g.R) is None and bp.g2_mul(q, g.R - 1) == g.g2_neg(q)


def test_pairing_cross_relation_fixes_the_fq2_ordering(cols):
    """e(b_g1[i], b_g2[j]) = e(b_g1[j], b_g2[i]): only the root chosen by comparing c1 first, then c0, satisfies it"""
    g1, g2 = cols
    both = [i for i in range(len(g1)) if g1[i] is not None and g2[i] is not None]
    for i, j in ((both[0], both[1]), (both[2], both[40]), (both[7], both[900])):
        assert bp.pairing_product_is_one([(g1[i], g2[j]), (opy.g1_neg(g1[j]), g2[i])])


def test_pippenger_equals_the_naive_oracle_sum(cols):
    g2 = cols[1]
    rng = random.Random(11)
    idx = list(range(0, 40))
    s = [rng.randrange(g.R) for _ in idx]
    s[3], s[5] = 0, g.R - 1
    want = None
    for i, si in zip(idx, s):
        if g2[i] is not None:
            want = bp.g2_add(want, bp.g2_mul(g2[i], si))
    assert g.msm([g2[i] for i in idx], s) == want


def test_reference_reproduces_the_frozen_vectors(cols, vec):
    g2 = cols[1]
    for n in gc.SIZES:
        for cls in gc.CLASSES:
            assert np.array_equal(g.points_to_wire([g.msm(g2[:n], gc.scalars(cls, n))])[0], vec[f"msm_{cls}_{n}"]), (cls, n)
    dup, opp = gc.pair_classes(g2)
    assert np.array_equal(g.points_to_wire([g.msm(g2, gc.pair_scalars(4869, dup, 1))])[0], vec["msm_dup_pairs"])
    assert g.msm(g2, gc.pair_scalars(4869, opp, 2)) is None and not vec["msm_opp_pairs"].any()
    off, n = gc.OFFSET_CASE
    assert np.array_equal(g.points_to_wire([g.msm(g2[off:off + n], gc.scalars("uniform", n, seed=3))])[0], vec["msm_offset"])
    a, b = gc.fq2_operands()
    assert np.array_equal(np.stack([g.fq2_to_wire(x) for x in a]), vec["fq2_a"])
    for op in gc.FQ2_OPS:
        assert np.array_equal(np.stack([g.fq2_to_wire(x) for x in gc.fq2_expected(op, a, b)]), vec[f"fq2_op{op}"])
    a, b = gc.group_operands(g2)
    assert np.array_equal(g.points_to_wire(a), vec["grp_a"]) and np.array_equal(g.points_to_wire(b), vec["grp_b"])
    for op in gc.GROUP_OPS:
        assert np.array_equal(g.points_to_wire(gc.group_expected(op, a, b)), vec[f"grp_op{op}"])


def test_host_fold_and_to_affine_match_the_reference(cols):
    from uzkge_amd import backend as b
    fin = [q for q in cols[1] if q is not None][:8]
    rng = random.Random(5)
    parts, want = [], None
    for k, q in enumerate(fin):
        if k == 3:
            parts.append(g.jac_to_wire(((5, 7), (11, 13), (0, 0))))           # an infinite partial: z = 0, x and y arbitrary
            continue
        z = (rng.randrange(1, g.P), rng.randrange(g.P))                        # a non-trivial Jacobian representative
        z2 = g.f2_sqr(z)
        parts.append(g.jac_to_wire((g.f2_mul(q[0], z2), g.f2_mul(q[1], g.f2_mul(z2, z)), z)))
        want = bp.g2_add(want, q)
    folded = b.g2_fold(np.stack(parts))
    assert g.point_from_wire(b.g2_to_affine(folded)) == want
    p0, n0 = g.jac_to_wire((fin[0][0], fin[0][1], (1, 0))), g.jac_to_wire((fin[0][0], g.f2_neg(fin[0][1]), (1, 0)))
    assert g.point_from_wire(b.g2_to_affine(b.g2_fold(np.stack([p0, p0])))) == bp.g2_add(fin[0], fin[0])      # P + P
    assert not b.g2_to_affine(b.g2_fold(np.stack([p0, n0]))).any()                                             # P + (-P)
    inf = b.g2_fold(np.zeros((0, 24), dtype=np.uint64))
    assert np.array_equal(inf, g.jac_to_wire(None)) and not b.g2_to_affine(inf).any()
    assert np.array_equal(b.g2_to_affine(p0), g.points_to_wire([fin[0]])[0])                                  # canonical words


def test_entry_points_check_arguments_before_the_device_and_need_one():
    from uzkge_amd import UzkgeError, _native as N, backend as b
    z = np.zeros(128, dtype=np.uint64)                               # room for one record of any hook (the raw one: 147 words)
    p = z.ctypes.data_as(ctypes.c_void_p)
    h, n = ctypes.c_uint64(0), ctypes.c_size_t(0)
    E = N.UZK_ERR_PARAMETER
    assert N.lib.uzk_g2_register(p, 1, None) == E and N.lib.uzk_g2_register(None, 1, ctypes.byref(h)) == E
    for dead in (0, 12345, (1 << 59) | 999):
        assert N.lib.uzk_g2_release(dead) == E
        assert N.lib.uzk_g2_len(dead, ctypes.byref(n)) == E
        assert N.lib.uzk_msm_g2(dead, 0, p, 1, p) == E
        assert N.lib.uzk_msm_g2_batch(dead, 0, p, 1, 2, p) == E
        assert N.lib.uzk_msm_g2_batch_device(dead, 0, p, 1, 2, p) == E
    assert N.lib.uzk_g2_len(12345, None) == E
    assert N.lib.uzk_msm_g2(12345, 0, p, 1, None) == E and N.lib.uzk_msm_g2(12345, 0, None, 1, p) == E
    assert N.lib.uzk_msm_g2_batch(12345, 0, None, 1, 2, p) == E and N.lib.uzk_msm_g2_batch_device(12345, 0, p, 1, 2, None) == E
    assert N.lib.uzk_g2_fold(None, 1, p) == E and N.lib.uzk_g2_fold(p, 1, None) == E
    assert N.lib.uzk_g2_to_affine(None, p) == E and N.lib.uzk_g2_to_affine(p, None) == E
    assert N.lib.uzk_test_g2_kat(0, None, p, p, 1) == E and N.lib.uzk_test_g2_kat(7, p, p, p, 1) == E
    assert N.lib.uzk_test_g2_raw_kat(0, None, p, 1) == E and N.lib.uzk_test_g2_raw_kat(0, p, None, 1) == E
    assert N.lib.uzk_test_g2_raw_kat(5, p, p, 1) == E and N.lib.uzk_test_g2_raw_kat(-1, p, p, 1) == E
    if b.device_count() == 0:
        assert N.lib.uzk_g2_register(p, 1, ctypes.byref(h)) == N.UZK_ERR_DEVICE
        assert N.lib.uzk_test_g2_kat(0, p, p, p, 1) == N.UZK_ERR_DEVICE
        assert N.lib.uzk_test_g2_raw_kat(0, p, p, 1) == N.UZK_ERR_DEVICE
        with pytest.raises(UzkgeError) as e:
            b.G2Bases.from_host(np.zeros((2, 16), dtype=np.uint64))
        assert e.value.kind == "DeviceError"
