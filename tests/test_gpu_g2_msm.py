"""The G2 MSM (uzk_msm_g2*) over the b_g2_query column of the reference's Groth16 reveal key (tests/golden/groth16-reveal-b-queries.bin:
775 infinities, 256 duplicated points, 254 opposite pairs), against the frozen outputs of tests/golden/vectors_g2.npz.  Every
comparison is bit-exact on canonical affine words after uzk_g2_to_affine."""
import ctypes
import os

import numpy as np
import pytest

import bn254_pairing as bp
import bn254_py as opy
import g2_cases as gc
import g2_ref as g
import oracle_c as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vec(golden_dir):
    return np.load(os.path.join(golden_dir, "vectors_g2.npz"))


@pytest.fixture(scope="module")
def cols():
    return g.load_fixture()


@pytest.fixture(scope="module")
def wire(cols):
    return g.points_to_wire(cols[1])


@pytest.fixture(scope="module")
def bases(gpu, wire):
    b = gpu.G2Bases.from_host(wire)
    yield b
    b.release()


def _aff(gpu, jac):
    return gpu.g2_to_affine(jac)


@pytest.mark.parametrize("n", gc.SIZES)
def test_sizes_and_scalar_classes(gpu, bases, vec, n):
    """uniform, all zero, all one, all r - 1 (the top window and the digits' sign), boolean-heavy (fat buckets: runs cut into tasks)"""
    assert bases.len() == 4869
    for cls in gc.CLASSES:
        got = _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(gc.scalars(cls, n))))
        assert np.array_equal(got, vec[f"msm_{cls}_{n}"]), (cls, n)
    if n == 0:
        assert not vec["msm_uniform_0"].any()


def test_equal_scalars_on_duplicate_and_opposite_pairs(gpu, bases, vec, cols):
    """the doubling branch inside a bucket (256 points occur twice); p and -p with one scalar cancel to infinity (254 pairs)"""
    dup, opp = gc.pair_classes(cols[1])
    assert (len(dup), len(opp)) == (256, 254)
    got = _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(gc.pair_scalars(4869, dup, 1))))
    assert got.any() and np.array_equal(got, vec["msm_dup_pairs"])
    got = _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(gc.pair_scalars(4869, opp, 2))))
    assert not got.any() and not vec["msm_opp_pairs"].any()


def test_offsets_and_an_all_infinity_range(gpu, bases, vec, cols):
    from uzkge_amd import UzkgeError
    off, n = gc.OFFSET_CASE
    got = _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(gc.scalars("uniform", n, seed=3)), offset=off))
    assert np.array_equal(got, vec["msm_offset"])
    off, n = gc.INF_RANGE
    assert all(q is None for q in cols[1][off:off + n])
    assert not _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(gc.scalars("uniform", n, seed=4)), offset=off)).any()
    for off, n in ((4869, 1), (4000, 870), (4870, 0)):
        with pytest.raises(UzkgeError) as e:
            gpu.msm_g2(bases, np.zeros((n, 4), dtype=np.uint64), offset=off)
        assert e.value.kind == "DegreeError"
    assert not _aff(gpu, gpu.msm_g2(bases, np.zeros((0, 4), dtype=np.uint64), offset=4869)).any()      # the empty sum at the end is fine


@pytest.mark.parametrize("batch", (3, 8))
def test_batch_equals_the_single_calls(gpu, bases, vec, batch):
    """different vectors on the batch axis; the device-scalar entry point gives the same words as the host-scalar one"""
    s = np.stack([g.scalars_to_wire(gc.scalars("uniform", 4869, seed=10 + b)) for b in range(batch)])
    got = gpu.msm_g2_batch(bases, s)
    assert got.shape == (batch, 24)
    d = gpu.dev_alloc(s.nbytes)
    try:
        gpu.dev_upload(d, s)
        got_dev = gpu.msm_g2_batch_device(bases, d, 4869, batch)
    finally:
        gpu.dev_free(d)
    for b in range(batch):
        single = _aff(gpu, gpu.msm_g2(bases, s[b]))
        assert np.array_equal(_aff(gpu, got[b]), single), b
        assert np.array_equal(_aff(gpu, got_dev[b]), single), b
        assert np.array_equal(single, vec[f"msm_batch_{b}"]), b


def test_chunk_boundary_against_the_closed_form(gpu, cols):
    """n = 2^15 + 1 (two point chunks, the second of one point) over the bases (i + 1) H: the sum is (sum_i s_i (i + 1) mod r) H"""
    h = next(q for q in cols[1] if q is not None)
    n = (1 << 15) + 1
    pts, cur = [], None
    for _ in range(n):
        cur = bp.g2_add(cur, h)
        pts.append(cur)
    s = gc.scalars("uniform", n, seed=5)
    b = gpu.G2Bases.from_host(g.points_to_wire(pts))
    try:
        got = _aff(gpu, gpu.msm_g2(b, g.scalars_to_wire(s)))
    finally:
        b.release()
    k = sum(si * (i + 1) for i, si in enumerate(s)) % g.R
    assert np.array_equal(got, g.points_to_wire([bp.g2_mul(h, k)])[0])


def test_bilinearity_ties_the_g2_msm_to_the_g1_msm(gpu, bases, cols):
    """e(sum s_i b_g1[i], b_g2[j]) e(-b_g1[j], sum s_i b_g2[i]) = 1: both columns are the same scalars (the B polynomials at tau)
    times the two generators, so the check needs neither g2_ref's Pippenger nor the frozen vectors"""
    g1, g2 = cols
    j = next(i for i in range(len(g1)) if g1[i] is not None and g2[i] is not None)
    s = gc.scalars("uniform", 4869, seed=6)
    sw = g.scalars_to_wire(s)
    g1_wire = oc.points_from_affine(g1)
    lhs = oc.jac_to_affine_ints(gpu.msm_raw(g1_wire, sw))
    rhs = g.point_from_wire(_aff(gpu, gpu.msm_g2(bases, sw)))
    assert lhs is not None and rhs is not None
    assert bp.pairing_product_is_one([(lhs, g2[j]), (opy.g1_neg(g1[j]), rhs)])


def test_bases_of_a_second_context(gpu, wire, vec):
    """handles live under the context that made them: a G2Bases of a second context works there and dies with release"""
    from uzkge_amd import UzkgeError, _native as N
    from uzkge_amd.errors import check
    ctx = gpu.ctx_create_on(0)
    try:
        gpu.ctx_set_current(ctx)
        b = gpu.G2Bases.from_host(wire[:257])
        got = _aff(gpu, gpu.msm_g2(b, g.scalars_to_wire(gc.scalars("uniform", 257))))
        assert np.array_equal(got, vec["msm_uniform_257"])
        handle = b.handle
        b.release()
        n = ctypes.c_size_t(0)
        assert N.lib.uzk_g2_len(handle, ctypes.byref(n)) == N.UZK_ERR_PARAMETER
        out = np.zeros(24, dtype=np.uint64)
        assert N.lib.uzk_msm_g2(handle, 0, None, 0, out.ctypes.data_as(ctypes.c_void_p)) == N.UZK_ERR_PARAMETER
        with pytest.raises(UzkgeError):
            check(N.lib.uzk_g2_release(handle))
    finally:
        gpu.ctx_set_current(0)
        gpu.ctx_destroy(ctx)
