"""The G2 MSM (uzk_msm_g2*) over the b_g2_query column of the reference's Groth16 reveal key (tests/golden/groth16-reveal-b-queries.bin:
775 infinities, 256 duplicated points, 254 opposite pairs), against the frozen outputs of tests/golden/vectors_g2.npz, and over the
chain (i + 1) H, whose sums have a closed form that owes nothing to the library: the second group of a batch above 128 vectors, point
chunks under a batch, equal and opposite chunks (the host's doubling and cancellation), a whole chunk in one bucket, and scalars of
extreme digits.  Every comparison is bit-exact on canonical affine words after uzk_g2_to_affine."""
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


CHUNK = 1 << 15


@pytest.fixture(scope="module")
def chain(cols):
    """(H, [(i + 1) H for i = 0 .. 2^15], their wire words): bases whose MSM has the closed form (sum_i s_i (i + 1) mod r) H, built once"""
    h = next(q for q in cols[1] if q is not None)
    pts, cur = [], None
    for _ in range(CHUNK + 1):
        cur = bp.g2_add(cur, h)
        pts.append(cur)
    return h, pts, g.points_to_wire(pts)


def _closed(h, s, ks):
    """the wire words of (sum_i s_i k_i mod r) H (zeros at infinity)"""
    k = sum(si * ki for si, ki in zip(s, ks)) % g.R
    return g.points_to_wire([bp.g2_mul(h, k) if k else None])[0]


def test_chunk_boundary_against_the_closed_form(gpu, chain):
    """n = 2^15 + 1 (two point chunks, the second of one point) over the bases (i + 1) H: the sum is (sum_i s_i (i + 1) mod r) H"""
    h, pts, wire = chain
    n = CHUNK + 1
    s = gc.scalars("uniform", n, seed=5)
    b = gpu.G2Bases.from_host(wire)
    try:
        got = _aff(gpu, gpu.msm_g2(b, g.scalars_to_wire(s)))
    finally:
        b.release()
    k = sum(si * (i + 1) for i, si in enumerate(s)) % g.R
    assert np.array_equal(got, g.points_to_wire([bp.g2_mul(h, k)])[0])


def test_a_second_group_of_vectors(gpu, chain):
    """batch = 129 over 33 bases: g2_msm_run's loop over groups of 128 vectors runs a second group (b0 = 128) of one vector; vectors 0,
    127 and 128 equal their single calls and the closed form"""
    h, _, wire = chain
    n, batch = 33, 129
    ss = [gc.scalars("uniform", n, seed=100 + b) for b in range(batch)]
    bases = gpu.G2Bases.from_host(wire[:n])
    try:
        got = gpu.msm_g2_batch(bases, np.stack([g.scalars_to_wire(s) for s in ss]))
        assert got.shape == (batch, 24)
        for b in (0, 127, 128):
            want = _closed(h, ss[b], range(1, n + 1))
            assert want.any()
            assert np.array_equal(_aff(gpu, got[b]), want), b
            assert np.array_equal(_aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(ss[b]))), want), b
    finally:
        bases.release()


def test_point_chunks_of_a_batch(gpu, chain):
    """batch = 2 with n = 2^15 + 1: every vector runs its own point chunks (scalars of a vector are n apart, the second chunk starts at
    an odd offset into them)"""
    h, _, wire = chain
    n = CHUNK + 1
    ss = [gc.scalars("uniform", n, seed=7 + b) for b in range(2)]
    bases = gpu.G2Bases.from_host(wire)
    try:
        got = gpu.msm_g2_batch(bases, np.stack([g.scalars_to_wire(s) for s in ss]))
    finally:
        bases.release()
    for b in range(2):
        assert np.array_equal(_aff(gpu, got[b]), _closed(h, ss[b], range(1, n + 1))), b


def test_equal_chunks_double_and_opposite_chunks_cancel_on_the_host(gpu, chain):
    """n = 2^16 with the second chunk a copy of the first, bases and scalars alike: each of the 32 window sums of chunk two equals chunk
    one's, so the host's j2_add takes its doubling branch 32 times; with the second chunk's bases negated all 32 sums cancel and the
    result is infinity"""
    h, pts, wire = chain
    s = gc.scalars("uniform", CHUNK, seed=8)
    sw = g.scalars_to_wire(s)
    sw2 = np.concatenate([sw, sw])
    for second, want in ((wire[:CHUNK], _closed(h, [2 * si for si in s], range(1, CHUNK + 1))),
                         (g.points_to_wire([g.g2_neg(q) for q in pts[:CHUNK]]), np.zeros(16, dtype=np.uint64))):
        bases = gpu.G2Bases.from_host(np.concatenate([wire[:CHUNK], second]))
        try:
            got = _aff(gpu, gpu.msm_g2(bases, sw2))
        finally:
            bases.release()
        assert np.array_equal(got, want)
    assert _closed(h, [2 * si for si in s], range(1, CHUNK + 1)).any()


@pytest.mark.parametrize("s", (1, 128))
def test_one_bucket_holds_a_whole_chunk(gpu, chain, s):
    """n = 2^15 with all scalars equal: one bucket holds every point -- 1024 tasks, run offsets up to 32767 in the 16-bit field of a task;
    s = 128 makes window 0's digit -128 (bucket 128, the top bucket of the last segment, every point negated) with the carry as
    window 1's digit 1"""
    h, _, wire = chain
    bases = gpu.G2Bases.from_host(wire[:CHUNK])
    try:
        got = _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire([s] * CHUNK)))
    finally:
        bases.release()
    want = g.points_to_wire([bp.g2_mul(h, s * (CHUNK * (CHUNK + 1) // 2) % g.R)])[0]
    assert np.array_equal(got, want)


def test_digit_extremes(gpu, chain):
    """257 scalars whose every byte is one of 0x00, 0x7f, 0x80, 0xff (the top byte 0x00 or 0x2f, below r's 0x30): the signed digits 0,
    127, -128 and -1, and the carries of the last two rippling through all 32 windows"""
    import random
    h, _, wire = chain
    n = 257
    rng = random.Random("g2-digit-extremes")
    s = [int.from_bytes(bytes([rng.choice((0x00, 0x7f, 0x80, 0xff)) for _ in range(31)] + [rng.choice((0x00, 0x2f))]), "little") for _ in range(n)]
    s[0] = int.from_bytes(bytes([0x80] * 31 + [0x2f]), "little")          # -128 in every window below the top one
    s[1] = int.from_bytes(bytes([0xff] * 31 + [0x2f]), "little")          # -1 and a carry in every window
    s[2] = int.from_bytes(bytes([0x7f] * 31 + [0x00]), "little")          # 127 everywhere, no carry
    s[3] = int.from_bytes(bytes([0x80] + [0x7f] * 30 + [0x00]), "little")  # one carry that turns every 127 above it into -128
    assert all(0 < x < g.R for x in s)
    bases = gpu.G2Bases.from_host(wire[:n])
    try:
        got = _aff(gpu, gpu.msm_g2(bases, g.scalars_to_wire(s)))
    finally:
        bases.release()
    want = _closed(h, s, range(1, n + 1))
    assert want.any() and np.array_equal(got, want)


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
