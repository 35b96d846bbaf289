"""The G2 MSM that ends on the device (uzk_msm_g2_batch_finish): chunk sums, the Horner chain over the 32 windows and the affine map as
kernels.  Bases are the chain (i + 1) H, so every sum has the closed form (sum_i s_i (i + 1) mod r) H in Python integers; every result
is also held against the affine of uzk_msm_g2_batch_device's sum (the host finish).  Bit-exact on canonical affine words."""
import ctypes

import numpy as np
import pytest

import bn254_pairing as bp
import g2_cases as gc
import g2_ref as g

pytestmark = pytest.mark.gpu

CHUNK = 1 << 15


@pytest.fixture(scope="module")
def chain():
    """(H, [(i + 1) H for i = 0 .. 2^15], their wire words), built once"""
    h = next(q for q in g.load_fixture()[1] if q is not None)
    pts, cur = [], None
    for _ in range(CHUNK + 1):
        cur = bp.g2_add(cur, h)
        pts.append(cur)
    return h, pts, g.points_to_wire(pts)


def _kh(h, k):
    """the wire words of (k mod r) H (zeros at infinity)"""
    k %= g.R
    return g.points_to_wire([bp.g2_mul(h, k) if k else None])[0]


def _closed(h, s, ks):
    return _kh(h, sum(si * ki for si, ki in zip(s, ks)))


def _run(gpu, wire, ss, outputs=("out",)):
    """ss: `batch` lists of n integer scalars over the n bases `wire`.  Returns the results [batch, 16] of uzk_msm_g2_batch_finish after
    checking them against the affine of uzk_msm_g2_batch_device's sums; with outputs naming "d_out" the device copy is checked too."""
    batch, n = len(ss), len(ss[0])
    sw = np.stack([g.scalars_to_wire(s) for s in ss]) if n else np.zeros((batch, 0, 4), dtype=np.uint64)
    bases = gpu.G2Bases.from_host(wire)
    d = gpu.dev_alloc(max(sw.nbytes, 32))
    d_out = gpu.dev_alloc(batch * 128)
    try:
        if sw.nbytes:
            gpu.dev_upload(d, sw)
        got = None
        if "out" in outputs and "d_out" in outputs:
            gpu.dev_upload(d_out, np.full((batch, 16), 0xdead, dtype=np.uint64))
            got = gpu.g2_msm_finish(bases, d, n, batch, d_out=d_out)
            assert np.array_equal(gpu.dev_download(d_out, (batch, 16)), got)
        if "out" in outputs:
            alone = gpu.g2_msm_finish(bases, d, n, batch)
            assert got is None or np.array_equal(alone, got)
            got = alone
        if "d_out" in outputs:
            gpu.dev_upload(d_out, np.full((batch, 16), 0xdead, dtype=np.uint64))
            assert gpu.g2_msm_finish(bases, d, n, batch, d_out=d_out, host=False) is None
            left = gpu.dev_download(d_out, (batch, 16))
            assert got is None or np.array_equal(left, got)
            got = left
        host = gpu.msm_g2_batch_device(bases, d, n, batch)
        for b in range(batch):
            assert np.array_equal(got[b], gpu.g2_to_affine(host[b])), b
    finally:
        gpu.dev_free(d)
        gpu.dev_free(d_out)
        bases.release()
    assert got.shape == (batch, 16)
    return got


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("n", (1, 7, 300))
def test_random_scalars(gpu, chain, n, batch):
    h, _, wire = chain
    ss = [gc.scalars("uniform", n, seed=40 + b) for b in range(batch)]
    got = _run(gpu, wire[:n], ss, outputs=("out", "d_out"))
    for b in range(batch):
        want = _closed(h, ss[b], range(1, n + 1))
        assert want.any() and np.array_equal(got[b], want), b


def test_zero_scalars_top_window_and_r_minus_one(gpu, chain):
    """all-zero scalars: affine zeros.  One scalar of 2^248: only the top window is set, 248 doublings follow.  Scalars r - 1."""
    h, _, wire = chain
    n = 7
    ss = [[0] * n, [1 << 248] + [0] * (n - 1), [g.R - 1] * n, [0] * (n - 1) + [1 << 248]]
    got = _run(gpu, wire[:n], ss, outputs=("out", "d_out"))
    assert not got[0].any()
    for b in range(1, 4):
        want = _closed(h, ss[b], range(1, n + 1))
        assert want.any() and np.array_equal(got[b], want), b
    assert np.array_equal(got[1], _kh(h, 1 << 248))


def test_the_horner_addition_doubles_and_cancels(gpu, chain):
    """Bases H, 256 H and a third point with scalars 2^248, 2^240: window 31 holds H and window 30 holds 256 H, so after eight doublings
    the running total EQUALS the next window's sum and the addition must double.  With -256 H in its place the total passes through
    infinity; the third base's low scalar, added afterwards to an infinite accumulator, must come through unchanged."""
    h, pts, _ = chain
    p256 = pts[255]
    assert p256 == bp.g2_mul(h, 256)
    third, low = pts[4], 0x1234
    wire_dbl = g.points_to_wire([h, p256, third])
    wire_can = g.points_to_wire([h, g.g2_neg(p256), third])
    s0 = [1 << 248, 1 << 240, 0]
    s1 = [1 << 248, 1 << 240, low]
    got = _run(gpu, wire_dbl, [s0, s1])
    assert np.array_equal(got[0], _kh(h, 2 << 248)) and got[0].any()
    assert np.array_equal(got[1], _kh(h, (2 << 248) + 5 * low))
    got = _run(gpu, wire_can, [s0, s1], outputs=("out", "d_out"))
    assert not got[0].any()                                            # O
    assert np.array_equal(got[1], _kh(h, 5 * low)) and got[1].any()


def test_point_chunks_are_summed_on_the_device(gpu, chain):
    """n = 2^15 + 1, batch 2: every vector runs two point chunks, the second of one point, and g2_chunk_sum adds their window sums"""
    h, _, wire = chain
    n = CHUNK + 1
    ss = [gc.scalars("uniform", n, seed=7 + b) for b in range(2)]
    got = _run(gpu, wire, ss)
    for b in range(2):
        assert np.array_equal(got[b], _closed(h, ss[b], range(1, n + 1))), b


def test_a_second_group_of_vectors(gpu, chain):
    """batch 129 at n = 7: the second group holds one vector"""
    h, _, wire = chain
    n, batch = 7, 129
    ss = [gc.scalars("uniform", n, seed=200 + b) for b in range(batch)]
    got = _run(gpu, wire[:n], ss, outputs=("out", "d_out"))
    for b in (0, 63, 64, 127, 128):
        want = _closed(h, ss[b], range(1, n + 1))
        assert want.any() and np.array_equal(got[b], want), b


def test_refusals_and_the_empty_sum(gpu, chain):
    """both outputs NULL is UZK_ERR_PARAMETER; offset + n beyond the bases is UZK_ERR_DEGREE; n = 0 is infinity"""
    from uzkge_amd import UzkgeError, _native as N
    _, _, wire = chain
    bases = gpu.G2Bases.from_host(wire[:7])
    d = gpu.dev_alloc(7 * 32)
    try:
        gpu.dev_upload(d, g.scalars_to_wire([1] * 7))
        assert N.lib.uzk_msm_g2_batch_finish(bases.handle, 0, ctypes.c_void_p(d), 7, 1, None, None) == N.UZK_ERR_PARAMETER
        with pytest.raises(UzkgeError) as e:
            gpu.g2_msm_finish(bases, d, 7, 1, offset=1)
        assert e.value.kind == "DegreeError"
        assert not gpu.g2_msm_finish(bases, d, 0, 2, offset=7).any()
    finally:
        gpu.dev_free(d)
        bases.release()
