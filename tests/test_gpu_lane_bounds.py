"""The prover's lane kernels (rounds.hip) driven to the limits their unchecked bounds rest on (uzk_test_lanes).  The lazy 29-bit
linear combination's running sum is bounded only by the host's gate count <= 128 (kLincomb29Max); the evaluation tree's LDS sums
only by the block size.  With every scalar, coefficient and point the WIRE words of r - 1 (raw words, not to_mont(r - 1): that
maximises the re-limbed 32 a each pair adds), the sums reach their stated limits; the results must equal the oracle, and the hook
reports which kernel ran from the launcher's own choice."""
import ctypes

import numpy as np
import pytest

import bn254_py as opy

pytestmark = pytest.mark.gpu

R = opy.R
RINV = pow(1 << 256, -1, R)
RM1 = np.asarray(opy.int_to_limbs(R - 1), dtype=np.uint64)       # the words of r - 1


def _w(x):
    return np.asarray(opy.int_to_limbs(x % R), dtype=np.uint64)


def _int(w):
    return opy.limbs_to_int([int(v) for v in w])


def _lanes(gpu, op, bufs, strides, count, lens, pts, args, lanes, length):
    from uzkge_amd import _native as N
    ptrs = (ctypes.c_void_p * count)(*bufs)
    st = np.ascontiguousarray(strides, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint32)
    pt = np.ascontiguousarray(pts if pts is not None else np.zeros(count), dtype=np.uint32)
    ar = np.ascontiguousarray(args, dtype=np.uint64)
    n_out = lanes * length if op == 0 else lanes * count
    out = np.zeros((n_out, 4), dtype=np.uint64)
    kern = ctypes.c_int(-1)
    rc = N.lib.uzk_test_lanes(op, ptrs, st.ctypes.data_as(ctypes.c_void_p), count, ln.ctypes.data_as(ctypes.c_void_p),
                              pt.ctypes.data_as(ctypes.c_void_p), ar.ctypes.data_as(ctypes.c_void_p), lanes, length,
                              out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(kern))
    return rc, out, kern.value


@pytest.fixture
def a29(gpu):
    yield gpu
    gpu.tune("arith29", 7)


@pytest.mark.parametrize("arith29", [2, 0])
@pytest.mark.parametrize("count", [1, 7, 8, 127, 128, 129])
@pytest.mark.parametrize("long_out", [False, True])
def test_lincomb_lanes_at_the_term_limit(a29, arith29, count, long_out):
    """out_len on either side of 2^17 picks GS = 4 or 1 (count >= 8); lanes = 1 and 3; uneven lengths including 0.  Coefficients and
    scalars are all r - 1 words, so out_j = (number of terms with j < len) (r - 1)^2 / 2^256 mod r."""
    gpu = a29
    gpu.tune("arith29", arith29)
    out_len = (1 << 17) + 5 if long_out else 1000
    for lanes in (1, 3):
        rng = np.random.default_rng(count * 10 + lanes)
        buf_len = out_len + 64
        d = gpu.dev_alloc(buf_len * 32 * lanes)
        try:
            gpu.dev_upload(d, np.tile(RM1, (buf_len * lanes, 1)))
            lens = rng.integers(0, out_len + 1, size=(lanes, count))
            lens[:, 0] = out_len                                 # the full length, then uneven ones and 0
            if count > 2:
                lens[:, 1] = 0
            strides = [buf_len if k % 2 else 0 for k in range(count)]   # some polynomials per lane, some shared by the lanes
            bufs = [d + 32 * (k % 7) for k in range(count)]
            lens = np.minimum(lens, buf_len - 7)
            args = np.tile(RM1, (lanes * count, 1))
            rc, out, kern = _lanes(gpu, 0, bufs, strides, count, lens, None, args, lanes, out_len)
            assert rc == 0
            want29 = bool(arith29 & 2) and count <= 128
            assert kern == (1 if want29 else 0) | (2 if (out_len <= 1 << 17 and count >= 8) else 0), kern
            unit = (R - 1) * (R - 1) * RINV % R
            table = np.stack([_w(c * unit) for c in range(count + 1)])
            j = np.arange(out_len)
            for b in range(lanes):
                cnt = (j[:, None] < lens[b][None, :]).sum(axis=1)
                assert np.array_equal(out[b * out_len:(b + 1) * out_len], table[cnt]), (lanes, b)
        finally:
            gpu.dev_free(d)


def test_lincomb_lanes_random_terms_match_the_oracle(a29):
    """Random scalars and coefficients mixed with r - 1 words at count = 128 (the 29-bit kernel's limit), GS = 4 and GS = 1."""
    gpu = a29
    gpu.tune("arith29", 7)
    rng = np.random.default_rng(5)
    count, lanes = 128, 3
    for out_len in (40, (1 << 17) + 1):
        n_chk = 40
        buf = np.tile(RM1, (out_len + count, 1))                 # polynomial k is buf[k : k + out_len]
        for i in range(n_chk + count):
            if rng.random() < 0.5:
                buf[i] = _w(int(rng.integers(0, 1 << 62)) ** 4)
        bi = [_int(w) for w in buf[:n_chk + count]]
        d = gpu.dev_alloc(buf.nbytes)
        try:
            gpu.dev_upload(d, buf)
            bufs = [d + 32 * k for k in range(count)]
            lens = np.full((lanes, count), out_len)
            lens[1, ::3] = 17
            scal = np.array([_w(int(rng.integers(1, 1 << 62)) ** 4) if rng.random() < 0.5 else RM1 for _ in range(lanes * count)])
            rc, out, kern = _lanes(gpu, 0, bufs, [0] * count, count, lens, None, scal, lanes, out_len)
            assert rc == 0 and kern & 1
            for b in range(lanes):
                for j in range(n_chk):
                    acc = sum(_int(scal[b * count + k]) * bi[k + j] for k in range(count) if j < lens[b, k])
                    assert _int(out[b * out_len + j]) == acc * RINV % R, (out_len, b, j)
        finally:
            gpu.dev_free(d)


def _eval_oracle(coefs_int, x_int, n):
    """Wire value of p(x) for n coefficients (wire ints) at the wire point x: Horner on the Montgomery words."""
    xs = x_int * RINV % R
    acc = 0
    for c in reversed(coefs_int[:n]):
        acc = (acc * xs + c) % R
    return acc


@pytest.mark.parametrize("arith29", [2, 0])
@pytest.mark.parametrize("lanes", [2, 4])
def test_eval_lanes_at_the_block_limit(a29, arith29, lanes):
    """max_len 2^18 (the largest the launcher takes; 2^18 + 1 is refused), the narrow (lanes < 4) and the wide (PER = 16) kernel,
    lengths off the block size, 0 and 1; coefficients and points the words of r - 1."""
    gpu = a29
    gpu.tune("arith29", arith29)
    max_len = 1 << 18
    lens = [max_len, 0, 1, 4097, 1023, max_len - 1]
    pts = [0, 1, 1, 0, 1, 0]
    count = len(lens)
    coefs = np.tile(RM1, (max_len, 1))
    rng = np.random.default_rng(lanes)
    coefs[:300] = [_w(int(rng.integers(0, 1 << 62)) ** 4) for _ in range(300)]
    d = gpu.dev_alloc(coefs.nbytes)
    try:
        gpu.dev_upload(d, coefs)
        points = np.tile(RM1, (2 * lanes, 1))
        points[3] = _w(123456789)
        rc, out, kern = _lanes(gpu, 1, [d] * count, [0] * count, count, lens, pts, points, lanes, max_len)
        assert rc == 0
        assert kern == (1 if arith29 & 2 else 0) | (2 if lanes >= 4 else 0), kern
        ci = [_int(c) for c in coefs]
        cache = {}
        for b in range(lanes):
            for k in range(count):
                x = _int(points[2 * b + pts[k]])
                key = (x, lens[k])
                if key not in cache:
                    cache[key] = _eval_oracle(ci, x, lens[k])
                assert _int(out[b * count + k]) == cache[key], (b, k)
        rc, _, _ = _lanes(gpu, 1, [d], [0], 1, [5], [0], points, lanes, max_len + 1)
        assert rc != 0, "max_len 2^18 + 1 must be refused"
    finally:
        gpu.dev_free(d)
