"""The G1 transform's host side, without a GPU: the SRS blob writer against the reference's own files, the size bound, the return
codes of every new entry point, and the test helper (tests/g1_ntt_ref.py) against the oracle's definition."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
import g1_ntt_ref as ref
from util import GOLDEN, rand_fr_wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRS_FILES = ("lagrange-srs-4096.bin", "lagrange-srs-8192.bin", "lagrange-srs-16384.bin", "srs-padding.bin")


def _bound():
    hdr = open(os.path.join(ROOT, "include", "uzkge_gpu.h")).read()
    return int(re.search(r"#define UZK_NTT_G1_MAX_LOG2 (\d+)", hdr).group(1))


@pytest.mark.parametrize("name", SRS_FILES)
def test_writer_reproduces_the_reference_files(name):
    """srs_g1_wire_to_bytes is the inverse of parse_srs_g1_wire on the four blobs the reference ships, byte for byte (the G2
    block passes through)."""
    from uzkge_amd.poly_commit import parse_srs_g1_wire, srs_g1_wire_to_bytes
    f = open(os.path.join(GOLDEN, name), "rb").read()
    len1, len2 = struct.unpack_from("<II", f, 0)
    assert srs_g1_wire_to_bytes(parse_srs_g1_wire(f), len2, f[8 + 64 * len1:]) == f


def test_writer_flags_infinity_and_the_sign_of_y():
    """None of the shipped files holds infinity: a hand-made vector covers it (zero coordinates, bit 6 of the last byte) together
    with both signs of y (bit 7 set when y > (p - 1) / 2)."""
    from uzkge_amd.poly_commit import parse_srs_g1_wire, srs_g1_wire_to_bytes
    g = opy.G1_GEN
    pts = [g, opy.g1_neg(g), None, opy.g1_mul(g, 7), opy.g1_neg(opy.g1_mul(g, 7))]
    blob = bytearray(struct.pack("<II", len(pts), 0))
    for p in pts:
        if p is None:
            blob += bytes(63) + b"\x40"
            continue
        yb = bytearray(p[1].to_bytes(32, "little"))
        if p[1] > (opy.P - 1) // 2:
            yb[31] |= 0x80
        blob += p[0].to_bytes(32, "little") + bytes(yb)
    signs = [blob[8 + 64 * i + 63] >> 7 for i in (0, 1, 3, 4)]
    assert sorted(signs[:2]) == [0, 1] and sorted(signs[2:]) == [0, 1]
    wire = parse_srs_g1_wire(bytes(blob))
    assert np.array_equal(wire, oc.points_from_affine(pts)) and not wire[2].any()
    assert srs_g1_wire_to_bytes(wire) == bytes(blob)
    assert srs_g1_wire_to_bytes(wire, 2, b"g2 block") == bytes(blob[:4]) + struct.pack("<I", 2) + bytes(blob[8:]) + b"g2 block"


def test_supported_sizes_and_the_bound_is_the_tested_bound():
    """2^k up to UZK_NTT_G1_MAX_LOG2, nothing else; the bound is the largest size tests/test_gpu_g1_ntt.py checks on the whole
    vector -- a size is accepted only if its result is checked."""
    from uzkge_amd import backend as b
    import test_gpu_g1_ntt as g
    k = _bound()
    for n in (1, 2, 1 << 14, 1 << k):
        assert b.ntt_g1_supported(n), n
    for n in (0, 3, 48, 98304, 1 << (k + 1)):
        assert not b.ntt_g1_supported(n), n
    assert max(g.LARGE_LOG2) == k == g.MAX_LOG2


def test_return_codes_before_the_device():
    """Argument checks come before the device is touched: bad sizes are FFTError, null pointers and unknown handles
    ParameterError, with or without a GPU; without one a well-formed call is DeviceError (no CPU fallback)."""
    from uzkge_amd import UzkgeError, _native as N, backend as b
    k = _bound()
    a = np.zeros((4, 8), dtype=np.uint64)
    p = a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_uint64(0)
    for bad in (0, 3, 48, 98304, 1 << (k + 1)):
        assert N.lib.uzk_ntt_g1(p, p, bad, 0) == N.UZK_ERR_FFT, bad
        assert N.lib.uzk_ntt_g1_device(p, p, bad, 1, 1) == N.UZK_ERR_FFT, bad
        assert N.lib.uzk_srs_to_lagrange(12345, bad, ctypes.byref(h)) == N.UZK_ERR_FFT, bad
        assert N.lib.uzk_ntt_g1_plan_info(bad, 0, ctypes.byref(h), ctypes.byref(h)) == N.UZK_ERR_FFT, bad
    assert N.lib.uzk_ntt_g1(None, p, 4, 0) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_ntt_g1(p, None, 4, 0) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_ntt_g1_device(None, p, 4, 0, 1) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_ntt_g1_device(p, None, 4, 0, 1) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_to_lagrange(12345, 4, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_to_lagrange(12345, 4, ctypes.byref(h)) == N.UZK_ERR_PARAMETER          # unknown handle
    assert N.lib.uzk_srs_download(12345, 0, 4, p) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_download(12345, 0, 4, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_ntt_g1_plan_info(4, 0, None, ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    with pytest.raises(UzkgeError) as e:
        b.ntt_g1(np.zeros((48, 8), dtype=np.uint64))
    assert e.value.kind == "FFTError"
    with pytest.raises(UzkgeError) as e:
        b.Srs(12345, 4).to_lagrange(4)
    assert e.value.kind == "ParameterError"
    if b.device_count() == 0:
        with pytest.raises(UzkgeError) as e:
            b.ntt_g1(a)
        assert e.value.kind == "DeviceError"
        assert N.lib.uzk_ntt_g1_device(p, p, 4, 0, 1) == N.UZK_ERR_DEVICE


def test_plan_counts_the_group_operations():
    """(n / 2) log2 n butterflies, of which those with twiddle 1 (t = 0 of every block) skip the scalar multiplication; a
    multiplication is 256 doublings and 67 additions (4-bit signed windows and their table), a butterfly two more additions; the
    inverse multiplies every point once more."""
    from uzkge_amd import backend as b
    for k in (1, 3, 12):
        n = 1 << k
        muls = sum(n // 2 - (n >> (s + 1)) for s in range(k))
        assert b.ntt_g1_plan_info(n) == (256 * muls, 67 * muls + k * n)
        assert b.ntt_g1_plan_info(n, inverse=True) == (256 * (muls + n), 67 * (muls + n) + k * n)


def test_helper_against_the_definition():
    """tests/g1_ntt_ref.py at n = 8: the recursive transform equals the DFT row by row with the pure-Python oracle's naive MSM, in
    both directions; inputs include infinity and a repeated point; the symmetric-matrix check accepts the right answer and
    rejects a wrong one."""
    g = opy.G1_GEN
    pts = [opy.g1_mul(g, 3), None, opy.g1_mul(g, 5), opy.g1_mul(g, 5), g, opy.g1_neg(g), opy.g1_mul(g, 11), None]
    wire = oc.points_from_affine(pts)
    w = opy.root_of_unity(8)
    for inverse in (False, True):
        got = ref.g1_ntt(wire, inverse)
        assert np.array_equal(got, ref.g1_ntt_rows(wire, inverse))
        ww = pow(w, -1, opy.R) if inverse else w
        s = pow(8, -1, opy.R) if inverse else 1
        for k in range(8):
            want = opy.msm_naive(pts, [s * pow(ww, i * k, opy.R) % opy.R for i in range(8)])
            assert opy.wire_to_affine(got[k].tobytes()) == want, (inverse, k)
        c = rand_fr_wire(8, 5)
        assert ref.symmetric_ok(wire, got, c, inverse)
        bad = got.copy(); bad[[2, 3]] = bad[[3, 2]]
        assert not ref.symmetric_ok(wire, bad, c, inverse)
    assert np.array_equal(ref.g1_ntt(ref.g1_ntt(wire), inverse=True), wire)
    m, pw = ref.tau_powers(12345, 8)
    lag = opy.ntt(pw, 8, inverse=True)
    assert [opy.wire_to_affine(r.tobytes()) for r in ref.g1_ntt(m, inverse=True)] == [opy.g1_mul(g, x) for x in lag]
