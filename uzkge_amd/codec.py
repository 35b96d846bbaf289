"""The point codec: ark-serialize's compressed G1, G2 and Baby Jubjub points decoded and encoded on the device (include/uzkge_gpu.h,
"the point codec"), and the layout of a compressed Groth16 proving key.

Encodings go in as bytes (n x 32 or n x 64, concatenated) or as uint8 arrays; points come out as wire arrays -- G1 [n, 8], G2 [n, 16]
(x.c0 x.c1 y.c0 y.c1), Baby Jubjub [n, 8] (x then y), canonical Montgomery words -- with one status byte each: 0 accepted, 1 not a
canonical encoding, 2 no point, 3 outside the prime-order subgroup (only when asked).  A point whose status is not 0, and an accepted
infinity, is all zeros."""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np

from . import _native as N
from .errors import UzkgeError, check

lib = N.lib
G1_BYTES, G2_BYTES, ED_BYTES = 32, 64, 32


def _vp(a: np.ndarray) -> ctypes.c_void_p:
    return a.ctypes.data_as(ctypes.c_void_p)


def _encodings(data, width: int) -> np.ndarray:
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if raw.size == 0 or raw.size % width:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "a whole number (at least one) of %d-byte encodings" % width)
    return raw


def _decompress(fn, data, width: int, words: int, *flags) -> Tuple[np.ndarray, np.ndarray]:
    raw = _encodings(data, width)
    n = raw.size // width
    out, status = np.zeros((n, words), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    check(fn(_vp(raw), n, *flags, _vp(out), _vp(status)))
    return out, status


def _compress(fn, points, width: int, words: int) -> Tuple[np.ndarray, np.ndarray]:
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
    n = p.shape[0]
    out, status = np.zeros((max(n, 1), width), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    check(fn(_vp(p) if n else None, n, _vp(out), _vp(status)))
    return out[:n], status[:n]


def g1_decompress(data) -> Tuple[np.ndarray, np.ndarray]:
    """uzk_g1_decompress_batch: (points [n, 8], status [n])"""
    return _decompress(lib.uzk_g1_decompress_batch, data, G1_BYTES, 8)


def g2_decompress(data, check_subgroup: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """uzk_g2_decompress_batch: (points [n, 16], status [n]); with check_subgroup also [r] Q = O (status 3)"""
    return _decompress(lib.uzk_g2_decompress_batch, data, G2_BYTES, 16, int(bool(check_subgroup)))


def ed_decompress(data, check_subgroup: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """uzk_ed_decompress_batch: (points [n, 8], status [n]); with check_subgroup also [L] P = identity (status 3)"""
    return _decompress(lib.uzk_ed_decompress_batch, data, ED_BYTES, 8, int(bool(check_subgroup)))


def g1_compress(points) -> Tuple[np.ndarray, np.ndarray]:
    """uzk_g1_compress_batch: (encodings [n, 32] uint8, status [n]: 1 a coordinate word not below p)"""
    return _compress(lib.uzk_g1_compress_batch, points, G1_BYTES, 8)


def g2_compress(points) -> Tuple[np.ndarray, np.ndarray]:
    return _compress(lib.uzk_g2_compress_batch, points, G2_BYTES, 16)


def ed_compress(points) -> Tuple[np.ndarray, np.ndarray]:
    return _compress(lib.uzk_ed_compress_batch, points, ED_BYTES, 8)


def g16_pk_layout(data: bytes) -> dict:
    """uzk_g16_pk_layout (host only): section name -> (offset, count, infinities) of a compressed ProvingKey<Bn254>."""
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    s = N.G16PkSections()
    check(lib.uzk_g16_pk_layout(_vp(raw) if raw.size else ctypes.c_void_p(ctypes.addressof(s)), raw.size, ctypes.byref(s)))
    return {name: (int(s.offset[k]), int(s.count[k]), int(s.infinities[k])) for k, name in enumerate(N.PK_SECTION_NAMES)}


def srs_register_compressed(data) -> int:
    """uzk_srs_register_compressed: the handle of n compressed G1 points decoded into device memory (for backend.Srs(handle, n))."""
    raw = _encodings(data, G1_BYTES)
    h = ctypes.c_uint64(0)
    check(lib.uzk_srs_register_compressed(_vp(raw), raw.size // G1_BYTES, ctypes.byref(h)))
    return h.value


def g2_register_compressed(data, check_subgroup: bool = False) -> int:
    """uzk_g2_register_compressed: the handle of n compressed G2 points (for backend.G2Bases(handle, n))."""
    raw = _encodings(data, G2_BYTES)
    h = ctypes.c_uint64(0)
    check(lib.uzk_g2_register_compressed(_vp(raw), raw.size // G2_BYTES, int(bool(check_subgroup)), ctypes.byref(h)))
    return h.value


def sqrt_kat(field: int, a) -> Tuple[np.ndarray, np.ndarray]:
    """uzk_test_sqrt_kat (test hook): field 0 Fq [n, 4], 1 Fq2 [n, 8], 2 Fr [n, 4]; returns (roots, is_square [n])"""
    words = 8 if field == 1 else 4
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, words)
    root, ok = np.zeros_like(x), np.zeros(x.shape[0], dtype=np.uint8)
    check(lib.uzk_test_sqrt_kat(field, _vp(x), x.shape[0], _vp(root), _vp(ok)))
    return root, ok
