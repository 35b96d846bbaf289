"""Thin numpy-facing wrappers over the C ABI.  Field elements travel as uint64 arrays in the wire
format of include/uzkge_gpu.h (Montgomery, 4 LE limbs): scalars [n,4], affine points [n,8],
Jacobian results [12]."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as N
from .errors import check

lib = N.lib


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need C-contiguous uint64"
    return a.ctypes.data_as(ctypes.c_void_p)


def init(device: int = 0) -> None:
    check(lib.uzk_init(device))


def shutdown() -> None:
    check(lib.uzk_shutdown())


def device_count() -> int:
    return lib.uzk_device_count()


def sync() -> None:
    check(lib.uzk_sync())


def ctx_create() -> int:
    """A new context (stream + workspaces + lock) on the bound device; see uzk_ctx_create."""
    h = ctypes.c_uint64(0)
    check(lib.uzk_ctx_create(ctypes.byref(h)))
    return h.value


def ctx_create_on(device: int) -> int:
    """A new context on HIP device `device` (uzk_ctx_create_on): SRS handles, circuits and provers made while it is current live
    there, so one process can drive several GPUs."""
    h = ctypes.c_uint64(0)
    check(lib.uzk_ctx_create_on(device, ctypes.byref(h)))
    return h.value


def ctx_device(ctx: int = 0) -> int:
    d = ctypes.c_int(0)
    check(lib.uzk_ctx_device(ctx, ctypes.byref(d)))
    return d.value


def ctx_set_current(ctx: int) -> None:
    """Make `ctx` (0 = default) the calling thread's current context."""
    check(lib.uzk_ctx_set_current(ctx))


def ctx_destroy(ctx: int) -> None:
    check(lib.uzk_ctx_destroy(ctx))


def ctx_current() -> int:
    h = ctypes.c_uint64(0)
    check(lib.uzk_ctx_current(ctypes.byref(h)))
    return h.value


def ctx_wait(other: int) -> None:
    """The calling thread's current context waits on the device for everything queued so far on context `other`."""
    check(lib.uzk_ctx_wait(other))


class ShardedSrs:
    """An SRS cut into contiguous point chunks over several devices of ONE process (uzk_srs_register_sharded): `devices` names the
    device of every chunk (an ordinal may repeat).  msm() runs the chunks side by side and folds the partial sums on the host."""

    def __init__(self, points: np.ndarray, devices, window_bits: int = -1):
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        dev = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_uint64(0)
        check(lib.uzk_srs_register_sharded(_ptr(pts), pts.shape[0], dev, len(devices), window_bits, ctypes.byref(h)))
        self.handle, self.n, self.n_chunks = h.value, pts.shape[0], len(devices)

    def msm(self, scalars: np.ndarray, want_partials: bool = False):
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(12, dtype=np.uint64)
        parts = np.zeros((self.n_chunks, 12), dtype=np.uint64)
        check(lib.uzk_msm_g1_sharded(self.handle, _ptr(s), s.shape[0], _ptr(parts) if want_partials else None, _ptr(out)))
        return (out, parts) if want_partials else out

    def info(self):
        """(n, [(device, lo, hi) per chunk])"""
        n, k = ctypes.c_size_t(0), ctypes.c_uint32(0)
        dev = (ctypes.c_int * self.n_chunks)()
        bounds = (ctypes.c_size_t * (2 * self.n_chunks))()
        check(lib.uzk_srs_sharded_info(self.handle, ctypes.byref(n), ctypes.byref(k), dev, bounds))
        return n.value, [(dev[i], bounds[2 * i], bounds[2 * i + 1]) for i in range(k.value)]

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_srs_release_sharded(self.handle))
            self.handle = 0


class Srs:
    """Device-resident SRS (static bases of KZG commit)."""

    def __init__(self, handle: int, n: int):
        self.handle, self.n = handle, n

    @classmethod
    def from_host(cls, points: np.ndarray) -> "Srs":
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        h = ctypes.c_uint64(0)
        check(lib.uzk_srs_register(_ptr(pts), pts.shape[0], ctypes.byref(h)))
        return cls(h.value, pts.shape[0])

    @classmethod
    def from_device(cls, d_ptr: int, n: int) -> "Srs":
        h = ctypes.c_uint64(0)
        check(lib.uzk_srs_register_device(ctypes.c_void_p(d_ptr), n, ctypes.byref(h)))
        return cls(h.value, n)

    def precompute(self, window_bits: int = 0) -> None:
        """Build the window table for a static SRS (uzk_srs_precompute)."""
        check(lib.uzk_srs_precompute(self.handle, window_bits))

    def to_lagrange(self, n: int) -> "Srs":
        """The Lagrange bases of size n from the first n points of this (monomial) SRS: the inverse G1 transform on the
        device (uzk_srs_to_lagrange).  The new SRS owns its memory."""
        h = ctypes.c_uint64(0)
        check(lib.uzk_srs_to_lagrange(self.handle, n, ctypes.byref(h)))
        return Srs(h.value, n)

    def download(self, offset: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Points [n, 8] of the SRS read back from the device (uzk_srs_download)."""
        if n is None:
            n = self.n - offset
        out = np.zeros((max(n, 0), 8), dtype=np.uint64)
        check(lib.uzk_srs_download(self.handle, offset, n, _ptr(out) if out.shape[0] else None))
        return out

    def check_curve(self, offset: int = 0, count: Optional[int] = None) -> dict:
        """uzk_srs_check_curve over points [offset, offset + count): {"checked", "infinity", "non_canonical", "off_curve",
        "first_bad"}; first_bad is an index into the SRS, None when every point is on the curve or the identity."""
        if count is None:
            count = self.n - offset
        r = N.SrsCurveReport()
        check(lib.uzk_srs_check_curve(self.handle, offset, count, ctypes.byref(r)))
        return {"checked": r.checked, "infinity": r.infinity, "non_canonical": r.non_canonical, "off_curve": r.off_curve,
                "first_bad": None if r.first_bad == 2 ** 64 - 1 else r.first_bad}

    def fold_powers(self, seed: bytes, offset: int = 0, count: Optional[int] = None):
        """uzk_srs_fold_powers: (left [12], right [12]) of the run [offset, offset + count) under the weights of the 32-byte seed;
        the run is a power sequence of tau iff e(right, H) = e(left, [tau] H) -- the caller's pairing."""
        if count is None:
            count = self.n - offset
        left, right = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(lib.uzk_srs_fold_powers(self.handle, offset, count, _seed(seed), _ptr(left), _ptr(right)))
        return left, right

    def fold_powers_lagrange(self, seed: bytes, n: int):
        """uzk_srs_fold_powers_lagrange: (first [8], left [12], right [12]) over the forward G1 transform of the first n points of
        this (Lagrange) SRS; first = sum_i L_i, the generator if the bases are what they claim to be."""
        first, left, right = np.zeros(8, dtype=np.uint64), np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(lib.uzk_srs_fold_powers_lagrange(self.handle, n, _seed(seed), _ptr(first), _ptr(left), _ptr(right)))
        return first, left, right

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_srs_release(self.handle))
            self.handle = 0


def _seed(seed: bytes):
    s = bytes(seed)
    if len(s) != 32:
        from .errors import UzkgeError
        raise UzkgeError(N.UZK_ERR_PARAMETER, "a fold seed is 32 bytes, got %d" % len(s))
    return ctypes.c_char_p(s)


def srs_fold_weights(seed: bytes, first: int, count: int) -> np.ndarray:
    """uzk_srs_fold_weights (host only): weights first .. first + count - 1 of the seed, [count, 4] Montgomery limbs."""
    out = np.zeros((count, 4), dtype=np.uint64)
    check(lib.uzk_srs_fold_weights(_seed(seed), first, count, _ptr(out) if count else None))
    return out


def srs_fold_weights_device(seed: bytes, count: int) -> np.ndarray:
    """uzk_test_srs_weights_device (test hook): weights 0 .. count - 1 as the device kernel writes them."""
    out = np.zeros((count, 4), dtype=np.uint64)
    check(lib.uzk_test_srs_weights_device(_seed(seed), count, _ptr(out) if count else None))
    return out


def msm(srs: Srs, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
    """sum_i scalars[i] * SRS[offset+i] -> Jacobian [12] (G1Projective::msm, kzg_poly_commitment.rs:290)."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(12, dtype=np.uint64)
    check(lib.uzk_msm_g1(srs.handle, offset, _ptr(s) if s.shape[0] else None, s.shape[0], _ptr(out)))
    return out


def msm_device(srs: Srs, d_scalars: int, n: int, offset: int = 0) -> np.ndarray:
    out = np.zeros(12, dtype=np.uint64)
    check(lib.uzk_msm_g1_device(srs.handle, offset, ctypes.c_void_p(d_scalars), n, _ptr(out)))
    return out


def msm_batch(srs: Srs, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
    """scalars [batch, n, 4] against the same bases -> [batch, 12] Jacobian results."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    assert s.ndim == 3 and s.shape[2] == 4
    out = np.zeros((s.shape[0], 12), dtype=np.uint64)
    check(lib.uzk_msm_g1_batch(srs.handle, offset, _ptr(s) if s.size else None, s.shape[1], s.shape[0], _ptr(out)))
    return out


def msm_batch_device(srs: Srs, d_scalars: int, n: int, batch: int, offset: int = 0) -> np.ndarray:
    out = np.zeros((batch, 12), dtype=np.uint64)
    check(lib.uzk_msm_g1_batch_device(srs.handle, offset, ctypes.c_void_p(d_scalars), n, batch, _ptr(out)))
    return out


def msm_raw(points: np.ndarray, scalars: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    if p.shape[0] != s.shape[0]:
        # ark_ec::VariableBaseMSM::msm returns Err(min_len) here; the reference unwraps it
        from .errors import UzkgeError
        raise UzkgeError(N.UZK_ERR_COMMITMENT, f"points ({p.shape[0]}) and scalars ({s.shape[0]}) differ in length")
    out = np.zeros(12, dtype=np.uint64)
    check(lib.uzk_msm_g1_raw(_ptr(p) if p.shape[0] else None, _ptr(s) if s.shape[0] else None, s.shape[0], _ptr(out)))
    return out


def g1_fold(partials: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(partials, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, dtype=np.uint64)
    check(lib.uzk_g1_fold(_ptr(p), p.shape[0], _ptr(out)))
    return out


def g1_to_affine(jac: np.ndarray) -> np.ndarray:
    j = np.ascontiguousarray(jac, dtype=np.uint64).reshape(12)
    out = np.zeros(8, dtype=np.uint64)
    check(lib.uzk_g1_to_affine(_ptr(j), _ptr(out)))
    return out


class G2Bases:
    """Device-resident G2 bases (b_g2_query of a Groth16 proving key): points [n, 16] = x.c0, x.c1, y.c0, y.c1 in Montgomery words,
    infinity = zeros."""

    def __init__(self, handle: int, n: int):
        self.handle, self.n = handle, n

    @classmethod
    def from_host(cls, points: np.ndarray) -> "G2Bases":
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 16)
        h = ctypes.c_uint64(0)
        check(lib.uzk_g2_register(_ptr(pts) if pts.shape[0] else None, pts.shape[0], ctypes.byref(h)))
        return cls(h.value, pts.shape[0])

    def len(self) -> int:
        n = ctypes.c_size_t(0)
        check(lib.uzk_g2_len(self.handle, ctypes.byref(n)))
        return n.value

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_g2_release(self.handle))
            self.handle = 0


def msm_g2(bases: G2Bases, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
    """sum_i scalars[i] * bases[offset + i] -> Jacobian [24]"""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(24, dtype=np.uint64)
    check(lib.uzk_msm_g2(bases.handle, offset, _ptr(s) if s.shape[0] else None, s.shape[0], _ptr(out)))
    return out


def msm_g2_batch(bases: G2Bases, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
    """scalars [batch, n, 4] against the same bases -> [batch, 24] Jacobian results."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    assert s.ndim == 3 and s.shape[2] == 4
    out = np.zeros((s.shape[0], 24), dtype=np.uint64)
    check(lib.uzk_msm_g2_batch(bases.handle, offset, _ptr(s) if s.size else None, s.shape[1], s.shape[0], _ptr(out)))
    return out


def msm_g2_batch_device(bases: G2Bases, d_scalars: int, n: int, batch: int, offset: int = 0) -> np.ndarray:
    out = np.zeros((batch, 24), dtype=np.uint64)
    check(lib.uzk_msm_g2_batch_device(bases.handle, offset, ctypes.c_void_p(d_scalars), n, batch, _ptr(out)))
    return out


def g2_msm_finish(bases: G2Bases, d_scalars: int, n: int, batch: int, offset: int = 0, d_out: int = 0, host: bool = True):
    """uzk_msm_g2_batch_finish: the sums of msm_g2_batch_device as canonical affine points [batch, 16] (infinity = zeros), combined
    and mapped to affine on the device.  d_out: a device address that also receives them (batch x 128 bytes); host=False: d_out alone,
    returns None."""
    out = np.zeros((max(batch, 1), 16), dtype=np.uint64) if host else None
    check(lib.uzk_msm_g2_batch_finish(bases.handle, offset, ctypes.c_void_p(d_scalars), n, batch, _ptr(out) if host else None,
                                      ctypes.c_void_p(d_out) if d_out else None))
    return out[:batch] if host else None


def g2_fold(partials: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(partials, dtype=np.uint64).reshape(-1, 24)
    out = np.zeros(24, dtype=np.uint64)
    check(lib.uzk_g2_fold(_ptr(p) if p.shape[0] else None, p.shape[0], _ptr(out)))
    return out


def g2_to_affine(jac: np.ndarray) -> np.ndarray:
    j = np.ascontiguousarray(jac, dtype=np.uint64).reshape(24)
    out = np.zeros(16, dtype=np.uint64)
    check(lib.uzk_g2_to_affine(_ptr(j), _ptr(out)))
    return out


class Groth16Key:
    """A Groth16 proving key and its R1CS resident on the device (uzk_g16_key_create).  Points travel in the wire format: G1
    [n, 8], G2 [n, 16], infinity = zeros; field elements [n, 4] Montgomery words.  `matrices` = three (row_ptr, col, val) triples in
    CSR for A, B, C.  Use as a context manager, or release() it."""

    def __init__(self, handle: int):
        self.handle = handle
        m, l, nc, n = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        check(lib.uzk_g16_key_info(handle, ctypes.byref(m), ctypes.byref(l), ctypes.byref(nc), ctypes.byref(n), None))
        self.n_vars, self.n_inputs, self.n_constraints, self.domain = m.value, l.value, nc.value, n.value

    @staticmethod
    def describe(n_vars: int, n_inputs: int, n_constraints: int, alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query, b_g1_query,
                 l_query, h_query, b_g2_query, matrices):
        """(descriptor, the arrays it points into): what from_arrays hands to uzk_g16_key_create"""
        d = N.G16KeyDesc()
        keep = []

        def arr(a, dtype, width):
            a = np.ascontiguousarray(a, dtype=dtype)
            if width:
                a = a.reshape(-1, width)
            keep.append(a)
            return a

        d.n_vars, d.n_inputs, d.n_constraints = n_vars, n_inputs, n_constraints
        for name, v, width in (("alpha_g1", alpha_g1, 8), ("beta_g1", beta_g1, 8), ("delta_g1", delta_g1, 8), ("beta_g2", beta_g2, 16),
                               ("delta_g2", delta_g2, 16)):
            w = np.ascontiguousarray(v, dtype=np.uint64).reshape(width)
            setattr(d, name, (ctypes.c_uint64 * width)(*[int(x) for x in w]))
        for name, v, width in (("a_query", a_query, 8), ("b_g1_query", b_g1_query, 8), ("l_query", l_query, 8), ("h_query", h_query, 8),
                               ("b_g2_query", b_g2_query, 16)):
            a = arr(v, np.uint64, width)
            setattr(d, name, a.ctypes.data if a.size else None)
            if name in ("l_query", "h_query"):
                setattr(d, name + "_len", a.shape[0])
        for k, (row_ptr, col, val) in enumerate(matrices):
            rp, cl, vl = arr(row_ptr, np.uint64, 0), arr(col, np.uint32, 0), arr(val, np.uint64, 4)
            d.row_ptr[k] = rp.ctypes.data if rp.size else None
            d.col[k] = cl.ctypes.data if cl.size else None
            d.val[k] = vl.ctypes.data if vl.size else None
        return d, keep

    @classmethod
    def from_arrays(cls, *args, **kwargs) -> "Groth16Key":
        d, keep = cls.describe(*args, **kwargs)
        h = ctypes.c_uint64(0)
        check(lib.uzk_g16_key_create(ctypes.byref(d), ctypes.byref(h)))
        del keep
        return cls(h.value)

    def h_device(self, d_z: int, batch: int, d_h: int) -> None:
        """the witness map on device-resident assignments (batch x n_vars) -> batch x domain coefficients at d_h"""
        check(lib.uzk_g16_h_device(self.handle, ctypes.c_void_p(d_z), batch, ctypes.c_void_p(d_h)))

    def h(self, z: np.ndarray) -> np.ndarray:
        """z [batch, n_vars, 4] -> h [batch, domain, 4]"""
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, self.n_vars, 4)
        batch = z.shape[0]
        d_z, d_h = dev_alloc(max(z.nbytes, 32)), dev_alloc(max(batch * self.domain * 32, 32))
        try:
            dev_upload(d_z, z)
            self.h_device(d_z, batch, d_h)
            return dev_download(d_h, (batch, self.domain, 4))
        finally:
            dev_free(d_z)
            dev_free(d_h)

    def _prove_finish(self, z, on_device: bool, r: np.ndarray, s: np.ndarray, d_blobs: int):
        """uzk_g16_prove_batch_finish -> (proofs [batch, 32], blobs [batch, 256] bytes)"""
        batch = r.shape[0]
        proofs = np.zeros((max(batch, 1), 32), dtype=np.uint64)
        blobs = np.zeros((max(batch, 1), N.G16_PROOF_BYTES), dtype=np.uint8)
        check(lib.uzk_g16_prove_batch_finish(self.handle, z, int(on_device), _ptr(r) if r.size else None, _ptr(s) if s.size else None, batch, _ptr(proofs),
                                             blobs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_blobs) if d_blobs else None))
        return proofs[:batch], blobs[:batch]

    def prove(self, z: np.ndarray, r: np.ndarray, s: np.ndarray, finish: str = "host", d_blobs: int = 0):
        """z [batch, n_vars, 4], r and s [batch, 4] -> proofs [batch, 32]: A (8 words), B (16), C (8), affine, infinity = zeros.
        finish="device": C, the affine maps and the encoding run on the device (uzk_g16_prove_batch_finish); returns (proofs, blobs) with
        blobs [batch, 256] bytes as Groth16VerifierKey.verify_batch reads them, also left at the device address d_blobs when given."""
        if finish not in ("host", "device"):
            raise ValueError("finish is 'host' or 'device'")
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, self.n_vars, 4)
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        assert r.shape[0] == z.shape[0] and s.shape[0] == z.shape[0]
        if finish == "device":
            return self._prove_finish(_ptr(z) if z.size else None, False, r, s, d_blobs)
        out = np.zeros((z.shape[0], 32), dtype=np.uint64)
        check(lib.uzk_g16_prove_batch(self.handle, _ptr(z) if z.size else None, _ptr(r) if r.size else None, _ptr(s) if s.size else None,
                                      z.shape[0], _ptr(out)))
        return out

    def prove_device(self, d_z: int, r: np.ndarray, s: np.ndarray, finish: str = "host", d_blobs: int = 0):
        """`prove` over assignments at the device address d_z"""
        if finish not in ("host", "device"):
            raise ValueError("finish is 'host' or 'device'")
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        assert r.shape[0] == s.shape[0]
        if finish == "device":
            return self._prove_finish(ctypes.c_void_p(d_z), True, r, s, d_blobs)
        out = np.zeros((r.shape[0], 32), dtype=np.uint64)
        check(lib.uzk_g16_prove_batch_device(self.handle, ctypes.c_void_p(d_z), _ptr(r) if r.size else None, _ptr(s) if s.size else None,
                                             r.shape[0], _ptr(out)))
        return out

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_g16_key_release(self.handle))
            self.handle = 0

    def __enter__(self) -> "Groth16Key":
        return self

    def __exit__(self, *exc) -> None:
        self.release()


def domain_supported(n: int) -> bool:
    return bool(lib.uzk_domain_supported(n))


def domain_group_gen(n: int) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64)
    check(lib.uzk_domain_group_gen(n, _ptr(out)))
    return out


def ntt(data: np.ndarray, inverse: bool = False, coset_shift: Optional[np.ndarray] = None) -> np.ndarray:
    """EvaluationDomain::fft / ifft over the size-len(data) domain (field_polynomial.rs:583-597);
    returns a new [n,4] array, natural order."""
    a = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4).copy()
    cs = None
    if coset_shift is not None:
        cs = np.ascontiguousarray(coset_shift, dtype=np.uint64).reshape(4)
    check(lib.uzk_ntt_fr(_ptr(a), a.shape[0], int(inverse), _ptr(cs) if cs is not None else None))
    return a


def ntt_inplace(a: np.ndarray, inverse: bool = False, coset_shift: Optional[np.ndarray] = None) -> None:
    """uzk_ntt_fr as the C ABI defines it: `a` ([n,4] u64, C-contiguous) is transformed in place (no copy here)."""
    assert a.dtype == np.uint64 and a.flags.c_contiguous and a.ndim == 2 and a.shape[1] == 4
    cs = None
    if coset_shift is not None:
        cs = np.ascontiguousarray(coset_shift, dtype=np.uint64).reshape(4)
    check(lib.uzk_ntt_fr(_ptr(a), a.shape[0], int(inverse), _ptr(cs) if cs is not None else None))


def ntt_batch(data: np.ndarray, inverse: bool = False, coset_shift: Optional[np.ndarray] = None) -> np.ndarray:
    """`data` [batch, n, 4]: batch independent transforms of size n in one call."""
    a = np.ascontiguousarray(data, dtype=np.uint64).copy()
    assert a.ndim == 3 and a.shape[2] == 4
    cs = None
    if coset_shift is not None:
        cs = np.ascontiguousarray(coset_shift, dtype=np.uint64).reshape(4)
    check(lib.uzk_ntt_fr_batch(_ptr(a), a.shape[1], a.shape[0], int(inverse), _ptr(cs) if cs is not None else None))
    return a


def ntt_batch_device(d_in: int, d_out: int, n: int, batch: int, inverse: bool = False,
                     coset_shift: Optional[np.ndarray] = None, sync: bool = False) -> None:
    cs = None
    if coset_shift is not None:
        cs = np.ascontiguousarray(coset_shift, dtype=np.uint64).reshape(4)
    check(lib.uzk_ntt_fr_batch_device(ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n, batch, int(inverse),
                                      _ptr(cs) if cs is not None else None, int(sync)))


def ntt_device(d_in: int, d_out: int, n: int, inverse: bool = False, coset_shift: Optional[np.ndarray] = None,
               sync: bool = False) -> None:
    cs = None
    if coset_shift is not None:
        cs = np.ascontiguousarray(coset_shift, dtype=np.uint64).reshape(4)
    check(lib.uzk_ntt_fr_device(ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n, int(inverse),
                                _ptr(cs) if cs is not None else None, int(sync)))


def ntt_g1_supported(n: int) -> bool:
    return bool(lib.uzk_ntt_g1_supported(n))


def ntt_g1(points: np.ndarray, inverse: bool = False) -> np.ndarray:
    """EvaluationDomain::fft / ifft over a vector of G1 points ([n, 8] affine wire rows, (0, 0) = infinity), natural
    order in and out; returns a new array.  inverse(monomial SRS) = Lagrange SRS."""
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros_like(p)
    check(lib.uzk_ntt_g1(_ptr(p) if p.shape[0] else None, _ptr(out) if p.shape[0] else None, p.shape[0], int(inverse)))
    return out


def ntt_g1_device(d_in: int, d_out: int, n: int, inverse: bool = False, sync: bool = False) -> None:
    check(lib.uzk_ntt_g1_device(ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n, int(inverse), int(sync)))


def ntt_g1_plan_info(n: int, inverse: bool = False) -> Tuple[int, int]:
    """(doublings, additions) one G1 transform of size n runs."""
    d, a = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib.uzk_ntt_g1_plan_info(n, int(inverse), ctypes.byref(d), ctypes.byref(a)))
    return d.value, a.value


def poly_eval_batch(coefs: np.ndarray, x_mont: np.ndarray) -> np.ndarray:
    """coefs [batch, n, 4] -> [batch, 4]: p_b(x) (FpPolynomial::eval for a batch at one point)."""
    c = np.ascontiguousarray(coefs, dtype=np.uint64)
    assert c.ndim == 3 and c.shape[2] == 4
    x = np.ascontiguousarray(x_mont, dtype=np.uint64).reshape(4)
    out = np.zeros((c.shape[0], 4), dtype=np.uint64)
    check(lib.uzk_poly_eval_batch(_ptr(c) if c.size else None, c.shape[1], c.shape[0], _ptr(x), _ptr(out)))
    return out


def poly_eval_batch_device(d_coefs: int, n: int, batch: int, x_mont: np.ndarray) -> np.ndarray:
    """batch device-resident polynomials of n coefficients each (contiguous) evaluated at one point -> [batch, 4]."""
    x = np.ascontiguousarray(x_mont, dtype=np.uint64).reshape(4)
    out = np.zeros((batch, 4), dtype=np.uint64)
    check(lib.uzk_poly_eval_batch_device(ctypes.c_void_p(d_coefs), n, batch, _ptr(x), _ptr(out)))
    return out


def z_poly(w: np.ndarray, perm: np.ndarray, group: np.ndarray, k: np.ndarray, beta: np.ndarray, gamma: np.ndarray) -> np.ndarray:
    """Permutation grand product evaluations (helpers.rs:160-220).  w [n_wires, n, 4], perm [n_wires, n] uint32."""
    wv = np.ascontiguousarray(w, dtype=np.uint64)
    n_wires, n = wv.shape[0], wv.shape[1]
    pm = np.ascontiguousarray(perm, dtype=np.uint32).reshape(n_wires, n)
    g = np.ascontiguousarray(group, dtype=np.uint64).reshape(n, 4)
    kk = np.ascontiguousarray(k, dtype=np.uint64).reshape(n_wires, 4)
    out = np.zeros((n, 4), dtype=np.uint64)
    check(lib.uzk_z_poly(_ptr(wv), pm.ctypes.data_as(ctypes.c_void_p), _ptr(g), _ptr(kk),
                         _ptr(np.ascontiguousarray(beta, dtype=np.uint64).reshape(4)),
                         _ptr(np.ascontiguousarray(gamma, dtype=np.uint64).reshape(4)), n, n_wires, _ptr(out)))
    return out


def z_poly_device(d_w: int, d_perm: int, d_group: int, k: np.ndarray, beta: np.ndarray, gamma: np.ndarray, n: int,
                  n_wires: int, d_z: int) -> None:
    """z_poly on device-resident wires / permutation / domain (helpers.rs:160-220); z -> d_z (n elements)."""
    kk = np.ascontiguousarray(k, dtype=np.uint64).reshape(n_wires, 4)
    check(lib.uzk_z_poly_device(ctypes.c_void_p(d_w), ctypes.c_void_p(d_perm), ctypes.c_void_p(d_group), _ptr(kk),
                                _ptr(np.ascontiguousarray(beta, dtype=np.uint64).reshape(4)),
                                _ptr(np.ascontiguousarray(gamma, dtype=np.uint64).reshape(4)), n, n_wires,
                                ctypes.c_void_p(d_z)))


def open_quotient_device(d_polys: int, n: int, batch: int, z: np.ndarray, alpha: np.ndarray, d_q: int) -> np.ndarray:
    """batch_prove's polynomial work (pcs.rs:119-135): writes q = sum_k alpha^k (p_k - p_k(z)) / (X - z) to d_q
    (n elements, the last one zero) and returns the evaluations p_k(z) [batch, 4]."""
    ev = np.zeros((batch, 4), dtype=np.uint64)
    check(lib.uzk_open_quotient_device(ctypes.c_void_p(d_polys), n, batch,
                                       _ptr(np.ascontiguousarray(z, dtype=np.uint64).reshape(4)),
                                       _ptr(np.ascontiguousarray(alpha, dtype=np.uint64).reshape(4)),
                                       ctypes.c_void_p(d_q), _ptr(ev)))
    return ev


def open_quotient(polys: np.ndarray, z: np.ndarray, alpha: np.ndarray):
    """Host-array form of open_quotient_device: polys [batch, n, 4] -> (q [n, 4] with a trailing zero, evals [batch, 4])."""
    p = np.ascontiguousarray(polys, dtype=np.uint64)
    assert p.ndim == 3 and p.shape[2] == 4
    batch, n = p.shape[0], p.shape[1]
    q = np.zeros((n, 4), dtype=np.uint64)
    ev = np.zeros((batch, 4), dtype=np.uint64)
    check(lib.uzk_open_quotient(_ptr(p), n, batch, _ptr(np.ascontiguousarray(z, dtype=np.uint64).reshape(4)),
                                _ptr(np.ascontiguousarray(alpha, dtype=np.uint64).reshape(4)), _ptr(q), _ptr(ev)))
    return q, ev


def fold_blinds_device(d_coefs: int, length: int, n_fold: int, d_out: int) -> np.ndarray:
    """Fold modulo X^N - 1 on the device (pcs.rs:137-156 / helpers.rs:1366-1383); returns blinds [len - N, 4]."""
    nb = max(0, length - n_fold)
    blinds = np.zeros((max(nb, 1), 4), dtype=np.uint64)
    check(lib.uzk_fold_blinds_device(ctypes.c_void_p(d_coefs), length, n_fold, ctypes.c_void_p(d_out), _ptr(blinds)))
    return blinds[:nb]


def poly_lincomb_device(d_polys, lens, scalars: np.ndarray, d_out: int, out_len: int) -> None:
    """d_out[j] = sum_k scalars[k] * poly_k[j] (r_poly's shape, helpers.rs:681-999); d_polys: device pointers, lens: lengths."""
    cnt = len(d_polys)
    ptrs = (ctypes.c_void_p * cnt)(*[ctypes.c_void_p(p) for p in d_polys])
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(cnt, 4)
    check(lib.uzk_poly_lincomb_device(ptrs, _ptr(ln), _ptr(sc), cnt, ctypes.c_void_p(d_out), out_len))


def hide_polynomial_device(d_coefs: int, length: int, blinds: np.ndarray, zeroing_degree: int) -> None:
    """hide_polynomial (helpers.rs:139-158) on device-resident coefficients."""
    bl = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(-1, 4)
    check(lib.uzk_hide_polynomial_device(ctypes.c_void_p(d_coefs), length, _ptr(bl) if bl.shape[0] else None, bl.shape[0], zeroing_degree))


def t_quotient_device(n: int, factor: int, vec_ptrs, alpha, beta, gamma, k, anemoi_g, anemoi_g_inv, edwards_a,
                      z_h_inv, d_out: int, sync: bool = True) -> None:
    """The quotient evaluations of t_poly (helpers.rs:284-656) on device-resident coset evaluations.
    vec_ptrs: 56 device pointers in UZK_TQ_* slot order; scalars as [4] uint64 Montgomery limbs,
    k [5, 4], z_h_inv [factor, 4]; d_out: n * factor elements."""
    from ._native import QuotientArgs, TQ_NVEC
    assert len(vec_ptrs) == TQ_NVEC
    a = QuotientArgs()
    a.n, a.factor = n, factor
    for i, p in enumerate(vec_ptrs):
        a.vec[i] = p
    def put(dst, src):
        v = np.ascontiguousarray(src, dtype=np.uint64).reshape(4)
        for j in range(4):
            dst[j] = int(v[j])
    put(a.alpha, alpha); put(a.beta, beta); put(a.gamma, gamma)
    put(a.anemoi_g, anemoi_g); put(a.anemoi_g_inv, anemoi_g_inv); put(a.edwards_a, edwards_a)
    kk = np.ascontiguousarray(k, dtype=np.uint64).reshape(5, 4)
    for j in range(5):
        put(a.k[j], kk[j])
    zz = np.ascontiguousarray(z_h_inv, dtype=np.uint64).reshape(-1, 4)
    for j in range(min(16, zz.shape[0])):
        put(a.z_h_inv[j], zz[j])
    check(lib.uzk_t_quotient_device(ctypes.byref(a), ctypes.c_void_p(d_out), int(sync)))


def synth_points_arith(d_points: int, n: int, seed_scalar_mont: np.ndarray) -> None:
    s = np.ascontiguousarray(seed_scalar_mont, dtype=np.uint64).reshape(4)
    check(lib.uzk_synth_points_arith(ctypes.c_void_p(d_points), n, _ptr(s)))


def synth_points_random(d_points: int, n: int, seed: int) -> None:
    check(lib.uzk_synth_points_random(ctypes.c_void_p(d_points), n, seed))


def synth_scalars(d_scalars: int, n: int, seed: int) -> None:
    check(lib.uzk_synth_scalars(ctypes.c_void_p(d_scalars), n, seed))


def synth_scalars_mix(d_scalars: int, n: int, seed: int) -> None:
    """Prover-like scalar mix (50 % zero, 20 % one, 10 % r-1, 10 % < 2^16, 10 % uniform)."""
    check(lib.uzk_synth_scalars_mix(ctypes.c_void_p(d_scalars), n, seed))


def field_op(field: str, op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Device field primitive applied element-wise (KATs: include/uzkge_gpu_test.h, every opcode).  field: 'fq' | 'fr'."""
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros_like(x)
    check(lib.uzk_test_field_kat(0 if field == "fq" else 1, op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]))
    return out


def const_operands(field: str, op: int, form_a: int, form_b: int, a: np.ndarray, b: np.ndarray, portable: bool = False) -> np.ndarray:
    """uzk_test_const_operands: a device primitive in the kernel whose operands have the given forms (literal words fixed at compile
    time, the rest loaded from a / b); include/uzkge_gpu_test.h lists ops and forms."""
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros_like(x)
    check(lib.uzk_test_const_operands(0 if field == "fq" else 1, op, form_a, form_b, int(portable), _ptr(x), _ptr(y), _ptr(out), x.shape[0]))
    return out


def field_elementwise(field: str, op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """uzk_field_op_device, the PRODUCT entry point: mul 0, add 1, sub 2, sqr 4, neg 5, from_mont 6, to_mont 7 on host arrays."""
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros_like(x)
    check(lib.uzk_field_op_device(0 if field == "fq" else 1, op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]))
    return out


def g1_op(op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 8)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((x.shape[0], 12), dtype=np.uint64)
    check(lib.uzk_test_g1_kat(op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]))
    return out


def g2_op(op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """uzk_test_g2_kat: op 0..5 on Fq2 elements [n, 8] -> [n, 8]; op 10..14 on affine points [n, 16] -> Jacobian [n, 24]"""
    w_in, w_out = (16, 24) if op >= 10 else (8, 8)
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, w_in)
    y = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, w_in)
    out = np.zeros((x.shape[0], w_out), dtype=np.uint64)
    check(lib.uzk_test_g2_kat(op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]))
    return out


def g2_raw_op(op: int, records: np.ndarray) -> np.ndarray:
    """uzk_test_g2_raw_kat: [n, 147] uint32 records (two raw points of 73 words and a flag) -> [n, 73] raw points"""
    x = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 147)
    out = np.zeros((x.shape[0], 73), dtype=np.uint32)
    check(lib.uzk_test_g2_raw_kat(op, x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0]))
    return out


def _raw_hook(fn, op: int, records: np.ndarray, w_in: int, w_out: int) -> np.ndarray:
    x = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, w_in)
    out = np.zeros((x.shape[0], w_out), dtype=np.uint32)
    check(fn(op, x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0]))
    return out


def fq12_raw_op(op: int, records: np.ndarray) -> np.ndarray:
    """uzk_test_fq12_raw_kat: [n, 216] uint32 records (two raw Fq12 elements of 108 words) -> [n, 108] raw elements"""
    return _raw_hook(lib.uzk_test_fq12_raw_kat, op, records, 216, 108)


def miller_step_raw(op: int, records: np.ndarray) -> np.ndarray:
    """uzk_test_miller_step_raw: [n, 108] uint32 records (T, Q, xP, -yP raw) -> [n, 126] (x, y, z, l0, l1, l3 raw, lane differences)"""
    return _raw_hook(lib.uzk_test_miller_step_raw, op, records, 108, 126)


def ed_raw_op(op: int, records: np.ndarray) -> np.ndarray:
    """uzk_test_ed_raw_kat: [n, 72] uint32 records (two raw extended points of 36 words) -> [n, 37] (a raw point and a flag)"""
    return _raw_hook(lib.uzk_test_ed_raw_kat, op, records, 72, 37)


def profile_enable(on: bool) -> None:
    check(lib.uzk_profile_enable(int(on)))


def profile_reset() -> None:
    check(lib.uzk_profile_reset())


def profile_get(name: str):
    ms = ctypes.c_double(0)
    cnt = ctypes.c_uint64(0)
    check(lib.uzk_profile_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
    return ms.value, cnt.value


def profile_table() -> dict:
    buf = ctypes.create_string_buffer(1 << 16)
    check(lib.uzk_profile_dump(buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out


def set_msm_window_bits(c: int) -> None:
    check(lib.uzk_msm_set_window_bits(c))


def msm_plan_info(n: int) -> Tuple[int, int]:
    """(window bits, windows) a general-mode MSM over n points will use."""
    cb, w = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.uzk_msm_plan_info(n, ctypes.byref(cb), ctypes.byref(w)))
    return cb.value, w.value


def tune(key: str, value: int) -> None:
    check(lib.uzk_tune(key.encode(), value))


# ---- device memory (uzk_dev_*): what a host language uses instead of a HIP binding ----------------------------
COPY_H2D, COPY_D2H, COPY_D2D = 0, 1, 2


def dev_alloc(nbytes: int) -> int:
    p = ctypes.c_void_p(0)
    check(lib.uzk_dev_alloc(nbytes, ctypes.byref(p)))
    return p.value or 0


def dev_free(d_ptr: int) -> None:
    check(lib.uzk_dev_free(ctypes.c_void_p(d_ptr)))


def host_alloc(nbytes: int) -> int:
    """Pinned host memory (uploads from it are asynchronous); returns the address."""
    p = ctypes.c_void_p(0)
    check(lib.uzk_host_alloc(nbytes, ctypes.byref(p)))
    return p.value or 0


def host_free(h_ptr: int) -> None:
    check(lib.uzk_host_free(ctypes.c_void_p(h_ptr)))


def dev_upload(d_dst: int, a: np.ndarray) -> None:
    a = np.ascontiguousarray(a)
    check(lib.uzk_dev_copy(ctypes.c_void_p(d_dst), a.ctypes.data_as(ctypes.c_void_p), a.nbytes, COPY_H2D))


def dev_download(d_src: int, shape, dtype=np.uint64) -> np.ndarray:
    out = np.empty(shape, dtype=dtype)
    check(lib.uzk_dev_copy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_src), out.nbytes, COPY_D2H))
    return out


def dev_copy(d_dst: int, d_src: int, nbytes: int) -> None:
    check(lib.uzk_dev_copy(ctypes.c_void_p(d_dst), ctypes.c_void_p(d_src), nbytes, COPY_D2D))


def dev_copy2d(dst: int, dst_pitch: int, src: int, src_pitch: int, width: int, rows: int, kind: int = COPY_D2D) -> None:
    check(lib.uzk_dev_copy2d(ctypes.c_void_p(dst), dst_pitch, ctypes.c_void_p(src), src_pitch, width, rows, kind))


def dev_memset(d_dst: int, byte: int, nbytes: int) -> None:
    check(lib.uzk_dev_memset(ctypes.c_void_p(d_dst), byte, nbytes))


def dev_memset2d(d_dst: int, pitch: int, byte: int, width: int, rows: int) -> None:
    check(lib.uzk_dev_memset2d(ctypes.c_void_p(d_dst), pitch, byte, width, rows))


# ---- batched / strided / pointer-list forms (one launch per prover step) -----------------------------------------
def _fr4(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(4)


def ntt_batch_strided_device(d_in: int, in_stride: int, d_out: int, out_stride: int, n: int, batch: int, inverse: bool = False,
                             coset_shift: Optional[np.ndarray] = None, sync: bool = False) -> None:
    cs = _fr4(coset_shift) if coset_shift is not None else None
    check(lib.uzk_ntt_fr_batch_strided_device(ctypes.c_void_p(d_in), in_stride, ctypes.c_void_p(d_out), out_stride, n, batch,
                                              int(inverse), _ptr(cs) if cs is not None else None, int(sync)))


def ntt_in_len_device(d_in: int, in_stride: int, d_out: int, out_stride: int, n: int, batch: int, in_len: int,
                      coset_shift: Optional[np.ndarray] = None) -> None:
    """uzk_test_ntt_in_len (test hook): the forward transform of ntt_batch_strided_device with the prover's statement that every
    input vector is zero from index in_len on (0 = no statement).  Synchronous."""
    cs = _fr4(coset_shift) if coset_shift is not None else None
    check(lib.uzk_test_ntt_in_len(ctypes.c_void_p(d_in), in_stride, ctypes.c_void_p(d_out), out_stride, n, batch,
                                  _ptr(cs) if cs is not None else None, in_len))


def msm_batch_tail_device(srs: Srs, d_scalars: int, stride: int, n: int, batch: int, tail, tail_n: int, offset: int = 0) -> np.ndarray:
    """`tail`: a host array [batch, tail_n, 4] or a device address (int) of batch * tail_n elements."""
    out = np.zeros((batch, 12), dtype=np.uint64)
    if isinstance(tail, (int, np.integer)):
        tp, on_dev = ctypes.c_void_p(int(tail)), 1
    else:
        t = np.ascontiguousarray(tail, dtype=np.uint64).reshape(batch * tail_n, 4) if tail_n else None
        tp, on_dev = (_ptr(t) if t is not None else None), 0
    check(lib.uzk_msm_g1_batch_tail_device(srs.handle, offset, ctypes.c_void_p(d_scalars), stride, n, batch, tp, tail_n, on_dev, _ptr(out)))
    return out


def hide_polynomial_batch_device(d_coefs: int, stride: int, len_in: int, blinds: np.ndarray, zeroing_degree: int) -> None:
    """blinds [count, hiding_degree, 4]."""
    bl = np.ascontiguousarray(blinds, dtype=np.uint64)
    assert bl.ndim == 3 and bl.shape[2] == 4
    check(lib.uzk_hide_polynomial_batch_device(ctypes.c_void_p(d_coefs), stride, len_in, bl.shape[0], _ptr(bl.reshape(-1, 4)), bl.shape[1],
                                               zeroing_degree))


def fold_blinds_batch_device(d_polys: int, in_stride: int, lens, n_fold: int, d_out: int, out_stride: int, d_tail: int, tail_n: int,
                             want_blinds: bool = False):
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    batch = ln.shape[0]
    bl = np.zeros((batch, max(tail_n // 2, 1), 4), dtype=np.uint64) if want_blinds else None
    check(lib.uzk_fold_blinds_batch_device(ctypes.c_void_p(d_polys), in_stride, _ptr(ln), n_fold, batch, ctypes.c_void_p(d_out), out_stride,
                                           ctypes.c_void_p(d_tail), tail_n, _ptr(bl.reshape(-1, 4)) if want_blinds else None))
    return bl[:, : tail_n // 2] if want_blinds else None


def poly_trimmed_len_device(d_polys: int, stride: int, lens) -> np.ndarray:
    """FpPolynomial::from_coefs' trimmed length of device-resident polynomials (1 + the highest non-zero index; 0 if zero)."""
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.zeros(ln.shape[0], dtype=np.uint64)
    check(lib.uzk_poly_trimmed_len_device(ctypes.c_void_p(d_polys), stride, _ptr(ln), ln.shape[0], _ptr(out), 1))
    return out


def poly_trimmed_len_async_device(d_polys: int, stride: int, lens, h_out: int) -> None:
    """The same without waiting: h_out = address of uzk_host_alloc memory (len(lens) u64), valid after the next synchronising call."""
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    check(lib.uzk_poly_trimmed_len_device(ctypes.c_void_p(d_polys), stride, _ptr(ln), ln.shape[0], ctypes.c_void_p(h_out), 0))


def split_t_device(d_t: int, t_len: int, chunk: int, rands: np.ndarray, d_chunks: int, chunk_stride: int) -> np.ndarray:
    """Returns the chunk lengths (the reference's coefs.len())."""
    r = np.ascontiguousarray(rands, dtype=np.uint64).reshape(-1, 4)
    lens = np.zeros(r.shape[0], dtype=np.uint64)
    check(lib.uzk_split_t_device(ctypes.c_void_p(d_t), t_len, chunk, r.shape[0], _ptr(r), ctypes.c_void_p(d_chunks), chunk_stride, _ptr(lens)))
    return lens


def _ptr_list(d_polys):
    return (ctypes.c_void_p * len(d_polys))(*[ctypes.c_void_p(p) for p in d_polys])


def poly_eval_ptrs_device(d_polys, lens, point_idx, points: np.ndarray) -> np.ndarray:
    cnt = len(d_polys)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    pi = np.ascontiguousarray(point_idx, dtype=np.uint32)
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros((cnt, 4), dtype=np.uint64)
    check(lib.uzk_poly_eval_ptrs_device(_ptr_list(d_polys), _ptr(ln), pi.ctypes.data_as(ctypes.c_void_p), cnt, _ptr(pts), pts.shape[0], _ptr(out)))
    return out


def open_quotient_ptrs_device(d_polys, lens, z: np.ndarray, alpha: np.ndarray, d_q: int, q_cap: int, want_evals: bool = False):
    cnt = len(d_polys)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    ev = np.zeros((cnt, 4), dtype=np.uint64) if want_evals else None
    check(lib.uzk_open_quotient_ptrs_device(_ptr_list(d_polys), _ptr(ln), cnt, _ptr(_fr4(z)), _ptr(_fr4(alpha)), ctypes.c_void_p(d_q), q_cap,
                                            _ptr(ev) if want_evals else None))
    return ev


# ---- circuits and the five prover rounds (uzk_circuit_*, uzk_prover_*, uzk_prove_round1..5) ---------------------------
CS_Q, CS_S, CS_L1, CS_QB, CS_QPRK, CS_COSET_QUOTIENT, CS_QPK, CS_QG, CS_QECC = 0, 9, 14, 15, 16, 20, 21, 33, 45
PB_EVALS, PB_COEFS, PB_COSET, PB_TQ, PB_T, PB_CHUNKS, PB_FOLD, PB_TAIL, PB_Q, PB_R = range(10)


def trimmed_len(coefs: np.ndarray) -> int:
    """coefs.len() after FpPolynomial::from_coefs (field_polynomial.rs:86-90): trailing zero coefficients dropped."""
    nz = np.nonzero(np.any(np.asarray(coefs).reshape(-1, 4) != 0, axis=1))[0]
    return int(nz[-1]) + 1 if nz.size else 0


class Circuit:
    """A circuit resident in HBM (uzk_circuit_create): commit bases, permutation, the 46 (21) polynomials and their coset tables."""

    def __init__(self, n: int, lagrange_bases: np.ndarray, blind_bases: np.ndarray, permutation: np.ndarray, k: np.ndarray, anemoi_g, anemoi_g_inv,
                 edwards_a, polys, shuffle: bool = True, precompute: bool = False, group_gen=None, lens=None, synthetic: bool = False):
        d = N.CircuitDesc()
        d.n, d.shuffle, d.precompute = n, int(shuffle), int(precompute)
        keep = []
        lag = np.ascontiguousarray(lagrange_bases, dtype=np.uint64).reshape(-1, 8)
        bb = np.ascontiguousarray(blind_bases, dtype=np.uint64).reshape(-1, 8)
        perm = np.ascontiguousarray(permutation, dtype=np.uint32).reshape(-1)
        assert lag.shape[0] == n and bb.shape[0] == 6 and perm.shape[0] == 5 * n
        keep += [lag, bb, perm]
        d.lagrange_bases, d.blind_bases, d.permutation = lag.ctypes.data, bb.ctypes.data, perm.ctypes.data

        kk = np.ascontiguousarray(k, dtype=np.uint64).reshape(5, 4)
        for j in range(5):
            for w in range(4):
                d.k[j][w] = int(kk[j, w])
        for name, val in (("anemoi_g", anemoi_g), ("anemoi_g_inv", anemoi_g_inv), ("edwards_a", edwards_a),
                          ("group_gen", domain_group_gen(n) if group_gen is None else group_gen)):
            v = np.ascontiguousarray(val, dtype=np.uint64).reshape(4)
            for w in range(4):
                getattr(d, name)[w] = int(v[w])
        n_slots = N.CIRCUIT_SLOTS if shuffle else CS_QPK
        for s in range(n_slots):
            if polys[s] is None:            # slot 20 (coset_quotient) is normally None: the library builds it
                continue
            a = np.ascontiguousarray(polys[s], dtype=np.uint64).reshape(-1, 4)
            keep.append(a)
            d.polys[s] = a.ctypes.data
            d.poly_lens[s] = trimmed_len(a) if lens is None else int(lens[s])
        h = ctypes.c_uint64(0)
        check(lib.uzk_circuit_create(ctypes.byref(d), ctypes.byref(h)))
        self.handle, self.n, self.shuffle, self.n_slots = h.value, n, shuffle, n_slots
        if synthetic:
            self.truncate_t(True)

    def truncate_t(self, on: bool) -> None:
        """TESTS / TIMING ONLY (uzk_test_circuit_truncate_t): a synthetic circuit no witness satisfies -- round 3 reads t as its
        first 5n - 2 + sum(hiding) coefficients, as tests/chain_oracle.py does."""
        check(lib.uzk_test_circuit_truncate_t(self.handle, int(on)))

    def info(self):
        """(n, evaluations per proof in round 4, r_poly scalars per proof in round 5, device)."""
        a, e, r, dv = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
        check(lib.uzk_circuit_info(self.handle, ctypes.byref(a), ctypes.byref(e), ctypes.byref(r), ctypes.byref(dv)))
        return a.value, e.value, r.value, dv.value

    def update_tables(self, first_slot: int, polys, lens=None) -> None:
        arrs = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
        ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        ln = (ctypes.c_uint64 * len(arrs))(*[trimmed_len(a) if lens is None else int(lens[i]) for i, a in enumerate(arrs)])
        check(lib.uzk_circuit_update_tables(self.handle, first_slot, len(arrs), ptrs, ln))

    def refresh_tables(self, first_slot: int, evals: np.ndarray, want_polys: bool = True, want_coset: bool = False):
        """The refresh / indexer loop on the device: evaluation vectors -> iFFT -> coset FFT -> Lagrange commit, installed in the
        slots.  Returns (commitments [count,12], polys [count,n,4] | None, lens, coset [count,6n,4] | None)."""
        e = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, self.n, 4)
        cnt = e.shape[0]
        polys = np.zeros((cnt, self.n, 4), dtype=np.uint64) if want_polys else None
        coset = np.zeros((cnt, 6 * self.n, 4), dtype=np.uint64) if want_coset else None
        lens = np.zeros(cnt, dtype=np.uint64)
        cms = np.zeros((cnt, 12), dtype=np.uint64)
        check(lib.uzk_circuit_refresh_tables(self.handle, first_slot, cnt, _ptr(e), _ptr(polys) if want_polys else None, _ptr(lens),
                                             _ptr(coset) if want_coset else None, _ptr(cms)))
        return cms, polys, lens, coset

    def table(self, slot: int, coset: bool = False):
        """(device address, element count) of a slot's polynomial or coset table."""
        p, ln = ctypes.c_void_p(0), ctypes.c_uint64(0)
        check(lib.uzk_circuit_table(self.handle, slot, int(coset), ctypes.byref(p), ctypes.byref(ln)))
        return p.value or 0, ln.value

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_circuit_release(self.handle))
            self.handle = 0


def _cs_info(fn, count: int) -> dict:
    """uzk_*_cs_info (host only): the shape of a circuit for `count` cards or players, and its public-input rows."""
    v = [ctypes.c_uint32(0) for _ in range(4)]
    check(fn(count, *[ctypes.byref(x) for x in v], None))
    rows = np.zeros(v[3].value, dtype=np.uint32)
    check(fn(count, None, None, None, None, rows.ctypes.data_as(ctypes.c_void_p)))
    return dict(size=v[0].value, n=v[1].value, num_vars=v[2].value, pi_count=v[3].value, pi_rows=rows)


def shuffle_cs_info(cards: int) -> dict:
    """uzk_shuffle_cs_info (host only): the shape of zshuffle's circuit for a deck of `cards`, and its public-input rows."""
    return _cs_info(lib.uzk_shuffle_cs_info, cards)


class _CsCircuit(Circuit):
    """What ShuffleCircuit and MatchCircuit share: a circuit the library lays out itself from a count (cards, players)."""

    def _create(self, info: dict, d, create, n_commitments: int, lagrange_bases, blind_bases, k, precompute, group_gen) -> None:
        """Fills the fields every uzk_*_circuit_desc has into `d` (the count is the caller's), creates the circuit, keeps its shape."""
        n = info["n"]
        d.precompute = int(precompute)
        lag = np.ascontiguousarray(lagrange_bases, dtype=np.uint64).reshape(-1, 8)
        bb = np.ascontiguousarray(blind_bases, dtype=np.uint64).reshape(-1, 8)
        assert lag.shape[0] == n and bb.shape[0] == 6, "n Lagrange bases and 6 blind bases"
        d.lagrange_bases, d.blind_bases = lag.ctypes.data, bb.ctypes.data
        kk = np.ascontiguousarray(k, dtype=np.uint64).reshape(5, 4)
        gg = np.ascontiguousarray(domain_group_gen(n) if group_gen is None else group_gen, dtype=np.uint64).reshape(4)
        for j in range(5):
            for w in range(4):
                d.k[j][w] = int(kk[j, w])
        for w in range(4):
            d.group_gen[w] = int(gg[w])
        h = ctypes.c_uint64(0)
        self.commitments = np.zeros((n_commitments, 12), dtype=np.uint64)
        check(create(ctypes.byref(d), ctypes.byref(h), _ptr(self.commitments)))
        self.handle, self.n = h.value, n
        self.size, self.num_vars, self.pi_rows = info["size"], info["num_vars"], info["pi_rows"]

    def _test_tables(self, tables: int, call):
        """(wiring [5, n], permutation [5, n], evaluation vectors [tables, n, 4]) through call(wiring, perm, evals)."""
        wiring, perm = np.zeros((5, self.n), dtype=np.uint32), np.zeros((5, self.n), dtype=np.uint32)
        evals = np.zeros((tables, self.n, 4), dtype=np.uint64)
        vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        check(call(vp(wiring), vp(perm), _ptr(evals)))
        return wiring, perm, evals


class ShuffleCircuit(_CsCircuit):
    """uzk_shuffle_circuit_create: zshuffle's circuit for a deck of `cards`, laid out and preprocessed on the device.  A Circuit in
    every respect (the rounds, info, table, release take it); `commitments` are the 32 of the verifier key ([32, 12] Jacobian)."""

    def __init__(self, cards: int, lagrange_bases: np.ndarray, blind_bases: np.ndarray, k: np.ndarray, precompute: bool = False, group_gen=None):
        d = N.ShuffleCircuitDesc()
        d.cards = cards
        self._create(shuffle_cs_info(cards), d, lib.uzk_shuffle_circuit_create, N.SHUFFLE_CS_KEY_COMMITMENTS, lagrange_bases, blind_bases, k,
                     precompute, group_gen)
        self.shuffle, self.n_slots, self.cards = True, N.CIRCUIT_SLOTS, cards

    def set_key(self, key: "RemarkKey") -> np.ndarray:
        """uzk_shuffle_circuit_set_key: the game's public-key tables from the key's T_pk; returns their 12 commitments [12, 12]."""
        cms = np.zeros((12, 12), dtype=np.uint64)
        check(lib.uzk_shuffle_circuit_set_key(self.handle, key.handle, _ptr(cms)))
        return cms

    def witness_batch(self, key: "RemarkKey", e1, e2, digits, perms, d_witness: int, d_wsel: int):
        """uzk_shuffle_witness_batch: e1, e2 [batch, cards, 8]; digits uint8 [batch, cards, 84]; perms uint32 [batch, cards] or None;
        d_witness / d_wsel: device addresses of batch x 5n / 3n elements.  Returns (pi_values [batch, 8 cards, 4], e1_out, e2_out
        [batch, cards, 8])."""
        a = np.ascontiguousarray(e1, dtype=np.uint64)
        cards = a.shape[-2] if a.ndim >= 2 else self.cards             # the decks' own size: the library refuses any but the circuit's
        a = a.reshape(-1, cards, 8)
        c = np.ascontiguousarray(e2, dtype=np.uint64).reshape(-1, cards, 8)
        batch = a.shape[0]
        dg = np.ascontiguousarray(digits, dtype=np.uint8).reshape(-1, cards, N.REMARK_ITERATIONS)
        pm = None if perms is None else np.ascontiguousarray(perms, dtype=np.uint32).reshape(-1, cards)
        assert c.shape[0] == batch and dg.shape[0] == batch and (pm is None or pm.shape[0] == batch), "one e2, digit row and perm per deck"
        pi = np.zeros((max(batch, 1), 8 * cards, 4), dtype=np.uint64)
        o1, o2 = np.zeros((max(batch, 1), cards, 8), dtype=np.uint64), np.zeros((max(batch, 1), cards, 8), dtype=np.uint64)
        vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        check(lib.uzk_shuffle_witness_batch(self.handle, key.handle, _ptr(a), _ptr(c), vp(dg), None if pm is None else vp(pm), cards, batch,
                                            ctypes.c_void_p(d_witness), ctypes.c_void_p(d_wsel), _ptr(pi), _ptr(o1), _ptr(o2)))
        return pi[:batch], o1[:batch], o2[:batch]

    def test_tables(self, key: "RemarkKey" = None):
        """uzk_test_shuffle_cs_tables (test hook): (wiring [5, n], permutation [5, n], evaluation vectors [44, n, 4])."""
        return self._test_tables(N.SHUFFLE_CS_TABLES, lambda *out: lib.uzk_test_shuffle_cs_tables(self.handle, key.handle if key is not None else 0, *out))


def match_cs_info(players: int) -> dict:
    """uzk_match_cs_info (host only): the shape of zmatchmaking's circuit for `players`, and its public-input rows."""
    return _cs_info(lib.uzk_match_cs_info, players)


class MatchCircuit(_CsCircuit):
    """uzk_match_circuit_create: zmatchmaking's circuit for `players`, laid out and preprocessed on the device.  A Circuit without the
    shuffle feature in every respect (the rounds, info, table, release take it); `commitments` are the 19 of the verifier key
    ([19, 12] Jacobian: cm_q (9), cm_s (5), cm_qb, cm_prk (4))."""

    def __init__(self, players: int, lagrange_bases: np.ndarray, blind_bases: np.ndarray, k: np.ndarray, precompute: bool = False, group_gen=None):
        d = N.MatchCircuitDesc()
        d.players = players
        self._create(match_cs_info(players), d, lib.uzk_match_circuit_create, N.MATCH_CS_KEY_COMMITMENTS, lagrange_bases, blind_bases, k,
                     precompute, group_gen)
        self.shuffle, self.n_slots, self.players = False, CS_QPK, players

    def witness_batch(self, inputs, seeds, randoms, d_witness: int):
        """uzk_match_witness_batch: inputs [batch, players, 4]; seeds, randoms [batch, 4]; d_witness: the device address of batch x 5n
        elements.  Returns (pi_values [batch, 2 players + 2, 4], outputs [batch, players, 4], commitments [batch, 4])."""
        a = np.ascontiguousarray(inputs, dtype=np.uint64)
        players = a.shape[-2] if a.ndim >= 2 else self.players         # the matches' own size: the library refuses any but the circuit's
        a = a.reshape(-1, players, 4)
        batch = a.shape[0]
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, 4)
        rn = np.ascontiguousarray(randoms, dtype=np.uint64).reshape(-1, 4)
        assert sd.shape[0] == batch and rn.shape[0] == batch, "one seed and one random number per match"
        pi = np.zeros((max(batch, 1), 2 * players + 2, 4), dtype=np.uint64)
        out, cm = np.zeros((max(batch, 1), players, 4), dtype=np.uint64), np.zeros((max(batch, 1), 4), dtype=np.uint64)
        check(lib.uzk_match_witness_batch(self.handle, _ptr(a), _ptr(sd), _ptr(rn), players, batch, ctypes.c_void_p(d_witness), _ptr(pi), _ptr(out), _ptr(cm)))
        return pi[:batch], out[:batch], cm[:batch]

    def test_tables(self):
        """uzk_test_match_cs_tables (test hook): (wiring [5, n], permutation [5, n], evaluation vectors [19, n, 4])."""
        return self._test_tables(N.MATCH_CS_KEY_COMMITMENTS, lambda *out: lib.uzk_test_match_cs_tables(self.handle, *out))


def match_divrem(values, m: int):
    """uzk_test_match_divrem (test hook): the witness kernel's division of plain integers [count, 4] by m -> (quotients [count, 4], remainders)."""
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
    q, r = np.zeros_like(v), np.zeros(v.shape[0], dtype=np.uint32)
    check(lib.uzk_test_match_divrem(_ptr(v), m, v.shape[0], _ptr(q), r.ctypes.data_as(ctypes.c_void_p)))
    return q, r


def reveal_cs_info() -> dict:
    """uzk_reveal_cs_info (host only): n_vars, n_inputs, n_constraints, domain and the non-zero counts of A, B, C"""
    m, l, nc, n = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    nnz = np.zeros(3, dtype=np.uint64)
    check(lib.uzk_reveal_cs_info(ctypes.byref(m), ctypes.byref(l), ctypes.byref(nc), ctypes.byref(n), _ptr(nnz)))
    return dict(n_vars=m.value, n_inputs=l.value, n_constraints=nc.value, domain=n.value, nnz=[int(v) for v in nnz])


def reveal_cs_matrices():
    """uzk_reveal_cs_matrices (host only): three (row_ptr uint64, col uint32, val [nnz, 4]) triples in CSR for A, B, C"""
    info = reveal_cs_info()
    mats = [(np.zeros(info["n_constraints"] + 1, dtype=np.uint64), np.zeros(k, dtype=np.uint32), np.zeros((k, 4), dtype=np.uint64)) for k in info["nnz"]]
    arrs = [(ctypes.c_void_p * 3)(*[m[j].ctypes.data for m in mats]) for j in range(3)]
    check(lib.uzk_reveal_cs_matrices(*arrs))
    return mats


class RevealCircuit:
    """uzk_reveal_circuit_create: the reveal circuit's R1CS joined to the points of a Groth16 proving key (the arguments of
    Groth16Key.describe without the matrices), resident on the device.  `key` is the inner Groth16Key: it lives as long as the circuit.
    Use as a context manager, or release() it."""

    def __init__(self, alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query, b_g1_query, l_query, h_query, b_g2_query, n_vars: int = None,
                 n_inputs: int = None):
        a = np.ascontiguousarray(a_query, dtype=np.uint64).reshape(-1, 8)
        d, keep = Groth16Key.describe(a.shape[0] if n_vars is None else n_vars, N.REVEAL_CS_INPUTS if n_inputs is None else n_inputs, 0, alpha_g1, beta_g1,
                                      delta_g1, beta_g2, delta_g2, a, b_g1_query, l_query, h_query, b_g2_query, [])
        h = ctypes.c_uint64(0)
        check(lib.uzk_reveal_circuit_create(ctypes.byref(d), ctypes.byref(h)))
        del keep
        self.handle = h.value
        k = ctypes.c_uint64(0)
        check(lib.uzk_reveal_circuit_key(self.handle, ctypes.byref(k)))
        self.key = Groth16Key(k.value)
        self.n_vars = self.key.n_vars

    def witness_batch(self, sk, e1, d_z: int) -> np.ndarray:
        """uzk_reveal_witness_batch: sk [4] plain words, e1 [m, 8] wire points, d_z the device address of m x n_vars elements.
        Returns the statements [m, 6, 4]."""
        sk = np.ascontiguousarray(sk, dtype=np.uint64).reshape(4)
        e1 = np.ascontiguousarray(e1, dtype=np.uint64).reshape(-1, 8)
        st = np.zeros((max(e1.shape[0], 1), 6, 4), dtype=np.uint64)
        check(lib.uzk_reveal_witness_batch(self.handle, _ptr(sk), _ptr(e1) if e1.size else None, e1.shape[0], ctypes.c_void_p(d_z), _ptr(st)))
        return st[:e1.shape[0]]

    def prove_snark_batch(self, sk, e1, r, s):
        """uzk_reveal_prove_snark_batch: r, s [m, 4].  Returns (statements [m, 6, 4], proofs [m, 32]: A (8 words), B (16), C (8))."""
        sk = np.ascontiguousarray(sk, dtype=np.uint64).reshape(4)
        e1 = np.ascontiguousarray(e1, dtype=np.uint64).reshape(-1, 8)
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        m = e1.shape[0]
        assert r.shape[0] == m and s.shape[0] == m, "one pair of blinds per card"
        st, out = np.zeros((max(m, 1), 6, 4), dtype=np.uint64), np.zeros((max(m, 1), 32), dtype=np.uint64)
        check(lib.uzk_reveal_prove_snark_batch(self.handle, _ptr(sk), _ptr(e1) if m else None, _ptr(r) if m else None, _ptr(s) if m else None, m, _ptr(st),
                                               _ptr(out)))
        return st[:m], out[:m]

    def prove_snark_batch_finish(self, sk, e1, r, s, d_blobs: int = 0):
        """uzk_reveal_prove_snark_batch_finish: as prove_snark_batch with the proofs finished and encoded on the device.  Returns
        (statements [m, 6, 4], proofs [m, 32], blobs [m, 256] bytes); the blobs are also left at the device address d_blobs when given."""
        sk = np.ascontiguousarray(sk, dtype=np.uint64).reshape(4)
        e1 = np.ascontiguousarray(e1, dtype=np.uint64).reshape(-1, 8)
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        m = e1.shape[0]
        assert r.shape[0] == m and s.shape[0] == m, "one pair of blinds per card"
        st, out = np.zeros((max(m, 1), 6, 4), dtype=np.uint64), np.zeros((max(m, 1), 32), dtype=np.uint64)
        blobs = np.zeros((max(m, 1), N.G16_PROOF_BYTES), dtype=np.uint8)
        check(lib.uzk_reveal_prove_snark_batch_finish(self.handle, _ptr(sk), _ptr(e1) if m else None, _ptr(r) if m else None, _ptr(s) if m else None, m,
                                                      _ptr(st), _ptr(out), blobs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_blobs) if d_blobs else None))
        return st[:m], out[:m], blobs[:m]

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_reveal_circuit_release(self.handle))
            self.handle, self.key.handle = 0, 0

    def __enter__(self) -> "RevealCircuit":
        return self

    def __exit__(self, *exc) -> None:
        self.release()


class VerifierKey:
    """A verifier key resident on the device (uzk_vk_create).  Points are wire rows of 8 words ((0,0) = infinity), scalars rows of 4;
    `prefix`: the caller's transcript bytes in front of transcript_init_plonk."""

    def __init__(self, cs_size: int, cm_q, cm_s, cm_qb, cm_prk, g1_0, k, anemoi_g, anemoi_g_inv, edwards_a, root, pi_root_powers, pi_lagrange,
                 prefix: bytes = b"", cm_q_ecc=None, cm_shuffle_public_key=None, cm_shuffle_generator=None, shuffle: bool = True):
        d = N.VkDesc()
        rp = np.ascontiguousarray(pi_root_powers, dtype=np.uint64).reshape(-1, 4)
        lc = np.ascontiguousarray(pi_lagrange, dtype=np.uint64).reshape(-1, 4)
        assert rp.shape == lc.shape
        pre = np.frombuffer(bytes(prefix), dtype=np.uint8).copy()
        d.cs_size, d.n_pi, d.shuffle, d.transcript_prefix_len = cs_size, rp.shape[0], int(shuffle), pre.size
        d.transcript_prefix = pre.ctypes.data if pre.size else None
        d.pi_root_powers, d.pi_lagrange = (rp.ctypes.data, lc.ctypes.data) if rp.shape[0] else (None, None)

        def points(name, rows, count):
            a = np.ascontiguousarray(rows, dtype=np.uint64).reshape(count, 8)
            dst = getattr(d, name)
            for i in range(count):
                row = dst if count == 1 and not isinstance(dst[0], ctypes.Array) else dst[i]
                for w in range(8):
                    row[w] = int(a[i, w])
        points("cm_q", cm_q, 9); points("cm_s", cm_s, 5); points("cm_qb", cm_qb, 1); points("cm_prk", cm_prk, 4); points("g1_0", g1_0, 1)
        if shuffle:
            points("cm_q_ecc", cm_q_ecc, 1); points("cm_shuffle_public_key", cm_shuffle_public_key, 12); points("cm_shuffle_generator", cm_shuffle_generator, 12)
        kk = np.ascontiguousarray(k, dtype=np.uint64).reshape(5, 4)
        for j in range(5):
            for w in range(4):
                d.k[j][w] = int(kk[j, w])
        for name, val in (("anemoi_g", anemoi_g), ("anemoi_g_inv", anemoi_g_inv), ("edwards_a", edwards_a), ("root", root)):
            v = np.ascontiguousarray(val, dtype=np.uint64).reshape(4)
            for w in range(4):
                getattr(d, name)[w] = int(v[w])
        h = ctypes.c_uint64(0)
        check(lib.uzk_vk_create(ctypes.byref(d), ctypes.byref(h)))
        self.handle = h.value
        self.cs_size, self.n_pi, self.proof_bytes, self.device = self.info()

    def info(self):
        """(cs_size, public inputs per proof, bytes per proof, device)."""
        a, b, c, dv = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
        check(lib.uzk_vk_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(dv)))
        return a.value, b.value, c.value, dv.value

    def set_public_key(self, pk) -> None:
        a = np.ascontiguousarray(pk, dtype=np.uint64).reshape(12, 8)
        check(lib.uzk_vk_set_public_key(self.handle, _ptr(a)))

    def fold(self, proofs, pis, weights=None, want_challenges: bool = False):
        """uzk_verify_fold: proofs = m blobs (bytes, or a uint8 array [m, proof_bytes]), pis [m, n_pi, 4], weights [m, 4] or None
        (m == 1 only).  Returns (left [12], right [12], status [m]) and, when asked, the challenges [m, 7, 4]."""
        raw = np.frombuffer(bytes(proofs), dtype=np.uint8) if isinstance(proofs, (bytes, bytearray)) else np.ascontiguousarray(proofs, dtype=np.uint8)
        assert raw.size % self.proof_bytes == 0, "proofs: a whole number of %d-byte blobs" % self.proof_bytes
        m = raw.size // self.proof_bytes
        pi = np.ascontiguousarray(pis, dtype=np.uint64).reshape(m, self.n_pi, 4)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64).reshape(m, 4)
        left, right = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        status = np.zeros(max(m, 1), dtype=np.uint8)
        ch = np.zeros((m, 7, 4), dtype=np.uint64) if want_challenges else None
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        check(lib.uzk_verify_fold(self.handle, vp(raw), vp(pi), m, None if w is None else _ptr(w), _ptr(left), _ptr(right), vp(status),
                                  _ptr(ch) if want_challenges else None))
        return (left, right, status[:m], ch) if want_challenges else (left, right, status[:m])

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_vk_release(self.handle))
            self.handle = 0


class Groth16VerifierKey:
    """A Groth16 verifying key resident on the device (uzk_g16_vk_create).  alpha_g1: a wire row of 8 words, the G2 points rows of 16,
    gamma_abc_g1 [l, 8] ((0, 0) = infinity).  The G2 points are the caller's side of the pairing; they are kept here as given."""

    def __init__(self, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1):
        ic = np.ascontiguousarray(gamma_abc_g1, dtype=np.uint64).reshape(-1, 8)
        d = N.G16VkDesc()
        d.n_inputs = ic.shape[0]
        for name, val, words in (("alpha_g1", alpha_g1, 8), ("beta_g2", beta_g2, 16), ("gamma_g2", gamma_g2, 16), ("delta_g2", delta_g2, 16)):
            v = np.ascontiguousarray(val, dtype=np.uint64).reshape(words)
            dst = getattr(d, name)
            for w in range(words):
                dst[w] = int(v[w])
        d.gamma_abc_g1 = ic.ctypes.data if ic.shape[0] else None
        h = ctypes.c_uint64(0)
        check(lib.uzk_g16_vk_create(ctypes.byref(d), ctypes.byref(h)))
        self.handle = h.value
        self.beta_g2, self.gamma_g2, self.delta_g2 = (np.array(v, dtype=np.uint64).reshape(16) for v in (beta_g2, gamma_g2, delta_g2))
        self.n_inputs, self.device = self.info()

    def info(self):
        """(l, the constant one included; device)."""
        a, dv = ctypes.c_uint32(0), ctypes.c_int(0)
        check(lib.uzk_g16_vk_info(self.handle, ctypes.byref(a), ctypes.byref(dv)))
        return a.value, dv.value

    def fold(self, proofs, publics, weights=None):
        """uzk_g16_verify_fold: proofs = m blobs of 256 bytes (bytes, or a uint8 array), publics [m, l - 1, 4], weights [m, 4] or None
        (m == 1 only).  Returns (a [m, 8], b [m, 16], alpha [12], x [12], c [12], status [m])."""
        raw = np.frombuffer(bytes(proofs), dtype=np.uint8) if isinstance(proofs, (bytes, bytearray)) else np.ascontiguousarray(proofs, dtype=np.uint8)
        assert raw.size % N.G16_PROOF_BYTES == 0, "proofs: a whole number of %d-byte blobs" % N.G16_PROOF_BYTES
        m = raw.size // N.G16_PROOF_BYTES
        pub = np.ascontiguousarray(publics, dtype=np.uint64).reshape(m, self.n_inputs - 1, 4)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64).reshape(m, 4)
        a, b = np.zeros((max(m, 1), 8), dtype=np.uint64), np.zeros((max(m, 1), 16), dtype=np.uint64)
        alpha, x, c = (np.zeros(12, dtype=np.uint64) for _ in range(3))
        status = np.zeros(max(m, 1), dtype=np.uint8)
        vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        check(lib.uzk_g16_verify_fold(self.handle, vp(raw), vp(pub), m, None if w is None else _ptr(w), _ptr(a), _ptr(b), _ptr(alpha), _ptr(x), _ptr(c),
                                      vp(status)))
        return a[:m], b[:m], alpha, x, c, status[:m]

    def verify_batch(self, proofs, publics, weights=None):
        """uzk_g16_verify_batch: the arguments of `fold`; the fold, then the product of its m + 3 pairings on the device with this key's
        beta, gamma, delta.  Returns (accepted, status [m]): accepted iff every status is 0 and the product is one."""
        raw = np.frombuffer(bytes(proofs), dtype=np.uint8) if isinstance(proofs, (bytes, bytearray)) else np.ascontiguousarray(proofs, dtype=np.uint8)
        assert raw.size % N.G16_PROOF_BYTES == 0, "proofs: a whole number of %d-byte blobs" % N.G16_PROOF_BYTES
        m = raw.size // N.G16_PROOF_BYTES
        pub = np.ascontiguousarray(publics, dtype=np.uint64).reshape(m, self.n_inputs - 1, 4)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64).reshape(m, 4)
        g2 = np.ascontiguousarray(np.stack([self.beta_g2, self.gamma_g2, self.delta_g2]), dtype=np.uint64)
        status = np.zeros(max(m, 1), dtype=np.uint8)
        accepted = ctypes.c_int(0)
        vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        check(lib.uzk_g16_verify_batch(self.handle, vp(raw), vp(pub), m, None if w is None else _ptr(w), _ptr(g2), vp(status), ctypes.byref(accepted)))
        return bool(accepted.value), status[:m]

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_g16_vk_release(self.handle))
            self.handle = 0


def pairing_product(p, q, want_gt: bool = True):
    """uzk_pairing_product: p [n, 8] affine G1 wire points, q [n, 16] affine G2 wire points (zeros = infinity).  Returns (gt, is_one):
    gt [6, 2, 4] = the coefficients of w^0 .. w^5 (c0, c1 Montgomery words), the product of the n pairings after the final
    exponentiation (None when not wanted)."""
    a = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8)
    b = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 16)
    assert a.shape[0] == b.shape[0], "one G2 point per G1 point"
    n = a.shape[0]
    gt = np.zeros((6, 2, 4), dtype=np.uint64) if want_gt else None
    one = ctypes.c_int(0)
    check(lib.uzk_pairing_product(_ptr(a) if n else None, _ptr(b) if n else None, n, _ptr(gt) if want_gt else None, ctypes.byref(one)))
    return gt, bool(one.value)


def _u8(blobs, size: int) -> np.ndarray:
    raw = np.frombuffer(bytes(blobs), dtype=np.uint8) if isinstance(blobs, (bytes, bytearray)) else np.ascontiguousarray(blobs, dtype=np.uint8)
    assert raw.size % size == 0, "a whole number of %d-byte blobs" % size
    return raw.reshape(-1)


def ed_check_points(points) -> np.ndarray:
    """uzk_ed_check_points: points [n, 8] (x then y, Montgomery words).  Returns status [n]: 0 in the prime subgroup, 1 a coordinate
    word >= q, 2 off the curve, 3 on the curve outside the subgroup."""
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    status = np.zeros(max(p.shape[0], 1), dtype=np.uint8)
    check(lib.uzk_ed_check_points(_ptr(p), p.shape[0], status.ctypes.data_as(ctypes.c_void_p)))
    return status[:p.shape[0]]


def ed_mul_batch(points, scalars) -> np.ndarray:
    """uzk_ed_mul_batch: scalars [n, 4] plain 256-bit integers (little-endian words); points [n, 8], or one point [8] shared by every
    item.  Returns [n, 8] canonical affine points."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(points, dtype=np.uint64)
    shared = p.size == 8 and p.ndim == 1
    p = p.reshape(-1, 8)
    assert shared or p.shape[0] == s.shape[0], "one point per scalar, or one point [8] for all"
    out = np.zeros((max(s.shape[0], 1), 8), dtype=np.uint64)
    check(lib.uzk_ed_mul_batch(_ptr(p), 0 if shared else 1, _ptr(s), s.shape[0], _ptr(out)))
    return out[:s.shape[0]]


def ed_sum_batch(rows) -> np.ndarray:
    """uzk_ed_sum_batch: rows [k, n, 8].  Returns [n, 8]: the sum over the k rows, card by card."""
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    assert r.ndim == 3 and r.shape[2] == 8, "rows [k, n, 8]"
    out = np.zeros((max(r.shape[1], 1), 8), dtype=np.uint64)
    check(lib.uzk_ed_sum_batch(_ptr(r), r.shape[0], r.shape[1], _ptr(out)))
    return out[:r.shape[1]]


def ed_unmask_batch(e2, reveals) -> np.ndarray:
    """uzk_ed_unmask_batch: e2 [n, 8], reveals [k, n, 8].  Returns [n, 8]: e2_j minus the k reveals of card j."""
    r = np.ascontiguousarray(reveals, dtype=np.uint64)
    assert r.ndim == 3 and r.shape[2] == 8, "reveals [k, n, 8]"
    e = np.ascontiguousarray(e2, dtype=np.uint64).reshape(-1, 8)
    assert e.shape[0] == r.shape[1], "one e2 per card"
    out = np.zeros((max(r.shape[1], 1), 8), dtype=np.uint64)
    check(lib.uzk_ed_unmask_batch(_ptr(e), _ptr(r), r.shape[0], r.shape[1], _ptr(out)))
    return out[:r.shape[1]]


def cp_reveal_prove_batch(sk, e1, omegas, anemoi: bool = False):
    """uzk_cp_reveal_prove_batch (anemoi: uzk_cp_reveal_prove0_batch, the zk-friendly challenge): sk [4] and omegas [m, 4] plain
    integers below L, e1 [m, 8] subgroup points.  Returns (reveal [m, 8], pk [8], proofs: uint8 [m, 160])."""
    k = np.ascontiguousarray(sk, dtype=np.uint64).reshape(4)
    p = np.ascontiguousarray(e1, dtype=np.uint64).reshape(-1, 8)
    w = np.ascontiguousarray(omegas, dtype=np.uint64).reshape(-1, 4)
    assert p.shape[0] == w.shape[0], "one omega per card"
    m = p.shape[0]
    reveal, pk = np.zeros((max(m, 1), 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    proofs = np.zeros((max(m, 1), N.CP_PROOF_BYTES), dtype=np.uint8)
    call = lib.uzk_cp_reveal_prove0_batch if anemoi else lib.uzk_cp_reveal_prove_batch
    check(call(_ptr(k), _ptr(p), _ptr(w), m, _ptr(reveal), _ptr(pk), proofs.ctypes.data_as(ctypes.c_void_p)))
    return reveal[:m], pk, proofs[:m]


def cp_reveal_verify_batch(statements, proofs, want_challenges: bool = False, anemoi: bool = False):
    """uzk_cp_reveal_verify_batch (anemoi: uzk_cp_reveal_verify0_batch): statements [m, 6, 4] (e1, reveal, pk: x and y each -- the public signals of the Groth16 reveal proof
    of the same statement), proofs m blobs of 160 bytes.  Returns verdict [m] (0 accepted, 1 .. 5 the first failing check), and with
    want_challenges also c [m, 4] as plain integers."""
    raw = _u8(proofs, N.CP_PROOF_BYTES)
    m = raw.size // N.CP_PROOF_BYTES
    st = np.ascontiguousarray(statements, dtype=np.uint64).reshape(m, 6, 4)
    verdict = np.zeros(max(m, 1), dtype=np.uint8)
    ch = np.zeros((max(m, 1), 4), dtype=np.uint64) if want_challenges else None
    vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    call = lib.uzk_cp_reveal_verify0_batch if anemoi else lib.uzk_cp_reveal_verify_batch
    check(call(_ptr(st), vp(raw), m, vp(verdict), _ptr(ch) if want_challenges else None))
    return (verdict[:m], ch[:m]) if want_challenges else verdict[:m]


def anemoi_permutations(length: int, out_len: int = 0) -> int:
    """uzk_anemoi_permutations: how many permutations one item of `length` inputs runs; out_len = 0: a hash."""
    return int(lib.uzk_anemoi_permutations(length, out_len))


def anemoi_permute_batch(states) -> np.ndarray:
    """uzk_anemoi_permute_batch: states [n, 4, 4] (x0 x1 y0 y1, Montgomery words).  Returns [n, 4, 4]."""
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 4, 4)
    out = np.zeros((max(s.shape[0], 1), 4, 4), dtype=np.uint64)
    check(lib.uzk_anemoi_permute_batch(_ptr(s), s.shape[0], _ptr(out)))
    return out[:s.shape[0]]


def _anemoi_inputs(inputs, length):
    x = np.ascontiguousarray(inputs, dtype=np.uint64)
    if length is None:
        assert x.ndim == 3 and x.shape[2] == 4, "inputs [n, len, 4] (or pass length= with anything that reshapes to it)"
        length = x.shape[1]
    n = x.size // (4 * length) if length else (x.shape[0] if x.ndim else 0)
    return x.reshape(n, length, 4), n, length


def anemoi_hash_batch(inputs, length: int = None, want_trace: bool = False):
    """uzk_anemoi_hash_batch: inputs [n, len, 4] (len = 0: [n, 0, 4]).  Returns out [n, 4], and with want_trace also the trace
    [n, P, 64, 4]: per permutation before (4 elements), the 14 rounds (56), after (4)."""
    x, n, length = _anemoi_inputs(inputs, length)
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    perms = anemoi_permutations(length, 0)
    tr = np.zeros((max(n, 1), perms, N.ANEMOI_TRACE_ELEMS, 4), dtype=np.uint64) if want_trace else None
    check(lib.uzk_anemoi_hash_batch(_ptr(x) if x.size else None, length, n, _ptr(out), _ptr(tr) if want_trace else None))
    return (out[:n], tr[:n]) if want_trace else out[:n]


def anemoi_stream_batch(inputs, out_len: int, length: int = None, want_trace: bool = False):
    """uzk_anemoi_stream_batch: inputs [n, len, 4].  Returns out [n, out_len, 4], and with want_trace also the trace [n, P, 64, 4]."""
    x, n, length = _anemoi_inputs(inputs, length)
    out = np.zeros((max(n, 1), max(out_len, 1), 4), dtype=np.uint64)
    perms = anemoi_permutations(length, out_len)
    tr = np.zeros((max(n, 1), perms, N.ANEMOI_TRACE_ELEMS, 4), dtype=np.uint64) if want_trace else None
    check(lib.uzk_anemoi_stream_batch(_ptr(x) if x.size else None, length, n, out_len, _ptr(out), _ptr(tr) if want_trace else None))
    return (out[:n], tr[:n]) if want_trace else out[:n]


class RemarkKey:
    """uzk_remark_key_create: the remask tables of one joint key, T_pk[i][j] = (j + 1) 16^i pk, resident on the current context's
    device for the length of a game.  A context manager: the key is released on exit."""

    def __init__(self, pk):
        p = np.ascontiguousarray(pk, dtype=np.uint64).reshape(8)
        h = ctypes.c_uint64(0)
        check(lib.uzk_remark_key_create(_ptr(p), ctypes.byref(h)))
        self.handle = h.value

    def tables(self, want_pk: bool = True, want_gen: bool = True):
        """uzk_remark_key_tables: (T_pk, T_G), each [84, 4, 3, 4] -- x, y, d x y of every entry -- or None where not wanted"""
        shape = (N.REMARK_ITERATIONS, 4, 3, 4)
        tp = np.zeros(shape, dtype=np.uint64) if want_pk else None
        tg = np.zeros(shape, dtype=np.uint64) if want_gen else None
        check(lib.uzk_remark_key_tables(self.handle, _ptr(tp) if want_pk else None, _ptr(tg) if want_gen else None))
        return tp, tg

    def remark_batch(self, e1, e2, digits, perm=None, want_trace: bool = False):
        """uzk_remark_batch: e1, e2 [n, 8]; digits uint8 [n, 84]; perm uint32 [n] or None.  Returns (e1_out [n, 8], e2_out [n, 8] in
        output order, trace [n, 84, 4, 4] in input order or None)."""
        a = np.ascontiguousarray(e1, dtype=np.uint64).reshape(-1, 8)
        c = np.ascontiguousarray(e2, dtype=np.uint64).reshape(-1, 8)
        n = a.shape[0]
        d = np.ascontiguousarray(digits, dtype=np.uint8).reshape(-1, N.REMARK_ITERATIONS)
        assert c.shape[0] == n and d.shape[0] == n, "one e2 and 84 digits per card"
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32).reshape(-1)
        assert pm is None or pm.size == n, "one perm entry per card"
        o1, o2 = np.zeros((max(n, 1), 8), dtype=np.uint64), np.zeros((max(n, 1), 8), dtype=np.uint64)
        tr = np.zeros((max(n, 1), N.REMARK_ITERATIONS, 4, 4), dtype=np.uint64) if want_trace else None
        vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        check(lib.uzk_remark_batch(self.handle, _ptr(a), _ptr(c), vp(d), None if pm is None else vp(pm), n, _ptr(o1), _ptr(o2), _ptr(tr) if want_trace else None))
        return o1[:n], o2[:n], (tr[:n] if want_trace else None)

    def release(self) -> None:
        if self.handle:
            check(lib.uzk_remark_key_release(self.handle))
            self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.release()


def cp_mask_prove_batch(pk, cards, rs, omegas):
    """uzk_cp_mask_prove_batch: pk [8]; cards [m, 8]; rs, omegas [m, 4] plain integers.  Returns (e1 [m, 8], e2 [m, 8], proofs: uint8
    [m, 160])."""
    k = np.ascontiguousarray(pk, dtype=np.uint64).reshape(8)
    p = np.ascontiguousarray(cards, dtype=np.uint64).reshape(-1, 8)
    r = np.ascontiguousarray(rs, dtype=np.uint64).reshape(-1, 4)
    w = np.ascontiguousarray(omegas, dtype=np.uint64).reshape(-1, 4)
    m = p.shape[0]
    assert r.shape[0] == m and w.shape[0] == m, "one r and one omega per card"
    e1, e2 = np.zeros((max(m, 1), 8), dtype=np.uint64), np.zeros((max(m, 1), 8), dtype=np.uint64)
    proofs = np.zeros((max(m, 1), N.CP_PROOF_BYTES), dtype=np.uint8)
    check(lib.uzk_cp_mask_prove_batch(_ptr(k), _ptr(p), _ptr(r), _ptr(w), m, _ptr(e1), _ptr(e2), proofs.ctypes.data_as(ctypes.c_void_p)))
    return e1[:m], e2[:m], proofs[:m]


def cp_mask_verify_batch(pk, cards, e1, e2, proofs, want_challenges: bool = False):
    """uzk_cp_mask_verify_batch: pk [8]; cards, e1, e2 [m, 8]; proofs m blobs of 160 bytes.  Returns verdict [m] (0 accepted, 1 .. 5 the
    first failing check), and with want_challenges also c [m, 4] as plain integers."""
    raw = _u8(proofs, N.CP_PROOF_BYTES)
    m = raw.size // N.CP_PROOF_BYTES
    k = np.ascontiguousarray(pk, dtype=np.uint64).reshape(8)
    arrs = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 8) for x in (cards, e1, e2)]
    assert all(x.shape[0] == m for x in arrs), "one card, one e1 and one e2 per proof"
    verdict = np.zeros(max(m, 1), dtype=np.uint8)
    ch = np.zeros((max(m, 1), 4), dtype=np.uint64) if want_challenges else None
    vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    check(lib.uzk_cp_mask_verify_batch(_ptr(k), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), vp(raw), m, vp(verdict), _ptr(ch) if want_challenges else None))
    return (verdict[:m], ch[:m]) if want_challenges else verdict[:m]


def fq12_kat(op: int, a, b=None) -> np.ndarray:
    """uzk_test_fq12_kat (test hook): a, b [n, 6, 2, 4] wire elements of Fq12."""
    x = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 6, 2, 4)
    y = x if b is None else np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 6, 2, 4)
    out = np.zeros_like(x)
    check(lib.uzk_test_fq12_kat(op, _ptr(x), _ptr(y), _ptr(out), x.shape[0]))
    return out


def miller_loops(p, q) -> np.ndarray:
    """uzk_test_miller (test hook): the n Miller values [n, 6, 2, 4] of the pairs, before the product and the final exponentiation."""
    a = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8)
    b = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 16)
    out = np.zeros((a.shape[0], 6, 2, 4), dtype=np.uint64)
    check(lib.uzk_test_miller(_ptr(a), _ptr(b), a.shape[0], _ptr(out)))
    return out


def keccak256_device(messages) -> list:
    """uzk_test_keccak256 (test hook): the digests of the messages by the device's transcript sponge."""
    offs = np.zeros(len(messages) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in messages])
    blob = np.frombuffer(b"".join(messages) + b"\0", dtype=np.uint8).copy()
    out = np.zeros((len(messages), 32), dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib.uzk_test_keccak256(vp(blob), vp(offs), len(messages), vp(out)))
    return [bytes(r) for r in out]


def preprocess_tables_device(srs: Srs, evals: np.ndarray, k1=None, want_coset: bool = False, want_commit: bool = True):
    """uzk_preprocess_tables: [count, n, 4] evaluation vectors -> (polys [count, n, 4], lens, coset [count, 6n, 4] | None,
    commitments [count, 12] | None).  Without commitments the SRS handle is not looked at (srs may be None)."""
    e = np.ascontiguousarray(evals, dtype=np.uint64)
    cnt, n = e.shape[0], e.shape[1]
    polys = np.zeros((cnt, n, 4), dtype=np.uint64)
    lens = np.zeros(cnt, dtype=np.uint64)
    coset = np.zeros((cnt, 6 * n, 4), dtype=np.uint64) if want_coset else None
    cms = np.zeros((cnt, 12), dtype=np.uint64) if want_commit else None
    check(lib.uzk_preprocess_tables(srs.handle if srs is not None else 0, n, cnt, _ptr(e), _ptr(_fr4(k1)) if k1 is not None else None, _ptr(polys), _ptr(lens),
                                    _ptr(coset) if want_coset else None, _ptr(cms) if want_commit else None))
    return polys, lens, coset, cms


def coalesce_config(max_lanes: int = 8, gather_wait_us: int = 0, straggler_wait_us: int = 0, groups: int = 0) -> None:
    """uzk_coalesce_config: how provers of one proof made from now on are shared (max_lanes <= 1: not at all; 0 = the defaults)."""
    check(lib.uzk_coalesce_config(max_lanes, gather_wait_us, straggler_wait_us, groups))


def coalesce_stats() -> dict:
    """uzk_coalesce_stats since the last coalesce_config."""
    a = (ctypes.c_uint64 * 16)()
    check(lib.uzk_coalesce_stats(a))
    return dict(rounds=a[0], calls=a[1], widest=a[2], moved_out=a[3], groups=a[4], gap_us_avg=(a[5] / a[6] if a[6] else 0.0),
                gather_us_avg=(a[7] / a[4] if a[4] else 0.0), group_sizes=[a[8 + i] for i in range(8)])


class Prover:
    """The device buffers of `batch` proofs in lockstep (uzk_prover_create) and the five rounds.  shared=True with batch == 1 is
    the library's default kind -- a prover of one proof whose concurrent round calls the library may run together with other
    threads' (uzk_coalesce_config); shared=False (uzk_prover_create_private) owns its lanes and can show its buffers."""

    def __init__(self, n: int, batch: int = 1, shared: bool = True):
        h = ctypes.c_uint64(0)
        check((lib.uzk_prover_create if shared else lib.uzk_prover_create_private)(n, batch, ctypes.byref(h)))
        self.handle, self.n, self.batch = h.value, n, batch

    def round1(self, circuit: Circuit, witness, wsel, pi_index, pi_value, hiding, blinds, on_device: bool = False) -> np.ndarray:
        """witness / wsel: arrays [batch, 5n, 4] / [batch, 3n, 4] (or None), or device addresses with on_device."""
        B, n_first = self.batch, 8 if wsel is not None else 5
        if on_device:
            w_ptr, s_ptr = ctypes.c_void_p(witness), (ctypes.c_void_p(wsel) if wsel is not None else None)
        else:
            w = np.ascontiguousarray(witness, dtype=np.uint64).reshape(B, 5 * self.n, 4)
            s = None if wsel is None else np.ascontiguousarray(wsel, dtype=np.uint64).reshape(B, 3 * self.n, 4)
            w_ptr, s_ptr = _ptr(w), (None if s is None else _ptr(s))
        idx = np.ascontiguousarray(pi_index, dtype=np.uint32).reshape(-1)
        val = np.ascontiguousarray(pi_value, dtype=np.uint64).reshape(B, idx.size, 4) if idx.size else np.zeros((B, 0, 4), dtype=np.uint64)
        hd = np.ascontiguousarray(hiding, dtype=np.uint32).reshape(n_first)
        bl = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(B, n_first, 3, 4)
        out = np.zeros((B * n_first, 12), dtype=np.uint64)
        check(lib.uzk_prove_round1(self.handle, circuit.handle, w_ptr, s_ptr, int(on_device), idx.ctypes.data_as(ctypes.c_void_p) if idx.size else None,
                                   _ptr(val) if idx.size else None, idx.size, hd.ctypes.data_as(ctypes.c_void_p), _ptr(bl), _ptr(out)))
        return out

    def round2(self, beta, gamma, blinds_z) -> np.ndarray:
        B = self.batch
        out = np.zeros((B, 12), dtype=np.uint64)
        check(lib.uzk_prove_round2(self.handle, _ptr(_frs(beta, B)), _ptr(_frs(gamma, B)), _ptr(_frs(blinds_z, 3 * B)), _ptr(out)))
        return out

    def round3(self, alpha, t_rands) -> np.ndarray:
        B = self.batch
        out = np.zeros((5 * B, 12), dtype=np.uint64)
        check(lib.uzk_prove_round3(self.handle, _ptr(_frs(alpha, B)), _ptr(_frs(t_rands, 5 * B)), _ptr(out)))
        return out

    def round4(self, zeta, shuffle: bool = True) -> np.ndarray:
        B, per = self.batch, 19 if shuffle else 15
        out = np.zeros((B * per, 4), dtype=np.uint64)
        check(lib.uzk_prove_round4(self.handle, _ptr(_frs(zeta, B)), _ptr(out), B * per))
        return out

    def round5(self, r_scalars, alpha_zeta, alpha_zeta_omega) -> np.ndarray:
        B = self.batch
        rs = np.ascontiguousarray(r_scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((2 * B, 12), dtype=np.uint64)
        check(lib.uzk_prove_round5(self.handle, _ptr(rs), rs.shape[0], _ptr(_frs(alpha_zeta, B)), _ptr(_frs(alpha_zeta_omega, B)), _ptr(out)))
        return out

    def buffer(self, which: int):
        """(device address, elements per proof) of a prover buffer (PB_*)."""
        p, ln = ctypes.c_void_p(0), ctypes.c_uint64(0)
        check(lib.uzk_prover_buffer(self.handle, which, ctypes.byref(p), ctypes.byref(ln)))
        return p.value or 0, ln.value

    def download(self, which: int, proof: int = 0) -> np.ndarray:
        p, ln = self.buffer(which)
        return dev_download(p + 32 * ln * proof, (ln, 4))

    def destroy(self) -> None:
        if self.handle:
            check(lib.uzk_prover_destroy(self.handle))
            self.handle = 0


def _frs(a, count: int) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(count, 4)
