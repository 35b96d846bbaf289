"""Host-side mirror of the reference's polynomial layer for the hot path, over the C ABI.

  FpPolynomial                 uzkge/src/poly_commit/field_polynomial.rs:13-17, 86-90, 154-159,
                               198-209 (eval), 470-477 (mul_var), 554-607 (domains, fft wrappers)
  KZGCommitmentSchemeBN254     uzkge/src/poly_commit/kzg_poly_commitment.rs:170-313
                               (from_unchecked_bytes :228-264, commit :278-293,
                                apply_blind_factors :299-313)

Same names, argument meaning and error behaviour as the Rust (errors are `UzkgeError` with the
reference's variant names).  All heavy work goes to the GPU through `backend`; what stays here is
what stays in Rust in the real integration: trimming, zero-padding, domain choice, length checks.
Coefficients are numpy uint64 arrays [n, 4] in the wire format (Montgomery, 4 LE limbs).
"""
from __future__ import annotations

import os
import struct
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from . import backend as B
from .errors import UzkgeError

FR_MODULUS = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FQ_MODULUS = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_MASK64 = (1 << 64) - 1


def _to_wire(x: int, mod: int) -> np.ndarray:
    v = (x << 256) % mod
    return np.array([(v >> (64 * i)) & _MASK64 for i in range(4)], dtype=np.uint64)


def _wire_int(row: np.ndarray) -> int:
    return sum(int(row[i]) << (64 * i) for i in range(4))


def fr_from_int(x: int) -> np.ndarray:
    """canonical integer -> Montgomery wire limbs."""
    return _to_wire(x % FR_MODULUS, FR_MODULUS)


def fr_to_int(row: np.ndarray) -> int:
    return _wire_int(row) * pow(1 << 256, -1, FR_MODULUS) % FR_MODULUS


def fr_neg(rows: np.ndarray) -> np.ndarray:
    """-x on wire-format rows (Montgomery form is linear: r - x)."""
    out = np.zeros_like(rows)
    for i, row in enumerate(rows.reshape(-1, 4)):
        v = _wire_int(row)
        v = (FR_MODULUS - v) % FR_MODULUS
        out.reshape(-1, 4)[i] = [(v >> (64 * k)) & _MASK64 for k in range(4)]
    return out


class FpPolynomial:
    """Dense polynomial over BN254 Fr, coefficients low to high."""

    def __init__(self, coefs: np.ndarray):
        self.coefs = np.ascontiguousarray(coefs, dtype=np.uint64).reshape(-1, 4)

    # -- construction -------------------------------------------------------------------------
    @classmethod
    def from_coefs(cls, coefs: np.ndarray) -> "FpPolynomial":
        """Trims trailing zeros like the reference (field_polynomial.rs:86-90,154-159); the zero
        polynomial keeps one zero coefficient."""
        c = np.ascontiguousarray(coefs, dtype=np.uint64).reshape(-1, 4)
        nz = np.flatnonzero(c.any(axis=1))
        keep = int(nz[-1]) + 1 if nz.size else 1
        if c.shape[0] == 0:
            c = np.zeros((1, 4), dtype=np.uint64)
        return cls(c[:keep].copy())

    @classmethod
    def from_ints(cls, ints: Sequence[int]) -> "FpPolynomial":
        return cls.from_coefs(np.stack([fr_from_int(x) for x in ints]) if len(ints) else np.zeros((0, 4), np.uint64))

    def get_coefs_ref(self) -> np.ndarray:
        return self.coefs

    def degree(self) -> int:
        nz = np.flatnonzero(self.coefs.any(axis=1))
        return int(nz[-1]) if nz.size else 0

    # -- small host-side helpers ---------------------------------------------------------------
    def eval(self, point: int) -> int:
        """Horner (field_polynomial.rs:198-209), canonical ints."""
        acc = 0
        for row in self.coefs[::-1]:
            acc = (acc * point + fr_to_int(row)) % FR_MODULUS
        return acc

    # -- domains (field_polynomial.rs:554-567) ------------------------------------------------
    @staticmethod
    def evaluation_domain(num_coeffs: int) -> Optional[int]:
        assert num_coeffs > 0 and num_coeffs & (num_coeffs - 1) == 0
        return num_coeffs if B.domain_supported(num_coeffs) else None

    @staticmethod
    def quotient_evaluation_domain(num_coeffs: int) -> Optional[int]:
        m = num_coeffs // 3 if num_coeffs % 3 == 0 else num_coeffs
        assert num_coeffs > 0 and m & (m - 1) == 0
        return num_coeffs if B.domain_supported(num_coeffs) else None

    # -- transforms ---------------------------------------------------------------------------
    def _padded(self, n: int) -> np.ndarray:
        out = np.zeros((n, 4), dtype=np.uint64)
        out[: self.coefs.shape[0]] = self.coefs
        return out

    def fft(self, num_coeffs: int) -> Optional[np.ndarray]:
        """field_polynomial.rs:570-580."""
        assert num_coeffs > self.degree()
        dom = (self.evaluation_domain(num_coeffs) if num_coeffs & (num_coeffs - 1) == 0
               else self.quotient_evaluation_domain(num_coeffs))
        if dom is None:
            return None
        return self.fft_with_domain(dom)

    def fft_with_domain(self, domain: int) -> np.ndarray:
        """`domain.fft(&self.coefs)` (field_polynomial.rs:583-586): zero-pad, natural order."""
        assert domain > self.degree()
        return B.ntt(self._padded(domain)[:domain] if self.coefs.shape[0] <= domain else self.coefs[:domain])

    def coset_fft_with_domain(self, domain: int, k: np.ndarray) -> np.ndarray:
        """fft of p(kX) (field_polynomial.rs:589-591); the k^j scaling is fused on the device."""
        assert domain > self.degree()
        return B.ntt(self._padded(domain), coset_shift=k)

    @classmethod
    def ifft_with_domain(cls, domain: int, values: np.ndarray) -> "FpPolynomial":
        """`domain.ifft(values)` then from_coefs (field_polynomial.rs:594-597)."""
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        buf = np.zeros((domain, 4), dtype=np.uint64)
        buf[: v.shape[0]] = v
        return cls.from_coefs(B.ntt(buf, inverse=True))

    @classmethod
    def coset_ifft_with_domain(cls, domain: int, values: np.ndarray, k_inv: np.ndarray) -> "FpPolynomial":
        """ifft then mul_var(k_inv) (field_polynomial.rs:601-607)."""
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        buf = np.zeros((domain, 4), dtype=np.uint64)
        buf[: v.shape[0]] = v
        return cls.from_coefs(B.ntt(buf, inverse=True, coset_shift=k_inv))

    def __eq__(self, other) -> bool:
        return isinstance(other, FpPolynomial) and np.array_equal(
            FpPolynomial.from_coefs(self.coefs).coefs, FpPolynomial.from_coefs(other.coefs).coefs)


def parse_srs_g1_wire(data: bytes) -> np.ndarray:
    """The G1 section of a reference SRS blob as wire-format affine points [len, 8] (host only): u32 len_g1 | u32 len_g2 |
    len_g1 x (x LE32 || y LE32, flags in the top two bits of the last byte) | G2 points (kzg_poly_commitment.rs:228-264)."""
    if len(data) < 8:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "DeserializationError: short SRS blob")
    len1, _len2 = struct.unpack_from("<II", data, 0)
    if len(data) < 8 + 64 * len1:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "DeserializationError: truncated G1 section")
    out = np.zeros((len1, 8), dtype=np.uint64)
    for i in range(len1):
        off = 8 + 64 * i
        x = int.from_bytes(data[off:off + 32], "little")
        yb = bytearray(data[off + 32:off + 64])
        flags = yb[31] & 0xC0
        yb[31] &= 0x3F
        if flags & 0x40:
            continue                       # infinity -> (0, 0)
        y = int.from_bytes(bytes(yb), "little")
        out[i, :4] = _to_wire(x, FQ_MODULUS)
        out[i, 4:] = _to_wire(y, FQ_MODULUS)
    return out


def srs_g1_wire_to_bytes(g1_wire: np.ndarray, len_g2: int = 0, g2_bytes: bytes = b"") -> bytes:
    """The writer for parse_srs_g1_wire (host only; `to_unchecked_bytes`, kzg_poly_commitment.rs:228-264): u32 len_g1 | u32 len_g2 |
    64 B per point -- canonical little-endian x and y out of the Montgomery wire words, bit 7 of the last byte set when
    y > (p - 1) / 2, bit 6 for infinity over zero coordinates -- then the G2 block, which this library never interprets and
    passes through as bytes."""
    pts = np.ascontiguousarray(g1_wire, dtype=np.uint64).reshape(-1, 8)
    r_inv = pow(1 << 256, -1, FQ_MODULUS)
    half = (FQ_MODULUS - 1) // 2
    out = bytearray(struct.pack("<II", pts.shape[0], len_g2))
    for row in pts:
        if not row.any():
            out += bytes(63) + b"\x40"
            continue
        x = _wire_int(row[:4]) * r_inv % FQ_MODULUS
        y = _wire_int(row[4:]) * r_inv % FQ_MODULUS
        yb = bytearray(y.to_bytes(32, "little"))
        if y > half:
            yb[31] |= 0x80
        out += x.to_bytes(32, "little") + bytes(yb)
    return bytes(out) + bytes(g2_bytes)


def srs_params_wire(srs_blob: bytes, size: int) -> np.ndarray:
    """load_srs_params (uzkge/src/gen_params/mod.rs:151-183) as a wire array (host only): powers 0..2050, the identity
    up to `size`, then the three padding powers size, size + 1, size + 2."""
    if size > 16384:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "ParameterError: size exceeds the embedded SRS")
    g1 = parse_srs_g1_wire(srs_blob)
    out = np.zeros((max(size + 3, 2051), 8), dtype=np.uint64)
    out[:2051] = g1[:2051]
    pad = {4096: 2051, 8192: 2054, 16384: 2057}.get(size)
    if pad is not None:
        out[size:size + 3] = g1[pad:pad + 3]
    return out


class KZGCommitmentSchemeBN254:
    """KZG over BN254 with the G1 powers resident on the GPU."""

    def __init__(self, g1_wire: np.ndarray):
        self.public_parameter_group_1 = np.ascontiguousarray(g1_wire, dtype=np.uint64).reshape(-1, 8)
        self._srs = B.Srs.from_host(self.public_parameter_group_1)

    @classmethod
    def from_unchecked_bytes(cls, data: bytes) -> "KZGCommitmentSchemeBN254":
        """Reference SRS blob: u32 len_g1 | u32 len_g2 | len_g1 x (x LE32 || y LE32, flags in the
        top two bits of the last byte) | G2 points (kzg_poly_commitment.rs:228-264).  The G2 part is
        only used by the verifier and is ignored here."""
        return cls(parse_srs_g1_wire(data))

    def max_degree(self) -> int:
        return self.public_parameter_group_1.shape[0] - 1

    def commit(self, polynomial: FpPolynomial) -> np.ndarray:
        """C = sum_i coef_i * SRS_i (kzg_poly_commitment.rs:278-293).  DegreeError when
        degree + 1 > SRS length; an all-zero polynomial commits to infinity."""
        degree = polynomial.degree()
        if degree + 1 > self.public_parameter_group_1.shape[0]:
            raise UzkgeError(N.UZK_ERR_DEGREE, "polynomial degree exceeds the SRS")
        return B.msm(self._srs, polynomial.get_coefs_ref()[: degree + 1])

    def apply_blind_factors(self, commitment: np.ndarray, blinds: np.ndarray, zeroing_degree: int) -> np.ndarray:
        """C += sum_i b_i * (SRS[i] - SRS[zeroing_degree + i]) (kzg_poly_commitment.rs:299-313)."""
        b = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(-1, 4)
        if b.shape[0] == 0:
            return commitment
        plus = B.msm(self._srs, b, offset=0)
        minus = B.msm(self._srs, fr_neg(b), offset=zeroing_degree)
        return B.g1_fold(np.stack([np.asarray(commitment, dtype=np.uint64).reshape(12), plus, minus]))

    def to_unchecked_bytes(self) -> bytes:
        """The G1 powers in the reference's blob format, no G2 part (as the reference's Lagrange files)."""
        return srs_g1_wire_to_bytes(self.public_parameter_group_1)

    def lagrange(self, n: int) -> "KZGCommitmentSchemeBN254":
        """A scheme over the Lagrange bases of size n derived on the device from the first n powers of this (monomial)
        scheme: usable wherever the reference loads `lagrange_pcs` from a file (ProverCommit), at any n = 2^k the G1
        transform supports."""
        srs = self._srs.to_lagrange(n)
        out = KZGCommitmentSchemeBN254.__new__(KZGCommitmentSchemeBN254)
        out._srs = srs
        out.public_parameter_group_1 = srs.download()
        return out

    def check(self, seed: Optional[bytes] = None, offset: int = 0, count: Optional[int] = None):
        """Validates the powers [offset, offset + count) on the device -- what from_unchecked_bytes skips (Validate::No,
        kzg_poly_commitment.rs:228-256).  Returns (report, left, right): the curve report of Srs.check_curve and the two points
        of Srs.fold_powers; the run is a power sequence of tau iff e(right, H) = e(left, [tau] H), the caller's pairing over the
        G2 part of the parameters.  ParameterError when a point is non-canonical or off the curve.  The seed of the fold is
        drawn here (os.urandom) unless given: it must not be known before the points are fixed."""
        report = self._srs.check_curve(offset, count)
        if report["first_bad"] is not None:
            raise UzkgeError(N.UZK_ERR_PARAMETER, "SRS point %d is not a curve point (%d non-canonical, %d off the curve)"
                             % (report["first_bad"], report["non_canonical"], report["off_curve"]))
        left, right = self._srs.fold_powers(os.urandom(32) if seed is None else seed, offset, count)
        return report, left, right

    def release(self) -> None:
        self._srs.release()


# ---------------------------------------------------------------------------------------------------
# The callers of the two primitives inside the prover: the Lagrange-basis commit path.
#   prover commit closure        uzkge/src/plonk/prover.rs:125-149
#   PolyComScheme::batch_prove   uzkge/src/poly_commit/pcs.rs:107-168
#   split_t_and_commit           uzkge/src/plonk/helpers.rs:1323-1408
# Fiat-Shamir (Keccak transcript) and the prover's RNG are out of scope: the
# challenge `alpha` and the random blinds are arguments here, where the Rust draws them.
# ---------------------------------------------------------------------------------------------------
def fr_add_rows(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a + b on wire-format rows (Montgomery form is linear)."""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros_like(a)
    for i in range(a.shape[0]):
        v = (_wire_int(a[i]) + _wire_int(b[i])) % FR_MODULUS
        out[i] = [(v >> (64 * k)) & _MASK64 for k in range(4)]
    return out


def max_power_of_2(degree: int) -> int:
    """The reference's loop `for i in (0..=degree).rev() { if (i & (i - 1)) == 0 {..break} }`
    (pcs.rs:139-145, helpers.rs:1367-1373): the largest power of two <= degree.  degree = 0 (a constant quotient) leaves
    the loop with 0 in a release build (0 & usize::MAX == 0): the fold then has no domain and the caller's `fft(.., 0)`
    fails -- PCSProveEvalError / FFTError in the reference, UzkgeError(FFT) here -- instead of an assertion."""
    if degree <= 0:
        return 0
    return 1 << (degree.bit_length() - 1)


def commit_folded_lagrange(pcs: KZGCommitmentSchemeBN254, lagrange_pcs: KZGCommitmentSchemeBN254, coefs: np.ndarray,
                           degree: int) -> np.ndarray:
    """The tail shared by batch_prove (pcs.rs:137-166, `degree` = q.degree()) and split_t_and_commit
    (helpers.rs:1366-1394, `degree` = coefs.len()): fold the coefficients from max_power_of_2 on back onto
    the low ones, fft(N), commit the evaluations over the Lagrange SRS, undo the fold with blind factors."""
    c = np.ascontiguousarray(coefs, dtype=np.uint64).reshape(-1, 4)
    npow = max_power_of_2(degree)
    if npow == 0:
        raise UzkgeError(N.UZK_ERR_FFT, "no evaluation domain for a degree-0 polynomial (max_power_of_2 = 0)")
    blinds = fr_neg(c[npow:])
    new_coefs = c[:npow].copy()
    if blinds.shape[0]:
        new_coefs[: blinds.shape[0]] = fr_add_rows(new_coefs[: blinds.shape[0]], c[npow:])    # coefs[i] - blinds[i]
    sub_q = FpPolynomial.from_coefs(new_coefs)
    q_eval = sub_q.fft(npow)
    if q_eval is None:
        raise UzkgeError(N.UZK_ERR_FFT, "no evaluation domain for the folded polynomial")
    cm = lagrange_pcs.commit(FpPolynomial.from_coefs(q_eval))
    return pcs.apply_blind_factors(cm, blinds, npow)


def batch_prove(pcs: KZGCommitmentSchemeBN254, lagrange_pcs: Optional[KZGCommitmentSchemeBN254],
                polys: Sequence[FpPolynomial], point: np.ndarray, alpha: np.ndarray):
    """PolyComScheme::batch_prove's default body (pcs.rs:107-168) with `alpha` given instead of drawn from the
    transcript.  Returns (commitment of q, evaluations p_k(point) [len(polys), 4]).  The evaluations, the linear
    combination and the division by X - point run on the device (uzk_open_quotient)."""
    assert len(polys) > 0
    n = max(p.coefs.shape[0] for p in polys)
    stack = np.zeros((len(polys), n, 4), dtype=np.uint64)
    for k, p in enumerate(polys):
        stack[k, : p.coefs.shape[0]] = p.coefs
    q_rows, evals = B.open_quotient(stack, point, alpha)
    q = FpPolynomial.from_coefs(q_rows)
    if lagrange_pcs is not None:
        return commit_folded_lagrange(pcs, lagrange_pcs, q.coefs, q.degree()), evals
    return pcs.commit(q), evals


def split_t_and_commit(pcs: KZGCommitmentSchemeBN254, lagrange_pcs: Optional[KZGCommitmentSchemeBN254], t: FpPolynomial,
                       n_wires_per_gate: int, n: int, rands: np.ndarray):
    """helpers.rs:1323-1408 with the prover's random blinds `rands` [n_wires_per_gate, 4] given: chunk i of t gets
    + rand_i * X^n and - rand_(i-1); every chunk is committed (Lagrange path: fold, fft, commit, blinds).
    Returns (commitments [n_wires_per_gate, 12], chunk polynomials)."""
    coefs_all = t.get_coefs_ref()
    coefs_len = coefs_all.shape[0]
    rands = np.ascontiguousarray(rands, dtype=np.uint64).reshape(n_wires_per_gate, 4)
    prev = np.zeros((1, 4), dtype=np.uint64)
    cms, polys = [], []
    for i in range(n_wires_per_gate):
        start = i * n
        end = coefs_len if i == n_wires_per_gate - 1 else (i + 1) * n
        coefs = coefs_all[start:min(coefs_len, end)].copy() if start < coefs_len else np.zeros((0, 4), np.uint64)
        if i != n_wires_per_gate - 1:
            padded = np.zeros((n + 1, 4), dtype=np.uint64)
            padded[: coefs.shape[0]] = coefs
            coefs = padded
            coefs[n] = fr_add_rows(coefs[n:n + 1], rands[i:i + 1])[0]
            coefs[0] = fr_add_rows(coefs[0:1], fr_neg(prev))[0]
        elif coefs.shape[0] == 0:
            coefs = fr_neg(prev)
        else:
            coefs[0] = fr_add_rows(coefs[0:1], fr_neg(prev))[0]
        prev = rands[i:i + 1]
        if lagrange_pcs is not None:
            cm = commit_folded_lagrange(pcs, lagrange_pcs, coefs, coefs.shape[0])
        else:
            cm = pcs.commit(FpPolynomial.from_coefs(coefs))
        cms.append(cm)
        polys.append(FpPolynomial.from_coefs(coefs))
    return np.stack(cms), polys


class ProverCommit:
    """The commit closure of prover_with_lagrange (prover.rs:125-149; twin in indexer.rs:284-299): the Lagrange
    SRS is used iff it has exactly n_constraints bases; then C = MSM(lagrange, evals) + blind factors, else the
    monomial commit of the coefficient polynomial."""

    def __init__(self, pcs: KZGCommitmentSchemeBN254, lagrange_pcs: Optional[KZGCommitmentSchemeBN254], n_constraints: int):
        self.pcs = pcs
        self.n_constraints = n_constraints
        self.lagrange_pcs = lagrange_pcs if (lagrange_pcs is not None and lagrange_pcs.max_degree() + 1 == n_constraints) else None

    def __call__(self, evals: np.ndarray, coef_polynomial: FpPolynomial, blinds: np.ndarray) -> np.ndarray:
        if self.lagrange_pcs is not None:
            cm = self.lagrange_pcs.commit(FpPolynomial.from_coefs(evals))
            return self.pcs.apply_blind_factors(cm, blinds, self.n_constraints)
        return self.pcs.commit(coef_polynomial)


def preprocess_tables(commit: ProverCommit, evals: np.ndarray, m: int, k1: np.ndarray, keep_on_device: bool = False):
    """The per-table loop of the preprocessing -- indexer_with_lagrange (uzkge/src/plonk/indexer.rs:316-470: the
    permutation, selector, boolean, Anemoi, ecc and shuffle tables) and refresh_prover_params_public_key
    (shuffle/src/gen_params/params.rs:88-121) -- for a stack `evals` [k, n, 4] of evaluation tables:
        coefs_i      = FpPolynomial::ifft_with_domain(domain_n, evals_i)
        coset_evals_i = coefs_i.coset_fft_with_domain(domain_m, k[1])
        cm_i         = commit(evals_i, coefs_i)        (the closure without blinds, indexer.rs:284-299)
    All k tables go through ONE batched inverse transform, ONE batched coset transform on the m-domain and ONE batched
    MSM; the tables cross PCIe once.  Returns (coefs [k, n, 4], coset_evals [k, m, 4], cms [k, 12]); with
    `keep_on_device` the first two are int64 CUDA tensors (the quotient kernel's resident inputs, uzk_t_quotient_device)
    instead of host arrays."""
    import torch
    ev_h = np.ascontiguousarray(evals, dtype=np.uint64)
    assert ev_h.ndim == 3 and ev_h.shape[2] == 4
    k, n = ev_h.shape[0], ev_h.shape[1]
    if n != commit.n_constraints or m % n != 0:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "tables must have n_constraints rows and the quotient domain must be a multiple of n")
    if not (B.domain_supported(n) and B.domain_supported(m)):
        raise UzkgeError(N.UZK_ERR_FFT, "no evaluation domain of that size")
    ev = torch.from_numpy(ev_h.view(np.int64)).cuda()
    coefs = torch.empty_like(ev)
    coset = torch.zeros((k, m, 4), dtype=torch.int64, device=ev.device)
    torch.cuda.synchronize()                       # the library runs on its own stream
    B.ntt_batch_device(ev.data_ptr(), coefs.data_ptr(), n, k, inverse=True, sync=True)
    coset[:, :n] = coefs
    torch.cuda.synchronize()
    B.ntt_batch_device(coset.data_ptr(), coset.data_ptr(), m, k, coset_shift=k1)
    if commit.lagrange_pcs is not None:
        cms = B.msm_batch_device(commit.lagrange_pcs._srs, ev.data_ptr(), n, k)
    else:
        if n > commit.pcs.public_parameter_group_1.shape[0]:
            raise UzkgeError(N.UZK_ERR_DEGREE, "polynomial degree exceeds the SRS")
        cms = B.msm_batch_device(commit.pcs._srs, coefs.data_ptr(), n, k)
    B.sync()
    if keep_on_device:
        return coefs, coset, cms
    return (coefs.cpu().numpy().view(np.uint64), coset.cpu().numpy().view(np.uint64), cms)


def fq_from_int(x: int) -> np.ndarray:
    return _to_wire(x % FQ_MODULUS, FQ_MODULUS)


def g1_wire(point) -> np.ndarray:
    """(x, y) as integers, or None for the point at infinity -> the 8-word wire row."""
    if point is None:
        return np.zeros(8, dtype=np.uint64)
    return np.concatenate([fq_from_int(int(point[0])), fq_from_int(int(point[1]))])


class PlonkVerifierKey:
    """PlonkVerifierParams (uzkge/src/plonk/indexer.rs) resident on the device, for batches of proofs: `fold` runs everything of the
    verifier (verifier.rs:17-164) in front of its two pairings for m proofs at once and returns the two G1 points of the ONE check
        e(L, [tau] G2) = e(R, G2)
    that stands for all of them; `verify_batch` goes on to that check on the device (uzk_pairing_product) and returns the verdict.

    vk: the key as integers -- cm_q (9 points), cm_s (5), cm_qb, cm_prk (4), k (5), anemoi_g, anemoi_g_inv, edwards_a, root, cs_size,
    pi_root_powers, pi_lagrange and, with the shuffle feature, cm_q_ecc, cm_shuffle_public_key (12), cm_shuffle_generator (12);
    points are (x, y) or None.  g1_0: the SRS's first point (default: the generator, as in the reference's parameters).
    prefix: the transcript bytes in front of transcript_init_plonk."""

    def __init__(self, vk: dict, prefix: bytes = b"", g1_0=(1, 2), shuffle: bool = True):
        pts = lambda rows: np.stack([g1_wire(p) for p in rows])
        frs = lambda vals: np.stack([fr_from_int(int(v)) for v in vals]) if len(vals) else np.zeros((0, 4), dtype=np.uint64)
        extra = dict(cm_q_ecc=g1_wire(vk["cm_q_ecc"]), cm_shuffle_public_key=pts(vk["cm_shuffle_public_key"]),
                     cm_shuffle_generator=pts(vk["cm_shuffle_generator"])) if shuffle else {}
        self.key = B.VerifierKey(int(vk["cs_size"]), pts(vk["cm_q"]), pts(vk["cm_s"]), g1_wire(vk["cm_qb"]), pts(vk["cm_prk"]), g1_wire(g1_0),
                                 frs(vk["k"]), fr_from_int(vk["anemoi_g"]), fr_from_int(vk["anemoi_g_inv"]), fr_from_int(vk["edwards_a"]),
                                 fr_from_int(vk["root"]), frs(vk["pi_root_powers"]), frs(vk["pi_lagrange"]), prefix=prefix, shuffle=shuffle, **extra)
        self.n_pi, self.proof_bytes = self.key.n_pi, self.key.proof_bytes

    def set_public_key(self, commitments) -> None:
        """cm_shuffle_public_key of the next game (12 points)."""
        self.key.set_public_key(np.stack([g1_wire(p) for p in commitments]))

    def fold(self, proofs: Sequence[bytes], pis: Sequence[Sequence[int]], weights: Optional[Sequence[int]] = None):
        """proofs: m blobs of PlonkProof::to_bytes_be; pis: m lists of n_pi integers; weights: m integers the CALLER draws after it has
        the proofs (None only for one proof: weight 1).  Returns (L, R, status): two Jacobian wire points [12] and one byte per proof
        (0 folded, 1 a non-canonical word, 2 a point off the curve -- such a proof is left out of both sums)."""
        m = len(proofs)
        if m != len(pis) or (weights is not None and len(weights) != m) or any(len(p) != self.proof_bytes for p in proofs):
            raise UzkgeError(N.UZK_ERR_PARAMETER, "PlonkVerifierKey.fold: one proof blob, one list of public inputs and one weight per proof")
        pi = np.zeros((m, self.n_pi, 4), dtype=np.uint64)
        for i, row in enumerate(pis):
            if len(row) != self.n_pi:
                raise UzkgeError(N.UZK_ERR_PARAMETER, "PlonkVerifierKey.fold: %d public inputs per proof" % self.n_pi)
            for j, v in enumerate(row):
                pi[i, j] = fr_from_int(int(v))
        w = None if weights is None else np.stack([fr_from_int(int(v)) for v in weights]) if m else np.zeros((0, 4), dtype=np.uint64)
        return self.key.fold(b"".join(proofs), pi, w)

    def verify_batch(self, proofs: Sequence[bytes], pis: Sequence[Sequence[int]], weights: Optional[Sequence[int]], g2_0, g2_1):
        """`fold`, then the check it stands for on the device: e(L, [tau] H) e(-R, H) = 1 with H = g2_0 and [tau] H = g2_1, the two G2
        elements of the SRS as integers ((x0, x1), (y0, y1)).  Returns (accepted, status): accepted iff every status is 0 and the
        product is one."""
        left, right, status = self.fold(proofs, pis, weights)
        l_aff, r_aff = B.g1_to_affine(left), B.g1_to_affine(right)
        y = _wire_int(r_aff[4:])
        if y:
            y = FQ_MODULUS - y                                       # Montgomery form is linear: -R
            r_aff = np.concatenate([r_aff[:4], np.array([(y >> (64 * k)) & _MASK64 for k in range(4)], dtype=np.uint64)])
        _, one = B.pairing_product(np.stack([l_aff, r_aff]), np.stack([g2_wire(g2_1), g2_wire(g2_0)]), want_gt=False)
        return bool(one and not np.any(status)), status

    def release(self) -> None:
        self.key.release()


# ---- Groth16 verifying keys ----------------------------------------------------------------------------------------------------
_P = FQ_MODULUS
_TWIST_B = (27 * pow(82, _P - 2, _P) % _P, (-3 * pow(82, _P - 2, _P)) % _P)       # 3 / (9 + u)


def _fq_sqrt(a: int):
    r = pow(a, (_P + 1) // 4, _P)                                                   # p = 3 mod 4
    return r if r * r % _P == a % _P else None


def _fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % _P, (a[0] * b[1] + a[1] * b[0]) % _P)


def _fq2_sqrt(a):
    """by the norm: with n = sqrt(a0^2 + a1^2), x0^2 = (a0 +- n) / 2 and x1 = a1 / (2 x0)"""
    if a[1] == 0:
        r = _fq_sqrt(a[0])
        if r is not None:
            return (r, 0)
        r = _fq_sqrt((-a[0]) % _P)
        return None if r is None else (0, r)
    n = _fq_sqrt((a[0] * a[0] + a[1] * a[1]) % _P)
    if n is None:
        return None
    for s in (n, _P - n):
        x0 = _fq_sqrt((a[0] + s) * ((_P + 1) // 2) % _P)
        if x0:
            x = (x0, a[1] * pow(2 * x0, _P - 2, _P) % _P)
            if _fq2_mul(x, x) == (a[0] % _P, a[1] % _P):
                return x
    return None


def _g1_decompress(b: bytes):
    """ark-serialize, compressed: x little-endian, bit 7 of the last byte = the larger y, bit 6 = infinity"""
    flags = b[31]
    if flags & 0x40:
        return None
    x = int.from_bytes(b[:31] + bytes([flags & 0x3f]), "little")
    y = _fq_sqrt((x * x * x + 3) % _P)
    if x >= _P or y is None:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "Groth16VerifierKey: a compressed G1 point is not on the curve")
    return (x, _P - y) if (y > _P - y) != bool(flags & 0x80) else (x, y)


def _g2_decompress(b: bytes):
    flags = b[63]
    if flags & 0x40:
        return None
    x = (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:63] + bytes([flags & 0x3f]), "little"))
    x3 = _fq2_mul(_fq2_mul(x, x), x)
    y = _fq2_sqrt(((x3[0] + _TWIST_B[0]) % _P, (x3[1] + _TWIST_B[1]) % _P)) if max(x) < _P else None
    if y is None:
        raise UzkgeError(N.UZK_ERR_PARAMETER, "Groth16VerifierKey: a compressed G2 point is not on the twist")
    ny = ((-y[0]) % _P, (-y[1]) % _P)
    return (x, ny) if ((y[1], y[0]) > (ny[1], ny[0])) != bool(flags & 0x80) else (x, y)       # ark-ff orders Fq2 by c1, then c0


def g2_wire(point) -> np.ndarray:
    """x.c0, x.c1, y.c0, y.c1 as Montgomery words [16]; None = infinity = zeros"""
    if point is None:
        return np.zeros(16, dtype=np.uint64)
    (x0, x1), (y0, y1) = point
    return np.concatenate([fq_from_int(int(v)) for v in (x0, x1, y0, y1)])


def g16_proof_blob(a, b, c) -> bytes:
    """The 256-byte blob of a proof: a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0, c.x, c.y as 32-byte big-endian words (the EVM order of
    the reference's contract); None = infinity = zeros."""
    a, c = a or (0, 0), c or (0, 0)
    (bx0, bx1), (by0, by1) = b or ((0, 0), (0, 0))
    return b"".join(int(v).to_bytes(32, "big") for v in (a[0], a[1], bx1, bx0, by1, by0, c[0], c[1]))


class Groth16VerifierKey:
    """A Groth16 verifying key resident on the device, for batches of proofs: `fold` runs everything in front of the pairings for m
    proofs at once and returns the G1 (and G2) arguments of the ONE product of m + 3 Miller loops
        prod_i e(rho_i A_i, B_i) . e(-(sum rho) alpha, beta) . e(-sum rho_i X_i, gamma) . e(-sum rho_i C_i, delta) = 1
    that stands for all of them; `verify_batch` goes on to that product on the device and returns the verdict.

    Points are integers: G1 (x, y), G2 ((x0, x1), (y0, y1)), None = infinity."""

    def __init__(self, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1):
        self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2, self.gamma_abc_g1 = alpha_g1, beta_g2, gamma_g2, delta_g2, list(gamma_abc_g1)
        ic = np.stack([g1_wire(p) for p in self.gamma_abc_g1]) if self.gamma_abc_g1 else np.zeros((0, 8), dtype=np.uint64)
        self.key = B.Groth16VerifierKey(g1_wire(alpha_g1), g2_wire(beta_g2), g2_wire(gamma_g2), g2_wire(delta_g2), ic)
        self.n_inputs = self.key.n_inputs

    @staticmethod
    def parse_key_bytes(head: bytes):
        """ark-serialize (compressed) VerifyingKey<Bn254> -- what a ProvingKey file starts with: alpha_g1 | beta_g2 | gamma_g2 |
        delta_g2 | u64 LE length | gamma_abc_g1.  Returns (alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1); bytes behind the key
        are ignored."""
        if len(head) < 232:
            raise UzkgeError(N.UZK_ERR_PARAMETER, "Groth16VerifierKey: %d bytes cannot hold a verifying key" % len(head))
        alpha = _g1_decompress(head[0:32])
        beta, gamma, delta = (_g2_decompress(head[32 + 64 * k:96 + 64 * k]) for k in range(3))
        l = struct.unpack_from("<Q", head, 224)[0]
        if l < 1 or l > N.G16_VERIFY_MAX_INPUTS or len(head) < 232 + 32 * l:
            raise UzkgeError(N.UZK_ERR_PARAMETER, "Groth16VerifierKey: gamma_abc_g1 of %d points" % l)
        return alpha, beta, gamma, delta, [_g1_decompress(head[232 + 32 * j:264 + 32 * j]) for j in range(l)]

    @classmethod
    def from_key_bytes(cls, head: bytes) -> "Groth16VerifierKey":
        return cls(*cls.parse_key_bytes(head))

    @classmethod
    def from_compressed(cls, data: bytes, validate: bool = False) -> "Groth16VerifierKey":
        """`from_key_bytes` with the points decoded on the device (uzk_g16_vk_create_compressed): data is a compressed verifying key,
        or a proving key whose first 232 + 32 l bytes are one.  validate: also the subgroup check of beta, gamma and delta.  The
        integer attributes of the other constructors (alpha_g1 ...) are not filled in."""
        import ctypes

        from . import codec
        raw = np.frombuffer(bytes(data), dtype=np.uint8)
        h = ctypes.c_uint64(0)
        codec.check(codec.lib.uzk_g16_vk_create_compressed(raw.ctypes.data_as(ctypes.c_void_p) if raw.size else None, raw.size, int(bool(validate)), ctypes.byref(h)))
        self = cls.__new__(cls)
        key = B.Groth16VerifierKey.__new__(B.Groth16VerifierKey)
        key.handle = h.value
        g2, _ = codec.g2_decompress(bytes(data[32:224]))             # accepted above: every status is 0
        key.beta_g2, key.gamma_g2, key.delta_g2 = (g2[k].copy() for k in range(3))
        key.n_inputs, key.device = key.info()
        self.key, self.n_inputs = key, key.n_inputs
        return self

    def _inputs(self, what, proofs, publics, weights):
        m = len(proofs)
        if m != len(publics) or (weights is not None and len(weights) != m) or any(len(p) != N.G16_PROOF_BYTES for p in proofs):
            raise UzkgeError(N.UZK_ERR_PARAMETER, "Groth16VerifierKey.%s: one 256-byte blob, one list of public inputs and one weight per proof" % what)
        pub = np.zeros((m, self.n_inputs - 1, 4), dtype=np.uint64)
        for i, row in enumerate(publics):
            if len(row) != self.n_inputs - 1:
                raise UzkgeError(N.UZK_ERR_PARAMETER, "Groth16VerifierKey.%s: %d public inputs per proof" % (what, self.n_inputs - 1))
            for j, v in enumerate(row):
                pub[i, j] = fr_from_int(int(v))
        w = None if weights is None else np.stack([fr_from_int(int(v)) for v in weights]) if m else np.zeros((0, 4), dtype=np.uint64)
        return pub, w

    def fold(self, proofs: Sequence[bytes], publics: Sequence[Sequence[int]], weights: Optional[Sequence[int]] = None):
        """proofs: m blobs of 256 bytes (g16_proof_blob); publics: m lists of l - 1 integers (the leading one is implied); weights: m
        integers the CALLER draws after it has the proofs (None only for one proof: weight 1).  Returns (a [m, 8], b [m, 16], alpha
        [12], x [12], c [12], status [m]): rho_i A_i as affine wire points, B_i, three Jacobian wire points and one byte per proof (0
        folded, 1 a word >= p, 2 a point off its curve, 3 B outside the subgroup -- such a proof is left out of every sum)."""
        pub, w = self._inputs("fold", proofs, publics, weights)
        return self.key.fold(b"".join(proofs), pub, w)

    def verify_batch(self, proofs: Sequence[bytes], publics: Sequence[Sequence[int]], weights: Optional[Sequence[int]] = None):
        """The arguments of `fold`; the fold and the product of its m + 3 pairings on the device (uzk_g16_verify_batch).  Returns
        (accepted, status [m]): accepted iff every status is 0 and the product is one; no proofs are accepted."""
        pub, w = self._inputs("verify_batch", proofs, publics, weights)
        return self.key.verify_batch(b"".join(proofs), pub, w)

    def info(self):
        return self.key.info()

    def release(self) -> None:
        self.key.release()


def hide_polynomial(polynomial: FpPolynomial, blinds: np.ndarray, zeroing_degree: int) -> FpPolynomial:
    """helpers.rs:139-158 with the random blinds given: adds (b_0 + b_1 X + ...) * (X^zeroing_degree - 1)."""
    b = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(-1, 4)
    size = max(polynomial.coefs.shape[0], zeroing_degree + b.shape[0])
    c = np.zeros((size, 4), dtype=np.uint64)
    c[: polynomial.coefs.shape[0]] = polynomial.coefs
    for i in range(b.shape[0]):
        c[i] = fr_add_rows(c[i:i + 1], b[i:i + 1])[0]
        c[zeroing_degree + i] = fr_add_rows(c[zeroing_degree + i:zeroing_degree + i + 1], fr_neg(b[i:i + 1]))[0]
    return FpPolynomial.from_coefs(c)


def load_srs_params(srs_blob: bytes, size: int) -> KZGCommitmentSchemeBN254:
    """uzkge/src/gen_params/mod.rs:151-183: the monomial SRS of a size-`size` circuit from the embedded blob --
    powers 0..2050, the identity up to `size`, then the three padding powers size, size+1, size+2."""
    return KZGCommitmentSchemeBN254(srs_params_wire(srs_blob, size))
