//! Bindings to `libuzkge_gpu.so` (C ABI: `include/uzkge_gpu.h`), the MI355X backend for the two hot paths of
//! `uzkge::plonk::prover`:
//!
//! * `G1Projective::msm(&points_raw, &coefs)`  -- `uzkge/src/poly_commit/kzg_poly_commitment.rs:287-290`
//! * `domain.fft(&self.coefs)` / `domain.ifft(&values)` -- `uzkge/src/poly_commit/field_polynomial.rs:585,595`
//!
//! `ffi` is generated from the header (`tools/gen_rust_bindings.py`); this file adds the error mapping and a few
//! safe conveniences.  The crate knows nothing about arkworks: field elements travel as `[u64; 4]` Montgomery limbs
//! (`Fp<MontBackend<_, 4>, 4>`'s inner `BigInt<4>`), the arkworks-side repacking lives in uzkge (`src/gpu.rs` of the
//! patch next to this crate).
pub mod ffi;
pub use ffi::*;

use std::ffi::CStr;
use std::os::raw::c_int;

/// The non-OK return codes, named after the `UzkgeError` variants they map to (`uzkge/src/errors.rs:5-44`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Error {
    Parameter,
    Degree,
    Fft,
    Commitment,
    /// no gfx950 device, HIP failure, out of device memory: there is no CPU fallback
    Device,
    Unknown(c_int),
}

pub fn check(rc: c_int) -> Result<(), Error> {
    match rc {
        UZK_OK => Ok(()),
        UZK_ERR_PARAMETER => Err(Error::Parameter),
        UZK_ERR_DEGREE => Err(Error::Degree),
        UZK_ERR_FFT => Err(Error::Fft),
        UZK_ERR_COMMITMENT => Err(Error::Commitment),
        UZK_ERR_DEVICE => Err(Error::Device),
        other => Err(Error::Unknown(other)),
    }
}

/// Description of the last non-OK return on this thread.
pub fn last_error() -> String {
    unsafe {
        let p = uzk_last_error();
        if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
    }
}

/// A device-resident SRS (the static bases of KZG commit); released on drop.
pub struct Srs {
    handle: u64,
    len: usize,
}

impl Srs {
    /// Copies `points` to HBM once; replaces the per-commit `normalize_batch` (kzg_poly_commitment.rs:287-288).
    pub fn register(points: &[uzk_g1_affine]) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_srs_register(points.as_ptr(), points.len(), &mut handle) })?;
        Ok(Srs { handle, len: points.len() })
    }
    /// Optional for a static SRS: window table in HBM (`uzk_srs_precompute`); identical results, shorter calls.
    pub fn precompute(&self, window_bits: c_int) -> Result<(), Error> {
        check(unsafe { uzk_srs_precompute(self.handle, window_bits) })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    pub fn handle(&self) -> u64 { self.handle }

    /// sum_i scalars[i] * SRS[offset + i]  (`G1Projective::msm`, kzg_poly_commitment.rs:290).
    pub fn msm(&self, offset: usize, scalars_mont: &[[u64; 4]]) -> Result<uzk_g1_jac, Error> {
        let mut out = uzk_g1_jac::default();
        check(unsafe { uzk_msm_g1(self.handle, offset, scalars_mont.as_ptr() as *const u64, scalars_mont.len(), &mut out) })?;
        Ok(out)
    }
    /// `batch` vectors of `n` scalars each against the same bases (the prover's independent commits in one call).
    pub fn msm_batch(&self, offset: usize, scalars_mont: &[[u64; 4]], n: usize) -> Result<Vec<uzk_g1_jac>, Error> {
        if n == 0 || scalars_mont.len() % n != 0 {
            return Err(Error::Parameter);
        }
        let batch = scalars_mont.len() / n;
        let mut out = vec![uzk_g1_jac::default(); batch];
        check(unsafe { uzk_msm_g1_batch(self.handle, offset, scalars_mont.as_ptr() as *const u64, n, batch as u32, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// The Lagrange bases of size `n` (a power of two up to 2^UZK_NTT_G1_MAX_LOG2) from the first `n` points of this monomial
    /// SRS: the inverse G1 transform on the device (`uzk_srs_to_lagrange`) -- what the reference reads from one of its three
    /// `lagrange-srs-*.bin` files (gen_params/mod.rs:186-199), for any size.  The new SRS owns its memory.
    pub fn to_lagrange(&self, n: usize) -> Result<Srs, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_srs_to_lagrange(self.handle, n as u64, &mut handle) })?;
        Ok(Srs { handle, len: n })
    }
    /// `n` points from `offset` on, read back from the device (to keep or save a derived basis).
    pub fn download(&self, offset: usize, n: usize) -> Result<Vec<uzk_g1_affine>, Error> {
        let mut out = vec![uzk_g1_affine::default(); n];
        check(unsafe { uzk_srs_download(self.handle, offset, n, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// Are the points `[offset, offset + count)` curve points?  (`uzk_srs_check_curve`; the reference loads its parameters with
    /// `Validate::No`, kzg_poly_commitment.rs:228-256.)  BN254 G1 has cofactor 1: on the curve is in the group.
    pub fn check_curve(&self, offset: usize, count: usize) -> Result<uzk_srs_curve_report, Error> {
        let mut out = uzk_srs_curve_report::default();
        check(unsafe { uzk_srs_check_curve(self.handle, offset, count, &mut out) })?;
        Ok(out)
    }
    /// `(left, right)` of the run `[offset, offset + count)`, `count >= 2`, under the 128-bit weights of `seed` (drawn after the
    /// points are fixed): the run is a power sequence of tau iff `e(right, H) == e(left, [tau] H)` -- the caller's pairing, over
    /// G2 points the caller has checked (`uzk_srs_fold_powers`).
    pub fn fold_powers(&self, offset: usize, count: usize, seed: &[u8; 32]) -> Result<(uzk_g1_jac, uzk_g1_jac), Error> {
        let (mut left, mut right) = (uzk_g1_jac::default(), uzk_g1_jac::default());
        check(unsafe { uzk_srs_fold_powers(self.handle, offset, count, seed.as_ptr(), &mut left, &mut right) })?;
        Ok((left, right))
    }
}

impl Srs {
    /// The indexer's per-table loop without a circuit (`uzk_preprocess_tables`): `evals.len() / n` evaluation vectors of n elements
    /// -> (coefficient forms: n each, zero padded; their trimmed lengths; coset evaluations over the 6n domain shifted by `k1`:
    /// 6n each; the commitments over this Lagrange SRS of n bases, empty unless `want_commit`).
    #[allow(clippy::type_complexity)]
    pub fn preprocess_tables(&self, evals: &[[u64; 4]], n: usize, k1: &[u64; 4], want_commit: bool) -> Result<(Vec<[u64; 4]>, Vec<u64>, Vec<[u64; 4]>, Vec<uzk_g1_jac>), Error> {
        if n == 0 || evals.is_empty() || evals.len() % n != 0 || n > u32::MAX as usize {
            return Err(Error::Parameter);
        }
        let count = evals.len() / n;
        let mut polys = vec![[0u64; 4]; evals.len()];
        let mut lens = vec![0u64; count];
        let mut coset = vec![[0u64; 4]; 6 * evals.len()];
        let mut cms = vec![uzk_g1_jac::default(); if want_commit { count } else { 0 }];
        let cms_ptr = if want_commit { cms.as_mut_ptr() } else { std::ptr::null_mut() };
        check(unsafe {
            uzk_preprocess_tables(self.handle, n as u32, count as u32, evals.as_ptr() as *const u64, k1.as_ptr(), polys.as_mut_ptr() as *mut u64, lens.as_mut_ptr(),
                                  coset.as_mut_ptr() as *mut u64, cms_ptr)
        })?;
        Ok((polys, lens, coset, cms))
    }
}

impl Drop for Srs {
    fn drop(&mut self) {
        unsafe { uzk_srs_release(self.handle) };
    }
}

/// Device-resident G2 bases (the `b_g2_query` of a Groth16 proving key); released on drop.
pub struct G2Bases {
    handle: u64,
    len: usize,
}

impl G2Bases {
    /// Copies `points` to HBM once (`uzk_g2_register`).
    pub fn register(points: &[uzk_g2_affine]) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_g2_register(points.as_ptr(), points.len(), &mut handle) })?;
        Ok(G2Bases { handle, len: points.len() })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    pub fn handle(&self) -> u64 { self.handle }

    /// sum_i scalars[i] * bases[offset + i]  (the G2 term of a Groth16 proof's B).
    pub fn msm_g2(&self, offset: usize, scalars_mont: &[[u64; 4]]) -> Result<uzk_g2_jac, Error> {
        let mut out = uzk_g2_jac::default();
        check(unsafe { uzk_msm_g2(self.handle, offset, scalars_mont.as_ptr() as *const u64, scalars_mont.len(), &mut out) })?;
        Ok(out)
    }
    /// `batch` vectors of `n` scalars each against the same bases: the reveal proofs of one deck in one launch sequence.
    pub fn msm_g2_batch(&self, offset: usize, scalars_mont: &[[u64; 4]], n: usize) -> Result<Vec<uzk_g2_jac>, Error> {
        if n == 0 || scalars_mont.len() % n != 0 {
            return Err(Error::Parameter);
        }
        let batch = scalars_mont.len() / n;
        let mut out = vec![uzk_g2_jac::default(); batch];
        check(unsafe { uzk_msm_g2_batch(self.handle, offset, scalars_mont.as_ptr() as *const u64, n, batch as u32, out.as_mut_ptr()) })?;
        Ok(out)
    }
}

impl Drop for G2Bases {
    fn drop(&mut self) {
        unsafe { uzk_g2_release(self.handle) };
    }
}

/// An SRS cut into contiguous point chunks over the GPUs of a node, driven from this one process (`uzk_srs_register_sharded`):
/// chunk i = [i n / N, (i + 1) n / N) lives on `devices[i]`; `msm` runs the chunks side by side and folds the 96-byte partial
/// sums on the host -- north_star's "MSM shards by point-chunk across the 8 GPUs of one node" behind one call.
pub struct ShardedSrs {
    handle: u64,
    len: usize,
}
impl ShardedSrs {
    /// `window_bits`: -1 no window table, 0 automatic, 4..24.
    pub fn register(points: &[uzk_g1_affine], devices: &[c_int], window_bits: c_int) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_srs_register_sharded(points.as_ptr(), points.len(), devices.as_ptr(), devices.len() as u32, window_bits, &mut handle) })?;
        Ok(ShardedSrs { handle, len: points.len() })
    }
    pub fn len(&self) -> usize { self.len }
    pub fn is_empty(&self) -> bool { self.len == 0 }
    /// sum_i scalars[i] * SRS[i]
    pub fn msm(&self, scalars_mont: &[[u64; 4]]) -> Result<uzk_g1_jac, Error> {
        let mut out = uzk_g1_jac::default();
        check(unsafe { uzk_msm_g1_sharded(self.handle, scalars_mont.as_ptr() as *const u64, scalars_mont.len(), std::ptr::null_mut(), &mut out) })?;
        Ok(out)
    }
}
impl Drop for ShardedSrs {
    fn drop(&mut self) {
        unsafe { uzk_srs_release_sharded(self.handle) };
    }
}

/// In-place transform over the size-`data.len()` domain, natural order (`EvaluationDomain::{fft, ifft}`);
/// `coset_shift`: forward = pre-scale by shift^j, inverse = post-scale by shift^j (pass k^-1).
pub fn ntt(data: &mut [[u64; 4]], inverse: bool, coset_shift: Option<&[u64; 4]>) -> Result<(), Error> {
    let shift = coset_shift.map_or(std::ptr::null(), |s| s.as_ptr());
    check(unsafe { uzk_ntt_fr(data.as_mut_ptr() as *mut u64, data.len() as u64, inverse as c_int, shift) })
}

/// group_gen of the size-n domain as this library defines it (5^((r-1)/n), Montgomery limbs).
pub fn domain_group_gen(n: u64) -> Result<[u64; 4], Error> {
    let mut out = [0u64; 4];
    check(unsafe { uzk_domain_group_gen(n, out.as_mut_ptr()) })?;
    Ok(out)
}

// ---------------------------------------------------------------------------------------------------------------------
// The device-resident prover (uzkge/src/plonk/gpu_prover.rs): circuits, provers and the five rounds.  Nothing here links the
// HIP runtime, and nothing here decides anything: lengths, folds, table snapshots and error conditions live in the library.
// ---------------------------------------------------------------------------------------------------------------------
use std::os::raw::c_void;

/// One field element on the wire: 4 little-endian u64 limbs, Montgomery form.
pub type Limbs = [u64; 4];

/// A context (one stream, one set of workspaces, one lock) for a prover thread; see `uzk_ctx_create`.
pub struct Context(u64);
impl Context {
    pub fn new() -> Result<Self, Error> {
        let mut h = 0u64;
        check(unsafe { uzk_ctx_create(&mut h) })?;
        Ok(Context(h))
    }
    /// A context on a named device (`uzk_ctx_create_on`): circuits, provers and SRS handles made while it is current live there,
    /// so one process can run a pool of prover threads over all the GPUs of a node.
    pub fn on_device(device: c_int) -> Result<Self, Error> {
        let mut h = 0u64;
        check(unsafe { uzk_ctx_create_on(device, &mut h) })?;
        Ok(Context(h))
    }
    pub fn device(&self) -> Result<c_int, Error> {
        let mut d: c_int = 0;
        check(unsafe { uzk_ctx_device(self.0, &mut d) })?;
        Ok(d)
    }
    /// Makes this context the calling thread's current one.
    pub fn make_current(&self) -> Result<(), Error> {
        check(unsafe { uzk_ctx_set_current(self.0) })
    }
}
impl Drop for Context {
    fn drop(&mut self) {
        unsafe {
            uzk_ctx_set_current(0);
            uzk_ctx_destroy(self.0);
        }
    }
}

/// A circuit resident in HBM (`uzk_circuit_create`): commit bases, permutation, the 46 (21) polynomials and their coset tables.
/// Process-wide: provers of every thread may use it at the same time.  Released on drop.
pub struct Circuit {
    handle: u64,
}
impl Circuit {
    /// `desc` and everything it points to are read before this returns.
    pub fn create(desc: &uzk_circuit_desc) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_circuit_create(desc, &mut handle) })?;
        Ok(Circuit { handle })
    }
    /// Replaces the polynomials of slots first_slot.. (coefficient forms, trimmed as `FpPolynomial::from_coefs` leaves them) and
    /// re-derives their coset tables; copy on write: a proof in flight keeps the tables it started with.
    pub fn update_tables(&self, first_slot: u32, polys: &[Vec<Limbs>]) -> Result<(), Error> {
        let ptrs: Vec<*const u64> = polys.iter().map(|p| p.as_ptr() as *const u64).collect();
        let lens: Vec<u64> = polys.iter().map(|p| p.len() as u64).collect();
        check(unsafe { uzk_circuit_update_tables(self.handle, first_slot, polys.len() as u32, ptrs.as_ptr(), lens.as_ptr()) })
    }
    /// The refresh / indexer loop as one device call (`uzk_circuit_refresh_tables`): `evals.len() / n` evaluation vectors of n
    /// elements -> (coefficient forms: n each, zero padded; their trimmed lengths; coset evaluations: 6n each, empty unless
    /// `want_coset`; the Lagrange commitments of the evaluations), installed in the slots.
    #[allow(clippy::type_complexity)]
    pub fn refresh_tables(&self, first_slot: u32, evals: &[Limbs], n: usize, want_coset: bool) -> Result<(Vec<Limbs>, Vec<u64>, Vec<Limbs>, Vec<uzk_g1_jac>), Error> {
        if n == 0 || evals.len() % n != 0 {
            return Err(Error::Parameter);
        }
        let count = evals.len() / n;
        let mut polys = vec![[0u64; 4]; evals.len()];
        let mut lens = vec![0u64; count];
        let mut coset = vec![[0u64; 4]; if want_coset { 6 * evals.len() } else { 0 }];
        let mut cms = vec![uzk_g1_jac::default(); count];
        let coset_ptr = if want_coset { coset.as_mut_ptr() as *mut u64 } else { std::ptr::null_mut() };
        check(unsafe {
            uzk_circuit_refresh_tables(self.handle, first_slot, count as u32, evals.as_ptr() as *const u64, polys.as_mut_ptr() as *mut u64, lens.as_mut_ptr(), coset_ptr,
                                       cms.as_mut_ptr())
        })?;
        Ok((polys, lens, coset, cms))
    }
    /// (n, evaluations round 4 writes per proof, r_poly scalars round 5 reads per proof, device) -- `uzk_circuit_info`.
    pub fn info(&self) -> Result<(u32, u32, u32, c_int), Error> {
        let (mut n, mut ev, mut rs, mut dev) = (0u32, 0u32, 0u32, 0 as c_int);
        check(unsafe { uzk_circuit_info(self.handle, &mut n, &mut ev, &mut rs, &mut dev) })?;
        Ok((n, ev, rs, dev))
    }
    pub fn handle(&self) -> u64 { self.handle }
}
impl Drop for Circuit {
    fn drop(&mut self) {
        unsafe { uzk_circuit_release(self.handle) };
    }
}

/// A verifier key resident on the device (`uzk_vk_create`), for batches of proofs: `fold` runs everything of the reference's verifier
/// in front of its two pairings for m proofs at once and returns the two G1 points of the ONE check e(L, [tau] G2) = e(R, G2) that
/// stands for all of them.  The pairing is the caller's (the library computes no pairing).  Process-wide; released on drop.
pub struct VerifierKey {
    handle: u64,
    n_pi: usize,
    proof_bytes: usize,
}
impl VerifierKey {
    /// `desc` and everything it points to are read before this returns.
    pub fn create(desc: &uzk_vk_desc) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_vk_create(desc, &mut handle) })?;
        let (mut cs, mut n_pi, mut bytes, mut dev) = (0u32, 0u32, 0u32, 0 as c_int);
        if let Err(e) = check(unsafe { uzk_vk_info(handle, &mut cs, &mut n_pi, &mut bytes, &mut dev) }) {
            unsafe { uzk_vk_release(handle) };
            return Err(e);
        }
        Ok(VerifierKey { handle, n_pi: n_pi as usize, proof_bytes: bytes as usize })
    }
    /// The public-key commitments of the next game (`uzk_vk_set_public_key`).
    pub fn set_public_key(&self, pk: &[uzk_g1_affine; 12]) -> Result<(), Error> {
        check(unsafe { uzk_vk_set_public_key(self.handle, pk.as_ptr()) })
    }
    pub fn n_pi(&self) -> usize { self.n_pi }
    pub fn proof_bytes(&self) -> usize { self.proof_bytes }
    /// `proofs`: m blobs of `PlonkProof::to_bytes_be`, back to back; `pi`: m x n_pi public inputs; `weights`: one element per proof,
    /// drawn by the caller AFTER it has the proofs (None only for one proof: weight 1).  Returns (L, R, status): status[i] != 0
    /// means proof i was malformed (1 a non-canonical word, 2 a point off the curve) and is in neither sum.
    pub fn fold(&self, proofs: &[u8], pi: &[Limbs], weights: Option<&[Limbs]>) -> Result<(uzk_g1_jac, uzk_g1_jac, Vec<u8>), Error> {
        if self.proof_bytes == 0 || proofs.len() % self.proof_bytes != 0 {
            return Err(Error::Parameter);
        }
        let m = proofs.len() / self.proof_bytes;
        if pi.len() != m * self.n_pi || weights.map_or(m > 1, |w| w.len() != m) {
            return Err(Error::Parameter);
        }
        let (mut left, mut right) = (uzk_g1_jac::default(), uzk_g1_jac::default());
        let mut status = vec![0u8; m.max(1)];
        let w_ptr = weights.map_or(std::ptr::null(), |w| w.as_ptr() as *const u64);
        check(unsafe {
            uzk_verify_fold(self.handle, proofs.as_ptr(), pi.as_ptr() as *const u64, m as u32, w_ptr, &mut left, &mut right, status.as_mut_ptr(),
                            std::ptr::null_mut())
        })?;
        status.truncate(m);
        Ok((left, right, status))
    }
}
impl Drop for VerifierKey {
    fn drop(&mut self) {
        unsafe { uzk_vk_release(self.handle) };
    }
}

/// What `Groth16Vk::fold` returns: the G1 arguments of the ONE product of m + 3 Miller loops that stands for m proofs.
pub struct Groth16Fold {
    /// rho_i A_i, canonical affine words (zeros for a proof with a nonzero status)
    pub a: Vec<uzk_g1_affine>,
    /// B_i in the wire form (zeros for a proof with a nonzero status)
    pub b: Vec<uzk_g2_affine>,
    /// (sum rho) alpha, sum rho_i X_i, sum rho_i C_i over the proofs with status 0
    pub alpha: uzk_g1_jac,
    pub x: uzk_g1_jac,
    pub c: uzk_g1_jac,
    /// 0 folded; 1 a word >= p; 2 a point off its curve; 3 B outside the subgroup
    pub status: Vec<u8>,
}

/// A Groth16 verifying key resident on the device (`uzk_g16_vk_create`), for batches of proofs.  The pairings are the caller's
/// (the library computes no pairing).  Process-wide; released on drop.
pub struct Groth16Vk {
    handle: u64,
    n_inputs: usize,
}
impl Groth16Vk {
    /// `desc` and everything it points to are read before this returns.
    pub fn create(desc: &uzk_g16_vk_desc) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_g16_vk_create(desc, &mut handle) })?;
        let (mut l, mut dev) = (0u32, 0 as c_int);
        if let Err(e) = check(unsafe { uzk_g16_vk_info(handle, &mut l, &mut dev) }) {
            unsafe { uzk_g16_vk_release(handle) };
            return Err(e);
        }
        Ok(Groth16Vk { handle, n_inputs: l as usize })
    }
    /// The key from its compressed bytes (`uzk_g16_vk_create_compressed`): a verifying key, or a proving key whose head is one.
    /// The points are decoded on the device; `validate` adds the subgroup check of beta, gamma and delta.
    pub fn from_compressed(key: &[u8], validate: bool) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_g16_vk_create_compressed(key.as_ptr(), key.len(), validate as c_int, &mut handle) })?;
        let (mut l, mut dev) = (0u32, 0 as c_int);
        if let Err(e) = check(unsafe { uzk_g16_vk_info(handle, &mut l, &mut dev) }) {
            unsafe { uzk_g16_vk_release(handle) };
            return Err(e);
        }
        Ok(Groth16Vk { handle, n_inputs: l as usize })
    }
    /// l, the constant one included.
    pub fn n_inputs(&self) -> usize { self.n_inputs }
    /// `proofs`: m blobs of `UZK_G16_PROOF_BYTES`, back to back; `public`: m x (l - 1) inputs; `weights`: one element per proof,
    /// drawn by the caller AFTER it has the proofs (None only for one proof: weight 1).
    pub fn fold(&self, proofs: &[u8], public: &[Limbs], weights: Option<&[Limbs]>) -> Result<Groth16Fold, Error> {
        let blob = UZK_G16_PROOF_BYTES as usize;
        if proofs.len() % blob != 0 {
            return Err(Error::Parameter);
        }
        let m = proofs.len() / blob;
        if public.len() != m * (self.n_inputs - 1) || weights.map_or(m > 1, |w| w.len() != m) {
            return Err(Error::Parameter);
        }
        let mut out = Groth16Fold {
            a: vec![uzk_g1_affine::default(); m.max(1)],
            b: vec![uzk_g2_affine::default(); m.max(1)],
            alpha: uzk_g1_jac::default(),
            x: uzk_g1_jac::default(),
            c: uzk_g1_jac::default(),
            status: vec![0u8; m.max(1)],
        };
        let w_ptr = weights.map_or(std::ptr::null(), |w| w.as_ptr() as *const u64);
        check(unsafe {
            uzk_g16_verify_fold(self.handle, proofs.as_ptr(), public.as_ptr() as *const u64, m as u32, w_ptr, out.a.as_mut_ptr(), out.b.as_mut_ptr(),
                                &mut out.alpha, &mut out.x, &mut out.c, out.status.as_mut_ptr())
        })?;
        out.a.truncate(m);
        out.b.truncate(m);
        out.status.truncate(m);
        Ok(out)
    }
    /// The arguments of `fold` and the key's beta, gamma, delta: the fold, then the product of its m + 3 pairings on the device
    /// (`uzk_g16_verify_batch`).  Returns (accepted, status): accepted iff every status is 0 and the product is one.
    pub fn verify_batch(&self, proofs: &[u8], public: &[Limbs], weights: Option<&[Limbs]>, g2: &[uzk_g2_affine; 3]) -> Result<(bool, Vec<u8>), Error> {
        let blob = UZK_G16_PROOF_BYTES as usize;
        if proofs.len() % blob != 0 {
            return Err(Error::Parameter);
        }
        let m = proofs.len() / blob;
        if public.len() != m * (self.n_inputs - 1) || weights.map_or(m > 1, |w| w.len() != m) {
            return Err(Error::Parameter);
        }
        let mut status = vec![0u8; m.max(1)];
        let mut accepted: c_int = 0;
        let w_ptr = weights.map_or(std::ptr::null(), |w| w.as_ptr() as *const u64);
        check(unsafe {
            uzk_g16_verify_batch(self.handle, proofs.as_ptr(), public.as_ptr() as *const u64, m as u32, w_ptr, g2.as_ptr(), status.as_mut_ptr(), &mut accepted)
        })?;
        status.truncate(m);
        Ok((accepted != 0, status))
    }
}

/// prod_i e(p_i, q_i) on the device (`uzk_pairing_product`): the element after the final exponentiation, and whether it is one.
/// Points at infinity (zeros) contribute 1; a point off its curve is a `Parameter` error.  Q's subgroup is the caller's business.
pub fn pairing_product(p: &[uzk_g1_affine], q: &[uzk_g2_affine]) -> Result<(uzk_gt, bool), Error> {
    if p.len() != q.len() || p.len() > UZK_PAIRING_MAX_PAIRS as usize {
        return Err(Error::Parameter);
    }
    let mut gt = uzk_gt::default();
    let mut one: c_int = 0;
    check(unsafe { uzk_pairing_product(p.as_ptr(), q.as_ptr(), p.len() as u32, &mut gt, &mut one) })?;
    Ok((gt, one != 0))
}
impl Drop for Groth16Vk {
    fn drop(&mut self) {
        unsafe { uzk_g16_vk_release(self.handle) };
    }
}

// ---- Baby Jubjub (ark_ed_on_bn254) and the Chaum-Pedersen reveal proofs over it ---------------------------------------------------
/// A point on the wire: x then y, the Montgomery words of `ark_bn254::Fr` (the element encoding of the Groth16 public signals).
pub type EdPoint = [Limbs; 2];
/// A reveal statement: e1, reveal, pk -- also the six public signals of the Groth16 reveal proof of the same statement.
pub type RevealStatement = [EdPoint; 3];

/// The status of every point (`uzk_ed_check_points`): 0 in the prime subgroup, 1 a coordinate word >= q, 2 off the curve, 3 on the
/// curve outside the subgroup.
pub fn ed_check_points(points: &[EdPoint]) -> Result<Vec<u8>, Error> {
    if points.is_empty() {
        return Err(Error::Parameter);
    }
    let mut status = vec![0u8; points.len()];
    check(unsafe { uzk_ed_check_points(points.as_ptr() as *const u64, points.len(), status.as_mut_ptr()) })?;
    Ok(status)
}

/// s_i P_i for 256-bit integers s_i as four little-endian words, not reduced (`uzk_ed_mul_batch`); one point serves every scalar.
pub fn ed_mul_batch(points: &[EdPoint], scalars: &[Limbs]) -> Result<Vec<EdPoint>, Error> {
    if scalars.is_empty() || (points.len() != scalars.len() && points.len() != 1) {
        return Err(Error::Parameter);
    }
    let stride = if points.len() == scalars.len() { 1 } else { 0 };
    let mut out = vec![[[0u64; 4]; 2]; scalars.len()];
    check(unsafe { uzk_ed_mul_batch(points.as_ptr() as *const u64, stride, scalars.as_ptr() as *const u64, scalars.len(), out.as_mut_ptr() as *mut u64) })?;
    Ok(out)
}

/// The sum over k rows of n points, card by card (`uzk_ed_sum_batch`); rows[k * n + j].
pub fn ed_sum_batch(rows: &[EdPoint], k: usize, n: usize) -> Result<Vec<EdPoint>, Error> {
    if k == 0 || n == 0 || rows.len() != k * n {
        return Err(Error::Parameter);
    }
    let mut out = vec![[[0u64; 4]; 2]; n];
    check(unsafe { uzk_ed_sum_batch(rows.as_ptr() as *const u64, k as u32, n as u32, out.as_mut_ptr() as *mut u64) })?;
    Ok(out)
}

/// e2_j minus the k reveals of card j (`uzk_ed_unmask_batch`); reveals[k * n + j].
pub fn ed_unmask_batch(e2: &[EdPoint], reveals: &[EdPoint], k: usize) -> Result<Vec<EdPoint>, Error> {
    let n = e2.len();
    if k == 0 || n == 0 || reveals.len() != k * n {
        return Err(Error::Parameter);
    }
    let mut out = vec![[[0u64; 4]; 2]; n];
    check(unsafe { uzk_ed_unmask_batch(e2.as_ptr() as *const u64, reveals.as_ptr() as *const u64, k as u32, n as u32, out.as_mut_ptr() as *mut u64) })?;
    Ok(out)
}

/// One player's reveals of m masked cards (`uzk_cp_reveal_prove_batch`): (reveal cards, pk, m proof blobs of UZK_CP_PROOF_BYTES).
/// `sk` and `omegas` are plain integers below the subgroup order; the caller draws one fresh omega per card.
pub fn cp_reveal_prove_batch(sk: &Limbs, e1: &[EdPoint], omegas: &[Limbs]) -> Result<(Vec<EdPoint>, EdPoint, Vec<u8>), Error> {
    let m = e1.len();
    if m == 0 || m > UZK_CP_MAX_BATCH as usize || omegas.len() != m {
        return Err(Error::Parameter);
    }
    let mut reveal = vec![[[0u64; 4]; 2]; m];
    let mut pk: EdPoint = [[0u64; 4]; 2];
    let mut proofs = vec![0u8; m * UZK_CP_PROOF_BYTES as usize];
    check(unsafe {
        uzk_cp_reveal_prove_batch(sk.as_ptr(), e1.as_ptr() as *const u64, omegas.as_ptr() as *const u64, m as u32, reveal.as_mut_ptr() as *mut u64,
                                  pk.as_mut_ptr() as *mut u64, proofs.as_mut_ptr())
    })?;
    Ok((reveal, pk, proofs))
}

/// The verdict byte of every (statement, proof) (`uzk_cp_reveal_verify_batch`): 0 accepted, 1 .. 3 a malformed point (as
/// `ed_check_points`), 4 the first equation fails, 5 the second.
pub fn cp_reveal_verify_batch(statements: &[RevealStatement], proofs: &[u8]) -> Result<Vec<u8>, Error> {
    let m = statements.len();
    if m == 0 || m > UZK_CP_MAX_BATCH as usize || proofs.len() != m * UZK_CP_PROOF_BYTES as usize {
        return Err(Error::Parameter);
    }
    let mut verdict = vec![0u8; m];
    check(unsafe { uzk_cp_reveal_verify_batch(statements.as_ptr() as *const u64, proofs.as_ptr(), m as u32, verdict.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(verdict)
}

/// `cp_reveal_prove_batch` with the zk-friendly challenge (`uzk_cp_reveal_prove0_batch`, dl.rs `prove0`): the Anemoi-Jive hash of the
/// twelve coordinates in place of the Keccak transcript; the same blob.
pub fn cp_reveal_prove0_batch(sk: &Limbs, e1: &[EdPoint], omegas: &[Limbs]) -> Result<(Vec<EdPoint>, EdPoint, Vec<u8>), Error> {
    let m = e1.len();
    if m == 0 || m > UZK_CP_MAX_BATCH as usize || omegas.len() != m {
        return Err(Error::Parameter);
    }
    let mut reveal = vec![[[0u64; 4]; 2]; m];
    let mut pk: EdPoint = [[0u64; 4]; 2];
    let mut proofs = vec![0u8; m * UZK_CP_PROOF_BYTES as usize];
    check(unsafe {
        uzk_cp_reveal_prove0_batch(sk.as_ptr(), e1.as_ptr() as *const u64, omegas.as_ptr() as *const u64, m as u32, reveal.as_mut_ptr() as *mut u64,
                                   pk.as_mut_ptr() as *mut u64, proofs.as_mut_ptr())
    })?;
    Ok((reveal, pk, proofs))
}

/// `cp_reveal_verify_batch` for the proofs of `prove0` (`uzk_cp_reveal_verify0_batch`): the same verdict bytes.
pub fn cp_reveal_verify0_batch(statements: &[RevealStatement], proofs: &[u8]) -> Result<Vec<u8>, Error> {
    let m = statements.len();
    if m == 0 || m > UZK_CP_MAX_BATCH as usize || proofs.len() != m * UZK_CP_PROOF_BYTES as usize {
        return Err(Error::Parameter);
    }
    let mut verdict = vec![0u8; m];
    check(unsafe { uzk_cp_reveal_verify0_batch(statements.as_ptr() as *const u64, proofs.as_ptr(), m as u32, verdict.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok(verdict)
}

// ---- Anemoi-Jive: hashes, the stream cipher, their traces ----------------------------------------------------------------------------
/// One permutation's share of a trace: before (x0 x1 y0 y1), the state after each of the 14 rounds' S-boxes, after.
pub type AnemoiTraceBlock = [Limbs; 64];

/// How many permutations one item of `len` inputs runs (`uzk_anemoi_permutations`); `out_len` 0: a hash.
pub fn anemoi_permutations(len: usize, out_len: usize) -> usize {
    unsafe { uzk_anemoi_permutations(len as u32, out_len as u32) as usize }
}

/// One permutation of every state x0 x1 y0 y1 (`uzk_anemoi_permute_batch`).
pub fn anemoi_permute_batch(states: &[[Limbs; 4]]) -> Result<Vec<[Limbs; 4]>, Error> {
    if states.is_empty() || states.len() > UZK_ANEMOI_MAX_BATCH as usize {
        return Err(Error::Parameter);
    }
    let mut out = vec![[[0u64; 4]; 4]; states.len()];
    check(unsafe { uzk_anemoi_permute_batch(states.as_ptr() as *const u64, states.len(), out.as_mut_ptr() as *mut u64) })?;
    Ok(out)
}

/// The hash of every input (`uzk_anemoi_hash_batch`): `inputs` holds n items of `len` elements each; with `want_trace` also
/// n x P trace blocks, P = `anemoi_permutations(len, 0)`.
pub fn anemoi_hash_batch(inputs: &[Limbs], len: usize, n: usize, want_trace: bool) -> Result<(Vec<Limbs>, Option<Vec<AnemoiTraceBlock>>), Error> {
    if n == 0 || n > UZK_ANEMOI_MAX_BATCH as usize || len > UZK_ANEMOI_MAX_INPUT as usize || inputs.len() != n * len {
        return Err(Error::Parameter);
    }
    let mut out = vec![[0u64; 4]; n];
    let mut trace = if want_trace { Some(vec![[[0u64; 4]; 64]; n * anemoi_permutations(len, 0)]) } else { None };
    let tp = trace.as_mut().map_or(std::ptr::null_mut(), |t| t.as_mut_ptr() as *mut u64);
    check(unsafe { uzk_anemoi_hash_batch(inputs.as_ptr() as *const u64, len as u32, n, out.as_mut_ptr() as *mut u64, tp) })?;
    Ok((out, trace))
}

/// `out_len` outputs of the stream cipher per input (`uzk_anemoi_stream_batch`); with `want_trace` also n x P trace blocks,
/// P = `anemoi_permutations(len, out_len)`.
pub fn anemoi_stream_batch(inputs: &[Limbs], len: usize, n: usize, out_len: usize, want_trace: bool) -> Result<(Vec<Limbs>, Option<Vec<AnemoiTraceBlock>>), Error> {
    if n == 0 || n > UZK_ANEMOI_MAX_BATCH as usize || len > UZK_ANEMOI_MAX_INPUT as usize || inputs.len() != n * len || out_len == 0 ||
        out_len > UZK_ANEMOI_MAX_OUTPUT as usize
    {
        return Err(Error::Parameter);
    }
    let mut out = vec![[0u64; 4]; n * out_len];
    let mut trace = if want_trace { Some(vec![[[0u64; 4]; 64]; n * anemoi_permutations(len, out_len)]) } else { None };
    let tp = trace.as_mut().map_or(std::ptr::null_mut(), |t| t.as_mut_ptr() as *mut u64);
    check(unsafe { uzk_anemoi_stream_batch(inputs.as_ptr() as *const u64, len as u32, n, out_len as u32, out.as_mut_ptr() as *mut u64, tp) })?;
    Ok((out, trace))
}

// ---- masking a card and the remask of a shuffle --------------------------------------------------------------------------------------
/// One table of a remask key: [84][4] entries of (x, y, d x y).
pub type RemarkTable = Vec<[Limbs; 3]>;
/// The result of `RemarkKey::remark_batch`: e1 and e2 of the new deck in output order, and the trace (n x 84 entries of
/// c2.x, c2.y, c1.x, c1.y in input card order) where it was asked for.
pub type RemarkOutput = (Vec<EdPoint>, Vec<EdPoint>, Option<Vec<[Limbs; 4]>>);

/// The remask tables of one joint key, resident on the current context's device (`uzk_remark_key_create`); released on drop.
pub struct RemarkKey {
    handle: u64,
}
impl RemarkKey {
    pub fn new(pk: &EdPoint) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_remark_key_create(pk.as_ptr() as *const u64, &mut handle) })?;
        Ok(Self { handle })
    }
    /// (T_pk, T_G): x, y, d x y of every entry (`uzk_remark_key_tables`) -- what compute_shuffle_public_key_selectors and
    /// load_shuffle_remark_parameters lay out over the circuit's domain.
    pub fn tables(&self) -> Result<(RemarkTable, RemarkTable), Error> {
        let entries = UZK_REMARK_ITERATIONS as usize * 4;
        let mut pk = vec![[[0u64; 4]; 3]; entries];
        let mut gen = vec![[[0u64; 4]; 3]; entries];
        check(unsafe { uzk_remark_key_tables(self.handle, pk.as_mut_ptr() as *mut u64, gen.as_mut_ptr() as *mut u64) })?;
        Ok((pk, gen))
    }
    /// Every card remasked by its 84 digits, then out[i] = remasked[perm[i]] (`uzk_remark_batch`).  digits: n x 84 bytes (bits 0, 1: j;
    /// bit 2 set: add, clear: subtract); perm: a permutation of 0 .. n-1, or None for the identity.
    pub fn remark_batch(&self, e1: &[EdPoint], e2: &[EdPoint], digits: &[u8], perm: Option<&[u32]>, want_trace: bool) -> Result<RemarkOutput, Error> {
        let n = e1.len();
        let iters = UZK_REMARK_ITERATIONS as usize;
        if n == 0 || n > UZK_ED_MAX_BATCH as usize || e2.len() != n || digits.len() != n * iters || perm.map_or(false, |p| p.len() != n) {
            return Err(Error::Parameter);
        }
        let mut o1 = vec![[[0u64; 4]; 2]; n];
        let mut o2 = vec![[[0u64; 4]; 2]; n];
        let mut trace = if want_trace { Some(vec![[[0u64; 4]; 4]; n * iters]) } else { None };
        let trace_ptr = trace.as_mut().map_or(std::ptr::null_mut(), |t| t.as_mut_ptr() as *mut u64);
        let perm_ptr = perm.map_or(std::ptr::null(), |p| p.as_ptr());
        check(unsafe {
            uzk_remark_batch(self.handle, e1.as_ptr() as *const u64, e2.as_ptr() as *const u64, digits.as_ptr(), perm_ptr, n as u32, o1.as_mut_ptr() as *mut u64,
                             o2.as_mut_ptr() as *mut u64, trace_ptr)
        })?;
        Ok((o1, o2, trace))
    }
}
impl Drop for RemarkKey {
    fn drop(&mut self) {
        unsafe { uzk_remark_key_release(self.handle) };
    }
}

/// The shape of zshuffle's circuit for a deck of `cards` (`uzk_shuffle_cs_info`, host only): (size, n, num_vars, the public-input rows).
pub fn shuffle_cs_info(cards: u32) -> Result<(u32, u32, u32, Vec<u32>), Error> {
    let (mut size, mut n, mut vars, mut pis) = (0u32, 0u32, 0u32, 0u32);
    check(unsafe { uzk_shuffle_cs_info(cards, &mut size, &mut n, &mut vars, &mut pis, std::ptr::null_mut()) })?;
    let mut rows = vec![0u32; pis as usize];
    check(unsafe { uzk_shuffle_cs_info(cards, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), rows.as_mut_ptr()) })?;
    Ok((size, n, vars, rows))
}

/// The witnesses of a batch of decks, resident on the device until dropped: what `uzk_prove_round1` takes with `inputs_on_device`.
pub struct ShuffleWitness {
    pub d_witness: *mut std::os::raw::c_void,
    pub d_wsel: *mut std::os::raw::c_void,
    /// batch x 8 cards online inputs, in the order of `verify_shuffle`
    pub pi_values: Vec<Limbs>,
    pub e1_out: Vec<EdPoint>,
    pub e2_out: Vec<EdPoint>,
}
impl Drop for ShuffleWitness {
    fn drop(&mut self) {
        unsafe {
            uzk_dev_free(self.d_witness);
            uzk_dev_free(self.d_wsel);
        }
    }
}

/// zshuffle's circuit for one deck size, laid out and preprocessed on the device (`uzk_shuffle_circuit_create`): an ordinary circuit
/// handle for the five rounds, plus the layout the witness kernels read.  Released on drop.
pub struct ShuffleCircuit {
    handle: u64,
    cards: u32,
    n: u32,
    /// the 32 commitments of the verifier key: cm_q (9), cm_s (5), cm_qb, cm_prk (4), cm_q_ecc, cm_shuffle_generator (12)
    pub commitments: Vec<uzk_g1_jac>,
}
impl ShuffleCircuit {
    /// `desc` and everything it points to are read before this returns.
    pub fn create(desc: &uzk_shuffle_circuit_desc) -> Result<Self, Error> {
        let (_, n, _, _) = shuffle_cs_info(desc.cards)?;
        let mut handle = 0u64;
        let mut commitments = vec![uzk_g1_jac::default(); UZK_SHUFFLE_CS_KEY_COMMITMENTS as usize];
        check(unsafe { uzk_shuffle_circuit_create(desc, &mut handle, commitments.as_mut_ptr()) })?;
        Ok(Self { handle, cards: desc.cards, n, commitments })
    }
    pub fn handle(&self) -> u64 { self.handle }
    pub fn n(&self) -> u32 { self.n }
    /// The game's public-key tables from the key's resident T_pk (`uzk_shuffle_circuit_set_key`): their 12 commitments.
    pub fn set_key(&self, key: &RemarkKey) -> Result<Vec<uzk_g1_jac>, Error> {
        let mut cms = vec![uzk_g1_jac::default(); 12];
        check(unsafe { uzk_shuffle_circuit_set_key(self.handle, key.handle, cms.as_mut_ptr()) })?;
        Ok(cms)
    }
    /// Remasks and permutes `e1.len() / cards` decks and leaves their witnesses on the device (`uzk_shuffle_witness_batch`).
    pub fn witness_batch(&self, key: &RemarkKey, e1: &[EdPoint], e2: &[EdPoint], digits: &[u8], perms: Option<&[u32]>) -> Result<ShuffleWitness, Error> {
        let cards = self.cards as usize;
        let total = e1.len();
        let iters = UZK_REMARK_ITERATIONS as usize;
        if total == 0 || total % cards != 0 || e2.len() != total || digits.len() != total * iters || perms.map_or(false, |p| p.len() != total) {
            return Err(Error::Parameter);
        }
        let batch = total / cards;
        let n = self.n as usize;
        let mut w = ShuffleWitness { d_witness: std::ptr::null_mut(), d_wsel: std::ptr::null_mut(), pi_values: vec![[0u64; 4]; 8 * total],
                                     e1_out: vec![[[0u64; 4]; 2]; total], e2_out: vec![[[0u64; 4]; 2]; total] };
        check(unsafe { uzk_dev_alloc(32 * 5 * n * batch, &mut w.d_witness) })?;
        check(unsafe { uzk_dev_alloc(32 * 3 * n * batch, &mut w.d_wsel) })?;
        let perm_ptr = perms.map_or(std::ptr::null(), |p| p.as_ptr());
        check(unsafe {
            uzk_shuffle_witness_batch(self.handle, key.handle, e1.as_ptr() as *const u64, e2.as_ptr() as *const u64, digits.as_ptr(), perm_ptr, self.cards,
                                      batch as u32, w.d_witness, w.d_wsel, w.pi_values.as_mut_ptr() as *mut u64, w.e1_out.as_mut_ptr() as *mut u64,
                                      w.e2_out.as_mut_ptr() as *mut u64)
        })?;
        Ok(w)
    }
}
impl Drop for ShuffleCircuit {
    fn drop(&mut self) {
        unsafe { uzk_circuit_release(self.handle) };
    }
}

/// The shape of zmatchmaking's circuit for `players` (`uzk_match_cs_info`, host only): (gates, n, variables, the public-input rows).
pub fn match_cs_info(players: u32) -> Result<(u32, u32, u32, Vec<u32>), Error> {
    let (mut size, mut n, mut vars, mut pis) = (0u32, 0u32, 0u32, 0u32);
    check(unsafe { uzk_match_cs_info(players, &mut size, &mut n, &mut vars, &mut pis, std::ptr::null_mut()) })?;
    let mut rows = vec![0u32; pis as usize];
    check(unsafe { uzk_match_cs_info(players, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), rows.as_mut_ptr()) })?;
    Ok((size, n, vars, rows))
}

/// The witnesses of a batch of matches, resident on the device until dropped: what `uzk_prove_round1` takes with `inputs_on_device`
/// and no wire selectors.
pub struct MatchWitness {
    pub d_witness: *mut std::os::raw::c_void,
    /// batch x (2 players + 2) online inputs, in the order of `verify_matchmaking`: inputs, outputs, random number, commitment
    pub pi_values: Vec<Limbs>,
    /// batch x players: the matched order
    pub outputs: Vec<Limbs>,
    /// batch: the Anemoi hash of every seed
    pub commitments: Vec<Limbs>,
}
impl Drop for MatchWitness {
    fn drop(&mut self) {
        unsafe { uzk_dev_free(self.d_witness) };
    }
}

/// zmatchmaking's circuit for one number of players, laid out and preprocessed on the device (`uzk_match_circuit_create`): an ordinary
/// circuit handle without the shuffle feature for the five rounds, plus the layout the witness kernels read.  Released on drop.
pub struct MatchCircuit {
    handle: u64,
    players: u32,
    n: u32,
    /// the 19 commitments of the verifier key: cm_q (9), cm_s (5), cm_qb, cm_prk (4)
    pub commitments: Vec<uzk_g1_jac>,
}
impl MatchCircuit {
    /// `desc` and everything it points to are read before this returns.
    pub fn create(desc: &uzk_match_circuit_desc) -> Result<Self, Error> {
        let (_, n, _, _) = match_cs_info(desc.players)?;
        let mut handle = 0u64;
        let mut commitments = vec![uzk_g1_jac::default(); UZK_MATCH_CS_KEY_COMMITMENTS as usize];
        check(unsafe { uzk_match_circuit_create(desc, &mut handle, commitments.as_mut_ptr()) })?;
        Ok(Self { handle, players: desc.players, n, commitments })
    }
    pub fn handle(&self) -> u64 { self.handle }
    pub fn n(&self) -> u32 { self.n }
    pub fn players(&self) -> u32 { self.players }
    /// Hashes the seeds, runs the stream ciphers and leaves the witnesses of `seeds.len()` matches on the device
    /// (`uzk_match_witness_batch`).  Elements are Montgomery limbs below r.
    pub fn witness_batch(&self, inputs: &[Limbs], seeds: &[Limbs], randoms: &[Limbs]) -> Result<MatchWitness, Error> {
        let players = self.players as usize;
        let batch = seeds.len();
        if batch == 0 || batch > UZK_MATCH_CS_MAX_BATCH as usize || randoms.len() != batch || inputs.len() != batch * players {
            return Err(Error::Parameter);
        }
        let n = self.n as usize;
        let mut w = MatchWitness { d_witness: std::ptr::null_mut(), pi_values: vec![[0u64; 4]; batch * (2 * players + 2)],
                                   outputs: vec![[0u64; 4]; batch * players], commitments: vec![[0u64; 4]; batch] };
        check(unsafe { uzk_dev_alloc(32 * 5 * n * batch, &mut w.d_witness) })?;
        check(unsafe {
            uzk_match_witness_batch(self.handle, inputs.as_ptr() as *const u64, seeds.as_ptr() as *const u64, randoms.as_ptr() as *const u64, self.players,
                                    batch as u32, w.d_witness, w.pi_values.as_mut_ptr() as *mut u64, w.outputs.as_mut_ptr() as *mut u64,
                                    w.commitments.as_mut_ptr() as *mut u64)
        })?;
        Ok(w)
    }
}
impl Drop for MatchCircuit {
    fn drop(&mut self) {
        unsafe { uzk_circuit_release(self.handle) };
    }
}

/// n_vars, n_inputs, n_constraints, the domain and the non-zero counts of A, B, C of the reveal circuit (`uzk_reveal_cs_info`; host only).
pub fn reveal_cs_info() -> Result<(u32, u32, u32, u64, [u64; 3]), Error> {
    let (mut m, mut l, mut nc, mut n, mut nnz) = (0u32, 0u32, 0u32, 0u64, [0u64; 3]);
    check(unsafe { uzk_reveal_cs_info(&mut m, &mut l, &mut nc, &mut n, nnz.as_mut_ptr()) })?;
    Ok((m, l, nc, n, nnz))
}

/// The reveal circuit's matrices A, B, C in CSR: (row_ptr, col, val) each (`uzk_reveal_cs_matrices`; host only).
pub fn reveal_cs_matrices() -> Result<Vec<(Vec<u64>, Vec<u32>, Vec<Limbs>)>, Error> {
    let (_, _, nc, _, nnz) = reveal_cs_info()?;
    let mut mats: Vec<(Vec<u64>, Vec<u32>, Vec<Limbs>)> =
        nnz.iter().map(|k| (vec![0u64; nc as usize + 1], vec![0u32; *k as usize], vec![[0u64; 4]; *k as usize])).collect();
    let row_ptr: Vec<*mut u64> = mats.iter_mut().map(|m| m.0.as_mut_ptr()).collect();
    let col: Vec<*mut u32> = mats.iter_mut().map(|m| m.1.as_mut_ptr()).collect();
    let val: Vec<*mut u64> = mats.iter_mut().map(|m| m.2.as_mut_ptr() as *mut u64).collect();
    check(unsafe { uzk_reveal_cs_matrices(row_ptr.as_ptr(), col.as_ptr(), val.as_ptr()) })?;
    Ok(mats)
}

/// The six public inputs of a reveal proof behind the leading one: e1.x e1.y reveal.x reveal.y pk.x pk.y.
pub type RevealSnarkStatement = [Limbs; 6];

/// The assignments of a batch of cards, resident on the device until dropped: what `uzk_g16_prove_batch_device` reads.
pub struct RevealWitness {
    pub d_z: *mut std::os::raw::c_void,
    pub statements: Vec<RevealSnarkStatement>,
}
impl Drop for RevealWitness {
    fn drop(&mut self) {
        unsafe { uzk_dev_free(self.d_z) };
    }
}

/// The reveal circuit joined to the points of a Groth16 proving key (`uzk_reveal_circuit_create`): its own matrices, the resident key
/// and the constants of the fixed-base chain.  Released on drop, the inner key with it.
pub struct RevealCircuit {
    handle: u64,
    key: u64,
}
impl RevealCircuit {
    /// `desc`: the key's points, the matrix pointers null; everything it points to is read before this returns.
    pub fn create(desc: &uzk_g16_key_desc) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_reveal_circuit_create(desc, &mut handle) })?;
        let mut key = 0u64;
        if let Err(e) = check(unsafe { uzk_reveal_circuit_key(handle, &mut key) }) {
            unsafe { uzk_reveal_circuit_release(handle) };
            return Err(e);
        }
        Ok(Self { handle, key })
    }
    /// The circuit over a compressed `ProvingKey<Bn254>` (groth16_pk.bin as it lies on disk): every point of the key is decoded on
    /// the device, all G1 encodings in one launch and all G2 encodings in one (`uzk_reveal_circuit_create_compressed`).  `validate`
    /// adds the subgroup check of the G2 points; a point that fails any check refuses the key (`last_error` names it).
    pub fn from_compressed(pk: &[u8], validate: bool) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_reveal_circuit_create_compressed(pk.as_ptr(), pk.len(), validate as c_int, &mut handle) })?;
        let mut key = 0u64;
        if let Err(e) = check(unsafe { uzk_reveal_circuit_key(handle, &mut key) }) {
            unsafe { uzk_reveal_circuit_release(handle) };
            return Err(e);
        }
        Ok(Self { handle, key })
    }
    pub fn handle(&self) -> u64 { self.handle }
    /// the inner Groth16 key, for the `uzk_g16_*` entry points; it lives as long as the circuit
    pub fn key(&self) -> u64 { self.key }
    /// The assignments of `e1.len()` cards under one secret, left on the device (`uzk_reveal_witness_batch`).  `sk`: a plain integer.
    pub fn witness_batch(&self, sk: &Limbs, e1: &[EdPoint]) -> Result<RevealWitness, Error> {
        let m = e1.len();
        if m == 0 || m > UZK_REVEAL_CS_MAX_BATCH as usize {
            return Err(Error::Parameter);
        }
        let mut w = RevealWitness { d_z: std::ptr::null_mut(), statements: vec![[[0u64; 4]; 6]; m] };
        check(unsafe { uzk_dev_alloc(32 * UZK_REVEAL_CS_VARS as usize * m, &mut w.d_z) })?;
        check(unsafe { uzk_reveal_witness_batch(self.handle, sk.as_ptr(), e1.as_ptr() as *const u64, m as u32, w.d_z, w.statements.as_mut_ptr() as *mut u64) })?;
        Ok(w)
    }
    /// Witness and proof of every card in one call (`uzk_reveal_prove_snark_batch`): `r`, `s` one pair of blinds per card
    /// (Montgomery limbs), drawn by the caller.
    pub fn prove_snark_batch(&self, sk: &Limbs, e1: &[EdPoint], r: &[Limbs], s: &[Limbs]) -> Result<(Vec<RevealSnarkStatement>, Vec<uzk_g16_proof>), Error> {
        let m = e1.len();
        if m == 0 || m > UZK_REVEAL_CS_MAX_BATCH as usize || r.len() != m || s.len() != m {
            return Err(Error::Parameter);
        }
        let mut statements = vec![[[0u64; 4]; 6]; m];
        let mut proofs = vec![uzk_g16_proof::default(); m];
        check(unsafe {
            uzk_reveal_prove_snark_batch(self.handle, sk.as_ptr(), e1.as_ptr() as *const u64, r.as_ptr() as *const u64, s.as_ptr() as *const u64, m as u32,
                                         statements.as_mut_ptr() as *mut u64, proofs.as_mut_ptr())
        })?;
        Ok((statements, proofs))
    }
    /// The same proofs finished and encoded on the device (`uzk_reveal_prove_snark_batch_finish`): per card the statement, the proof in
    /// the struct layout and the `UZK_G16_PROOF_BYTES` blob `uzk_g16_verify_batch` reads (eight 32-byte big-endian words in the EVM
    /// order), with no curve arithmetic on the host.
    pub fn prove_snark_finish(&self, sk: &Limbs, e1: &[EdPoint], r: &[Limbs], s: &[Limbs]) -> Result<(Vec<RevealSnarkStatement>, Vec<uzk_g16_proof>, Vec<u8>), Error> {
        let m = e1.len();
        if m == 0 || m > UZK_REVEAL_CS_MAX_BATCH as usize || r.len() != m || s.len() != m {
            return Err(Error::Parameter);
        }
        let mut statements = vec![[[0u64; 4]; 6]; m];
        let mut proofs = vec![uzk_g16_proof::default(); m];
        let mut blobs = vec![0u8; m * UZK_G16_PROOF_BYTES as usize];
        check(unsafe {
            uzk_reveal_prove_snark_batch_finish(self.handle, sk.as_ptr(), e1.as_ptr() as *const u64, r.as_ptr() as *const u64, s.as_ptr() as *const u64, m as u32,
                                                statements.as_mut_ptr() as *mut u64, proofs.as_mut_ptr(), blobs.as_mut_ptr(), std::ptr::null_mut())
        })?;
        Ok((statements, proofs, blobs))
    }
    /// the inner key as a borrowed `Groth16Key`: it lives as long as the circuit
    pub fn groth16_key(&self) -> Groth16Key<'_> {
        Groth16Key { handle: self.key, _owner: std::marker::PhantomData }
    }
}

/// A Groth16 proving key resident on the device, borrowed from the object that owns it (`RevealCircuit::groth16_key`).
pub struct Groth16Key<'a> {
    handle: u64,
    _owner: std::marker::PhantomData<&'a RevealCircuit>,
}
impl<'a> Groth16Key<'a> {
    pub fn handle(&self) -> u64 { self.handle }
    /// (n_vars, n_inputs, n_constraints, domain) of the key (`uzk_g16_key_info`)
    pub fn info(&self) -> Result<(u32, u32, u32, u64), Error> {
        let (mut m, mut l, mut nc, mut n) = (0u32, 0u32, 0u32, 0u64);
        check(unsafe { uzk_g16_key_info(self.handle, &mut m, &mut l, &mut nc, &mut n, std::ptr::null_mut()) })?;
        Ok((m, l, nc, n))
    }
    /// `r.len()` proofs over host assignments `z` (`r.len()` x n_vars Montgomery elements, z[0] = 1 each), finished and encoded on the
    /// device (`uzk_g16_prove_batch_finish`): the proofs in the struct layout and their `UZK_G16_PROOF_BYTES` blobs.
    pub fn prove_finish(&self, z: &[Limbs], r: &[Limbs], s: &[Limbs]) -> Result<(Vec<uzk_g16_proof>, Vec<u8>), Error> {
        let batch = r.len();
        let (m, _, _, _) = self.info()?;
        if batch == 0 || s.len() != batch || z.len() != batch * m as usize {
            return Err(Error::Parameter);
        }
        let mut proofs = vec![uzk_g16_proof::default(); batch];
        let mut blobs = vec![0u8; batch * UZK_G16_PROOF_BYTES as usize];
        check(unsafe {
            uzk_g16_prove_batch_finish(self.handle, z.as_ptr() as *const std::os::raw::c_void, 0, r.as_ptr() as *const u64, s.as_ptr() as *const u64, batch as u32,
                                       proofs.as_mut_ptr(), blobs.as_mut_ptr(), std::ptr::null_mut())
        })?;
        Ok((proofs, blobs))
    }
}
impl Drop for RevealCircuit {
    fn drop(&mut self) {
        unsafe { uzk_reveal_circuit_release(self.handle) };
    }
}

/// m cards masked under the joint key (`uzk_cp_mask_prove_batch`): (e1, e2, m proof blobs of UZK_CP_PROOF_BYTES).  `rs` and `omegas`
/// are plain integers below the subgroup order, drawn by the caller.
pub fn cp_mask_prove_batch(pk: &EdPoint, cards: &[EdPoint], rs: &[Limbs], omegas: &[Limbs]) -> Result<(Vec<EdPoint>, Vec<EdPoint>, Vec<u8>), Error> {
    let m = cards.len();
    if m == 0 || m > UZK_CP_MAX_BATCH as usize || rs.len() != m || omegas.len() != m {
        return Err(Error::Parameter);
    }
    let mut e1 = vec![[[0u64; 4]; 2]; m];
    let mut e2 = vec![[[0u64; 4]; 2]; m];
    let mut proofs = vec![0u8; m * UZK_CP_PROOF_BYTES as usize];
    check(unsafe {
        uzk_cp_mask_prove_batch(pk.as_ptr() as *const u64, cards.as_ptr() as *const u64, rs.as_ptr() as *const u64, omegas.as_ptr() as *const u64, m as u32,
                                e1.as_mut_ptr() as *mut u64, e2.as_mut_ptr() as *mut u64, proofs.as_mut_ptr())
    })?;
    Ok((e1, e2, proofs))
}

/// The verdict byte of every (card, masked card, proof) under the joint key (`uzk_cp_mask_verify_batch`): 0 accepted, 1 .. 3 a
/// malformed point among pk, card, e1, e2, a, b, 4 the first equation fails, 5 the second.
pub fn cp_mask_verify_batch(pk: &EdPoint, cards: &[EdPoint], e1: &[EdPoint], e2: &[EdPoint], proofs: &[u8]) -> Result<Vec<u8>, Error> {
    let m = cards.len();
    if m == 0 || m > UZK_CP_MAX_BATCH as usize || e1.len() != m || e2.len() != m || proofs.len() != m * UZK_CP_PROOF_BYTES as usize {
        return Err(Error::Parameter);
    }
    let mut verdict = vec![0u8; m];
    check(unsafe {
        uzk_cp_mask_verify_batch(pk.as_ptr() as *const u64, cards.as_ptr() as *const u64, e1.as_ptr() as *const u64, e2.as_ptr() as *const u64, proofs.as_ptr(),
                                 m as u32, verdict.as_mut_ptr(), std::ptr::null_mut())
    })?;
    Ok(verdict)
}

/// How provers of ONE proof made from now on are shared between threads (`uzk_coalesce_config`): the library runs round calls of
/// several threads that stand at the same round of proofs over the same circuit as one lockstep launch sequence.  On by default
/// (at most 8 proofs per sequence, the provers at work spread over 4 sequences, 2000 us gathering wait -- include/uzkge_gpu.h; 0 = a default);
/// `max_lanes` <= 1 switches it off.
pub fn coalesce_config(max_lanes: u32, gather_wait_us: u32, straggler_wait_us: u32, groups: u32) -> Result<(), Error> {
    check(unsafe { uzk_coalesce_config(max_lanes, gather_wait_us, straggler_wait_us, groups) })
}

/// The device buffers of `batch` proofs in lockstep over circuits of size n (`uzk_prover_create`) and the five rounds.  Per-proof
/// arrays are [batch][..]; lengths are checked here and again by the library (a short slice is a `Parameter` error, never a read
/// or write past it).  `batch` = 1 is a SHARED prover: each thread keeps its own and calls the rounds of its own proof, and the
/// library merges the calls of threads that prove over the same circuit at the same time.
pub struct Prover {
    handle: u64,
    n: usize,
    batch: usize,
}
impl Prover {
    pub fn new(n: u32, batch: u32) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_prover_create(n, batch, &mut handle) })?;
        Ok(Prover { handle, n: n as usize, batch: batch as usize })
    }
    /// A prover that owns its lanes whatever `batch` is (`uzk_prover_create_private`): its proofs run alone on the calling
    /// context's stream (latency measurements, diagnostics).
    pub fn new_private(n: u32, batch: u32) -> Result<Self, Error> {
        let mut handle = 0u64;
        check(unsafe { uzk_prover_create_private(n, batch, &mut handle) })?;
        Ok(Prover { handle, n: n as usize, batch: batch as usize })
    }
    /// prover.rs:151-192.  witness: batch x 5n; wsel: batch x 3n or empty; hiding: 5 (+3); blinds: batch x (5 | 8) x 3.
    #[allow(clippy::too_many_arguments)]
    pub fn round1(&self, circuit: &Circuit, witness: &[Limbs], wsel: &[Limbs], pi_index: &[u32], pi_value: &[Limbs], hiding: &[u32], blinds: &[Limbs]) -> Result<Vec<uzk_g1_jac>, Error> {
        let n_first = if wsel.is_empty() { 5 } else { 8 };
        if witness.len() != self.batch * 5 * self.n || (!wsel.is_empty() && wsel.len() != self.batch * 3 * self.n) || hiding.len() != n_first
            || blinds.len() != self.batch * n_first * 3 || pi_value.len() != self.batch * pi_index.len() {
            return Err(Error::Parameter);
        }
        let mut out = vec![uzk_g1_jac::default(); self.batch * n_first];
        let wsel_ptr = if wsel.is_empty() { std::ptr::null() } else { wsel.as_ptr() as *const c_void };
        check(unsafe {
            uzk_prove_round1(self.handle, circuit.handle, witness.as_ptr() as *const c_void, wsel_ptr, 0, pi_index.as_ptr(), pi_value.as_ptr() as *const u64,
                             pi_index.len() as u32, hiding.as_ptr(), blinds.as_ptr() as *const u64, out.as_mut_ptr())
        })?;
        Ok(out)
    }
    /// prover.rs:194-209 for every proof of the batch: beta, gamma: one each; blinds_z: three each; returns cm_z per proof.
    pub fn round2(&self, beta: &[Limbs], gamma: &[Limbs], blinds_z: &[Limbs]) -> Result<Vec<uzk_g1_jac>, Error> {
        if beta.len() != self.batch || gamma.len() != self.batch || blinds_z.len() != 3 * self.batch {
            return Err(Error::Parameter);
        }
        let mut out = vec![uzk_g1_jac::default(); self.batch];
        check(unsafe { uzk_prove_round2(self.handle, beta.as_ptr() as *const u64, gamma.as_ptr() as *const u64, blinds_z.as_ptr() as *const u64, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// prover.rs:211-239: alpha: one per proof; t_rands: five per proof; returns the five commitments of t's chunks per proof.
    pub fn round3(&self, alpha: &[Limbs], t_rands: &[Limbs]) -> Result<Vec<uzk_g1_jac>, Error> {
        if alpha.len() != self.batch || t_rands.len() != 5 * self.batch {
            return Err(Error::Parameter);
        }
        let mut out = vec![uzk_g1_jac::default(); 5 * self.batch];
        check(unsafe { uzk_prove_round3(self.handle, alpha.as_ptr() as *const u64, t_rands.as_ptr() as *const u64, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// prover.rs:241-273: zeta: one per proof; returns `per` evaluations per proof, packed: 19 for a circuit with the shuffle
    /// feature's terms (`shuffle`), 15 without.  The library is told how many elements the buffer holds and refuses the round
    /// (`Parameter`) when the circuit of the proof gives more.
    pub fn round4(&self, zeta: &[Limbs], shuffle: bool) -> Result<Vec<Limbs>, Error> {
        if zeta.len() != self.batch {
            return Err(Error::Parameter);
        }
        let per = if shuffle { 19 } else { 15 };
        let mut out = vec![[0u64; 4]; per * self.batch];
        check(unsafe { uzk_prove_round4(self.handle, zeta.as_ptr() as *const u64, out.as_mut_ptr() as *mut u64, out.len()) })?;
        Ok(out)
    }
    /// prover.rs:296-372: r_scalars: 19 | 43 per proof (the order of uzk_prove_round5); the two opening challenges: one each per
    /// proof; returns the two opening commitments per proof.  The library checks the count against the circuit of the proof.
    pub fn round5(&self, r_scalars: &[Limbs], alpha_zeta: &[Limbs], alpha_zeta_omega: &[Limbs]) -> Result<Vec<uzk_g1_jac>, Error> {
        if alpha_zeta.len() != self.batch || alpha_zeta_omega.len() != self.batch || (r_scalars.len() != 19 * self.batch && r_scalars.len() != 43 * self.batch) {
            return Err(Error::Parameter);
        }
        let mut out = vec![uzk_g1_jac::default(); 2 * self.batch];
        check(unsafe {
            uzk_prove_round5(self.handle, r_scalars.as_ptr() as *const u64, r_scalars.len(), alpha_zeta.as_ptr() as *const u64, alpha_zeta_omega.as_ptr() as *const u64,
                             out.as_mut_ptr())
        })?;
        Ok(out)
    }
    pub fn batch(&self) -> usize { self.batch }
}
impl Drop for Prover {
    fn drop(&mut self) {
        unsafe { uzk_prover_destroy(self.handle) };
    }
}

// ---- the point codec: ark-serialize's compressed points, decoded and encoded on the device ------------------------------------------
/// `uzk_*_decompress_batch` / `uzk_*_compress_batch`: encodings back to back (G1 32 bytes, G2 64, Baby Jubjub 32), points in the wire
/// forms, one status byte per point -- 0 accepted, 1 not a canonical encoding, 2 no point, 3 outside the prime-order subgroup (only
/// when asked).  A point whose status is not 0, and an accepted infinity, is all zeros.
pub mod codec {
    use super::*;

    fn count(bytes: usize, width: usize) -> Result<usize, Error> {
        if bytes == 0 || bytes % width != 0 || bytes / width > UZK_CODEC_MAX_BATCH as usize {
            return Err(Error::Parameter);
        }
        Ok(bytes / width)
    }
    pub fn g1_decompress(enc: &[u8]) -> Result<(Vec<uzk_g1_affine>, Vec<u8>), Error> {
        let n = count(enc.len(), 32)?;
        let (mut out, mut status) = (vec![uzk_g1_affine::default(); n], vec![0u8; n]);
        check(unsafe { uzk_g1_decompress_batch(enc.as_ptr(), n, out.as_mut_ptr(), status.as_mut_ptr()) })?;
        Ok((out, status))
    }
    pub fn g2_decompress(enc: &[u8], check_subgroup: bool) -> Result<(Vec<uzk_g2_affine>, Vec<u8>), Error> {
        let n = count(enc.len(), 64)?;
        let (mut out, mut status) = (vec![uzk_g2_affine::default(); n], vec![0u8; n]);
        check(unsafe { uzk_g2_decompress_batch(enc.as_ptr(), n, check_subgroup as c_int, out.as_mut_ptr(), status.as_mut_ptr()) })?;
        Ok((out, status))
    }
    pub fn ed_decompress(enc: &[u8], check_subgroup: bool) -> Result<(Vec<EdPoint>, Vec<u8>), Error> {
        let n = count(enc.len(), 32)?;
        let (mut out, mut status) = (vec![[[0u64; 4]; 2]; n], vec![0u8; n]);
        check(unsafe { uzk_ed_decompress_batch(enc.as_ptr(), n, check_subgroup as c_int, out.as_mut_ptr() as *mut u64, status.as_mut_ptr()) })?;
        Ok((out, status))
    }
    pub fn g1_compress(points: &[uzk_g1_affine]) -> Result<(Vec<u8>, Vec<u8>), Error> {
        let n = count(points.len() * 32, 32)?;
        let (mut out, mut status) = (vec![0u8; 32 * n], vec![0u8; n]);
        check(unsafe { uzk_g1_compress_batch(points.as_ptr(), n, out.as_mut_ptr(), status.as_mut_ptr()) })?;
        Ok((out, status))
    }
    pub fn g2_compress(points: &[uzk_g2_affine]) -> Result<(Vec<u8>, Vec<u8>), Error> {
        let n = count(points.len() * 64, 64)?;
        let (mut out, mut status) = (vec![0u8; 64 * n], vec![0u8; n]);
        check(unsafe { uzk_g2_compress_batch(points.as_ptr(), n, out.as_mut_ptr(), status.as_mut_ptr()) })?;
        Ok((out, status))
    }
    pub fn ed_compress(points: &[EdPoint]) -> Result<(Vec<u8>, Vec<u8>), Error> {
        let n = count(points.len() * 32, 32)?;
        let (mut out, mut status) = (vec![0u8; 32 * n], vec![0u8; n]);
        check(unsafe { uzk_ed_compress_batch(points.as_ptr() as *const u64, n, out.as_mut_ptr(), status.as_mut_ptr()) })?;
        Ok((out, status))
    }
    /// Host only: where the sections of a compressed Groth16 proving key lie (`uzk_g16_pk_layout`).
    pub fn g16_pk_layout(pk: &[u8]) -> Result<uzk_g16_pk_sections, Error> {
        let mut out = uzk_g16_pk_sections::default();
        check(unsafe { uzk_g16_pk_layout(pk.as_ptr(), pk.len(), &mut out) })?;
        Ok(out)
    }
}
