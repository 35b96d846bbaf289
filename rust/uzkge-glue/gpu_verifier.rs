//! uzkge/src/plonk/gpu_verifier.rs -- a BATCH of proofs under one verifier key checked with one pairing (cargo feature `gpu`).
//!
//! `verifier` (verifier.rs:17-164) ends in `Bn254::multi_pairing([left, -right], [[tau] G2, G2]) == 1` with `left` and `right` sums
//! of (commitment, scalar) products (`batch_verify_diff_points`, kzg_poly_commitment.rs:373-422).  With one random weight per proof
//! the m equations of a batch collapse into ONE; `uzk_verify_fold` (include/uzkge_gpu.h) computes its two G1 points on the device --
//! the m Keccak transcripts, the verifier scalars, two MSMs -- and what stays here is what only this side has: the weights
//! (drawn AFTER the proofs are known, from the caller's rng), the two G2 elements and the pairing, and the reference verifier
//! as the way to NAME the wrong proofs of a rejected batch.
//!
//! `verify_batch` returns `None` when the device cannot serve the call (no GPU, a HIP failure, a key it cannot hold): the caller
//! verifies proof by proof as before.  Nothing here panics on a device error.
use std::collections::HashMap;
use std::sync::{Arc, Mutex};

use ark_bn254::{Bn254, Fq, Fr, G1Affine, G1Projective, G2Affine};
use ark_ec::{pairing::Pairing, CurveGroup};
use ark_ff::{BigInteger, One, PrimeField, UniformRand};
use ark_std::rand::{CryptoRng, RngCore};
use lazy_static::lazy_static;
use uzkge_gpu_sys as sys;

use super::{
    constraint_system::ConstraintSystem,
    indexer::{PlonkProof, PlonkVerifierParams},
    verifier::verifier,
};
use crate::{
    gpu::{affine_to_wire, fr_limbs, g1_affine_from_wire, g2_affine_from_wire, g2_affine_to_wire, jac_from_wire},
    poly_commit::{field_polynomial::FpPolynomial, kzg_poly_commitment::{KZGCommitment, KZGCommitmentSchemeBN254}, pcs::ToBytes},
    utils::transcript::Transcript,
};

type Limbs = [u64; 4];
type Pcs = KZGCommitmentSchemeBN254;

lazy_static! {
    /// Resident keys by what identifies them: the key's commitments, cs_size and the transcript prefix -- never an address.
    /// The public-key commitments are not part of the identity: they change once per game and are replaced in place.
    static ref KEYS: Mutex<HashMap<Vec<u8>, Arc<Mutex<(sys::VerifierKey, Vec<u8>)>>>> = Mutex::new(HashMap::new());
}

fn wire(cms: &[KZGCommitment<G1Projective>]) -> Vec<sys::uzk_g1_affine> {
    let points: Vec<G1Projective> = cms.iter().map(|c| c.0).collect();
    G1Projective::normalize_batch(&points).iter().map(affine_to_wire).collect()
}
fn fill(dst: &mut [sys::uzk_g1_affine], src: &[sys::uzk_g1_affine]) -> Option<()> {
    if dst.len() != src.len() {
        return None;
    }
    dst.copy_from_slice(src);
    Some(())
}
fn identity_of(vp: &PlonkVerifierParams<Pcs>, prefix: &[u8]) -> Vec<u8> {
    let mut key: Vec<u8> = vp.cm_q_vec.iter().chain(vp.cm_s_vec.iter()).chain(vp.cm_prk_vec.iter()).flat_map(|c| c.to_bytes()).collect();
    key.extend(vp.cm_qb.to_bytes());
    #[cfg(feature = "shuffle")]
    {
        key.extend(vp.cm_q_ecc.to_bytes());
        key.extend(vp.cm_shuffle_generator_vec.iter().flat_map(|c| c.to_bytes()));
    }
    key.extend((vp.cs_size as u64).to_le_bytes());
    key.extend(prefix);
    key
}
fn public_key_of(_vp: &PlonkVerifierParams<Pcs>) -> Vec<u8> {
    #[cfg(feature = "shuffle")]
    let key = _vp.cm_shuffle_public_key_vec.iter().flat_map(|c| c.to_bytes()).collect();
    #[cfg(not(feature = "shuffle"))]
    let key = Vec::new();
    key
}

/// The key of `vp` on the device, made on first use.
fn resident(pcs: &Pcs, vp: &PlonkVerifierParams<Pcs>, prefix: &[u8]) -> Option<Arc<Mutex<(sys::VerifierKey, Vec<u8>)>>> {
    let id = identity_of(vp, prefix);
    if let Some(k) = KEYS.lock().ok()?.get(&id) {
        return Some(k.clone());
    }
    let domain = FpPolynomial::<Fr>::evaluation_domain(vp.cs_size)?;
    let root: Fr = domain.group_gen;
    let n_pi = vp.public_vars_constraint_indices.len();
    if vp.lagrange_constants.len() != n_pi || vp.k.len() != 5 {
        return None;
    }
    let root_powers: Vec<Limbs> = vp.public_vars_constraint_indices.iter().map(|i| fr_limbs(&ark_ff::Field::pow(&root, [*i as u64]))).collect();
    let lagrange: Vec<Limbs> = vp.lagrange_constants.iter().map(fr_limbs).collect();
    let zero = sys::uzk_g1_affine::default();
    let mut d = sys::uzk_vk_desc {
        cs_size: vp.cs_size as u32,
        n_pi: n_pi as u32,
        shuffle: cfg!(feature = "shuffle") as u32,
        transcript_prefix_len: prefix.len() as u32,
        transcript_prefix: prefix.as_ptr(),
        pi_root_powers: root_powers.as_ptr() as *const u64,
        pi_lagrange: lagrange.as_ptr() as *const u64,
        cm_q: [zero; 9],
        cm_s: [zero; 5],
        cm_qb: zero,
        cm_prk: [zero; 4],
        cm_q_ecc: zero,
        cm_shuffle_public_key: [zero; 12],
        cm_shuffle_generator: [zero; 12],
        g1_0: zero,
        k: [[0u64; 4]; 5],
        anemoi_g: fr_limbs(&vp.anemoi_generator),
        anemoi_g_inv: fr_limbs(&vp.anemoi_generator_inv),
        edwards_a: [0u64; 4],
        root: fr_limbs(&root),
    };
    fill(&mut d.cm_q, &wire(&vp.cm_q_vec))?;
    fill(&mut d.cm_s, &wire(&vp.cm_s_vec))?;
    fill(&mut d.cm_prk, &wire(&vp.cm_prk_vec))?;
    d.cm_qb = *wire(std::slice::from_ref(&vp.cm_qb)).first()?;
    d.g1_0 = affine_to_wire(&pcs.public_parameter_group_1.first()?.into_affine());
    #[cfg(feature = "shuffle")]
    {
        d.edwards_a = fr_limbs(&vp.edwards_a);
        d.cm_q_ecc = *wire(std::slice::from_ref(&vp.cm_q_ecc)).first()?;
        fill(&mut d.cm_shuffle_public_key, &wire(&vp.cm_shuffle_public_key_vec))?;
        fill(&mut d.cm_shuffle_generator, &wire(&vp.cm_shuffle_generator_vec))?;
    }
    for (dst, k) in d.k.iter_mut().zip(vp.k.iter()) {
        *dst = fr_limbs(k);
    }
    let key = sys::VerifierKey::create(&d).ok()?;
    let entry = Arc::new(Mutex::new((key, public_key_of(vp))));
    KEYS.lock().ok()?.insert(id, entry.clone());
    Some(entry)
}

/// Forgets every resident verifier key (their device memory is freed).
pub fn release_verifier_keys() {
    if let Ok(mut keys) = KEYS.lock() {
        keys.clear();
    }
}

/// Verifies `batch` = [(public inputs, proof)] under `params` with ONE pairing.  `prefix`: the bytes the caller's transcript holds
/// in front of `transcript_init_plonk` (for `verify_shuffle`: the padded label and `n_cards` as a 32-byte word); `new_transcript`
/// makes that transcript for the reference verifier.
///   Some(Ok(()))        every proof is accepted
///   Some(Err(indices))  the batch was rejected: the proofs the reference verifier refuses, one by one (or the malformed ones)
///   None                the device could not serve the call: nothing was decided
pub fn verify_batch<R: CryptoRng + RngCore, CS: ConstraintSystem<Fr>>(
    prng: &mut R,
    new_transcript: impl Fn() -> Transcript,
    prefix: &[u8],
    pcs: &Pcs,
    cs: &CS,
    params: &PlonkVerifierParams<Pcs>,
    batch: &[(&[Fr], &PlonkProof<Pcs>)],
) -> Option<Result<(), Vec<usize>>> {
    if batch.is_empty() {
        return Some(Ok(()));
    }
    if batch.len() > sys::UZK_VERIFY_MAX_BATCH as usize || pcs.public_parameter_group_2.len() < 2 {
        return None;
    }
    let entry = resident(pcs, params, prefix)?;
    let mut guard = entry.lock().ok()?;
    #[cfg(feature = "shuffle")]
    {
        let public_key = public_key_of(params);
        if guard.1 != public_key {
            let pk = wire(&params.cm_shuffle_public_key_vec);
            let mut twelve = [sys::uzk_g1_affine::default(); 12];
            fill(&mut twelve, &pk)?;
            guard.0.set_public_key(&twelve).ok()?;
            guard.1 = public_key;
        }
    }
    let key = &guard.0;
    let mut proofs = Vec::with_capacity(batch.len() * key.proof_bytes());
    let mut pi = Vec::with_capacity(batch.len() * key.n_pi());
    for (inputs, proof) in batch {
        if inputs.len() != key.n_pi() {
            return None;
        }
        proofs.extend(proof.to_bytes_be());
        pi.extend(inputs.iter().map(fr_limbs));
    }
    // the weights: uniform, drawn now -- after every proof of the batch is fixed.  One proof needs none.
    let weights: Vec<Limbs> = if batch.len() == 1 { vec![fr_limbs(&Fr::one())] } else { (0..batch.len()).map(|_| fr_limbs(&Fr::rand(prng))).collect() };
    let (left, right, status) = key.fold(&proofs, &pi, Some(&weights)).ok()?;
    drop(guard);
    let malformed: Vec<usize> = status.iter().enumerate().filter(|(_, s)| **s != 0).map(|(i, _)| i).collect();
    if !malformed.is_empty() {
        return Some(Err(malformed));
    }
    let (left, right) = (jac_from_wire(&left), jac_from_wire(&right));
    let g2_0 = pcs.public_parameter_group_2[0];
    let g2_1 = pcs.public_parameter_group_2[1];
    let verdict = Bn254::multi_pairing(&[left, -right], &[g2_1, g2_0]).0;
    if verdict == <Bn254 as Pairing>::TargetField::one() {
        return Some(Ok(()));
    }
    // rejected: the reference verifier names the wrong ones
    let mut bad = Vec::new();
    for (i, (inputs, proof)) in batch.iter().enumerate() {
        let mut transcript = new_transcript();
        if verifier(&mut transcript, pcs, cs, params, inputs, proof).is_err() {
            bad.push(i);
        }
    }
    Some(Err(bad))
}

// ---- Groth16 reveal proofs: M proofs under one verifying key, M + 3 Miller loops, one final exponentiation ----------------------

/// A Groth16 verifying key as the fold needs it (ark-groth16's `VerifyingKey<Bn254>`, field by field).
pub struct RevealVerifyingKey<'a> {
    pub alpha_g1: &'a G1Affine,
    pub beta_g2: &'a G2Affine,
    pub gamma_g2: &'a G2Affine,
    pub delta_g2: &'a G2Affine,
    pub gamma_abc_g1: &'a [G1Affine],
}

fn word(out: &mut Vec<u8>, c: &Fq) {
    out.extend(c.into_bigint().to_bytes_be());
}
/// The 256-byte blob of a proof: a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0, c.x, c.y as 32-byte big-endian words (the order in
/// which shuffle/src/sdk.rs:306-319 emits them for the contract); the point at infinity is zeros.
pub fn reveal_proof_bytes(a: &G1Affine, b: &G2Affine, c: &G1Affine) -> Vec<u8> {
    let mut out = Vec::with_capacity(sys::UZK_G16_PROOF_BYTES as usize);
    let zero = Fq::from(0u64);
    let g1 = |out: &mut Vec<u8>, p: &G1Affine| {
        if p.infinity { word(out, &zero); word(out, &zero); } else { word(out, &p.x); word(out, &p.y); }
    };
    g1(&mut out, a);
    if b.infinity {
        for _ in 0..4 { word(&mut out, &zero); }
    } else {
        word(&mut out, &b.x.c1); word(&mut out, &b.x.c0); word(&mut out, &b.y.c1); word(&mut out, &b.y.c0);
    }
    g1(&mut out, c);
    out
}

/// What both reveal verifiers need: the key on the device, the three G2 points in wire form, the proofs' blobs, the public inputs and
/// the weights (drawn here, after every proof of the batch is fixed).  None: the batch does not fit the entry point, or no device.
struct RevealBatch {
    key: sys::Groth16Vk,
    g2: [sys::uzk_g2_affine; 3],
    proofs: Vec<u8>,
    public: Vec<Limbs>,
    weights: Vec<Limbs>,
}
fn prepare_reveals<R: CryptoRng + RngCore>(prng: &mut R, vk: &RevealVerifyingKey, batch: &[(&[Fr], (G1Affine, G2Affine, G1Affine))]) -> Option<RevealBatch> {
    let l = vk.gamma_abc_g1.len();
    if batch.len() > sys::UZK_G16_VERIFY_MAX_BATCH as usize || l == 0 || l > sys::UZK_G16_VERIFY_MAX_INPUTS as usize {
        return None;
    }
    let ic: Vec<sys::uzk_g1_affine> = vk.gamma_abc_g1.iter().map(affine_to_wire).collect();
    let g2 = [g2_affine_to_wire(vk.beta_g2), g2_affine_to_wire(vk.gamma_g2), g2_affine_to_wire(vk.delta_g2)];
    let desc = sys::uzk_g16_vk_desc {
        n_inputs: l as u32,
        reserved: 0,
        alpha_g1: affine_to_wire(vk.alpha_g1),
        beta_g2: g2[0],
        gamma_g2: g2[1],
        delta_g2: g2[2],
        gamma_abc_g1: ic.as_ptr(),
    };
    let key = sys::Groth16Vk::create(&desc).ok()?;
    let mut proofs = Vec::with_capacity(batch.len() * sys::UZK_G16_PROOF_BYTES as usize);
    let mut public: Vec<Limbs> = Vec::with_capacity(batch.len() * (l - 1));
    for (inputs, (a, b, c)) in batch {
        if inputs.len() != l - 1 {
            return None;
        }
        proofs.extend(reveal_proof_bytes(a, b, c));
        public.extend(inputs.iter().map(fr_limbs));
    }
    let weights: Vec<Limbs> = if batch.len() == 1 { vec![fr_limbs(&Fr::one())] } else { (0..batch.len()).map(|_| fr_limbs(&Fr::rand(prng))).collect() };
    Some(RevealBatch { key, g2, proofs, public, weights })
}

/// Checks `batch` = [(public inputs without the leading one, (A, B, C))] under `vk` with ONE product of pairings: the weights are
/// drawn here, after every proof of the batch is fixed; `uzk_g16_verify_fold` decodes and checks the points (B's subgroup included),
/// computes rho_i A_i and the three sums on the device; the M + 3 Miller loops and the final exponentiation are arkworks'.
///   Some(Ok(()))        every proof is accepted
///   Some(Err(indices))  malformed proofs (a nonzero status), or -- an empty list -- a well-formed batch whose product is not one:
///                       the caller then checks proof by proof to name the wrong ones
///   None                the device could not serve the call: nothing was decided
pub fn fold_reveals<R: CryptoRng + RngCore>(prng: &mut R, vk: &RevealVerifyingKey, batch: &[(&[Fr], (G1Affine, G2Affine, G1Affine))]) -> Option<Result<(), Vec<usize>>> {
    if batch.is_empty() {
        return Some(Ok(()));
    }
    let r = prepare_reveals(prng, vk, batch)?;
    let fold = r.key.fold(&r.proofs, &r.public, Some(&r.weights)).ok()?;
    let malformed: Vec<usize> = fold.status.iter().enumerate().filter(|(_, s)| **s != 0).map(|(i, _)| i).collect();
    if !malformed.is_empty() {
        return Some(Err(malformed));
    }
    let mut g1: Vec<G1Affine> = fold.a.iter().map(g1_affine_from_wire).collect();
    let mut g2: Vec<G2Affine> = fold.b.iter().map(g2_affine_from_wire).collect();
    for (sum, q) in [(&fold.alpha, vk.beta_g2), (&fold.x, vk.gamma_g2), (&fold.c, vk.delta_g2)] {
        g1.push((-jac_from_wire(sum)).into_affine());
        g2.push(*q);
    }
    if Bn254::multi_pairing(g1, g2).0 == <Bn254 as Pairing>::TargetField::one() {
        Some(Ok(()))
    } else {
        Some(Err(Vec::new()))
    }
}

/// `fold_reveals` to the end on the device: `uzk_g16_verify_batch` folds the batch and runs the product of its M + 3 pairings there
/// (rho_i A_i and B_i never visit the host), so no arkworks pairing is needed.  Same answers as `fold_reveals`.
pub fn verify_reveals<R: CryptoRng + RngCore>(prng: &mut R, vk: &RevealVerifyingKey, batch: &[(&[Fr], (G1Affine, G2Affine, G1Affine))]) -> Option<Result<(), Vec<usize>>> {
    if batch.is_empty() {
        return Some(Ok(()));
    }
    let r = prepare_reveals(prng, vk, batch)?;
    let (accepted, status) = r.key.verify_batch(&r.proofs, &r.public, Some(&r.weights), &r.g2).ok()?;
    let malformed: Vec<usize> = status.iter().enumerate().filter(|(_, s)| **s != 0).map(|(i, _)| i).collect();
    if !malformed.is_empty() {
        return Some(Err(malformed));
    }
    if accepted {
        Some(Ok(()))
    } else {
        Some(Err(Vec::new()))
    }
}
