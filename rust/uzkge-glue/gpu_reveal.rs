//! shuffle/src/gpu_reveal.rs -- the plain reveal path of a deck on the device (cargo feature `gpu`).
//!
//! `reveal` and `verify_reveal` (shuffle/src/reveal.rs over uzkge/src/chaum_pedersen/dl.rs) handle one card: four scalar
//! multiplications on Baby Jubjub and a Keccak transcript each, 52 times per player per deck.  `gpu_reveal_cards` and
//! `gpu_verify_reveals_cp` hand a whole deck to `uzk_cp_reveal_prove_batch` / `uzk_cp_reveal_verify_batch` (include/uzkge_gpu.h): one
//! lane per multiplication, per equation for the verifier.  What stays here is what only this side has: the omegas (drawn from the
//! caller's rng, one per card, in card order -- the draws `prove` makes) and the conversions.
//!
//! Both return `None` when the device cannot serve the call (no GPU, a HIP failure): the caller then runs the reference's loop as
//! before.  Nothing here panics on a device error.  A single proof stays with the reference: a call costs one doubling chain
//! whatever the batch, which one card does not repay.
//!
//! Layout: `ark_ed_on_bn254::Fq` is `ark_bn254::Fr` -- a coordinate's Montgomery limbs are the wire words; `ark_ed_on_bn254::Fr`
//! (the scalars, order L) goes over as the plain integer `into_bigint()`.
use ark_ec::CurveGroup;
use ark_ed_on_bn254::{EdwardsAffine, EdwardsProjective, Fq, Fr};
use ark_ff::{BigInt, PrimeField, UniformRand};
use ark_std::rand::{CryptoRng, RngCore};
use uzkge::chaum_pedersen::dl::ChaumPedersenDLProof;
use uzkge_gpu_sys as sys;

use crate::{keygen::{Keypair, PublicKey}, MaskedCard, RevealCard};

fn point_to_wire(p: &EdwardsProjective) -> sys::EdPoint {
    let a = p.into_affine();                       // the identity is (0, 1): an ordinary affine point of a twisted Edwards curve
    [(a.x.0).0, (a.y.0).0]
}
fn point_from_wire(w: &sys::EdPoint) -> EdwardsProjective {
    EdwardsAffine::new_unchecked(Fq::new_unchecked(BigInt(w[0])), Fq::new_unchecked(BigInt(w[1]))).into()
}
fn scalar_to_wire(s: &Fr) -> [u64; 4] {
    s.into_bigint().0
}

/// `reveal` for every card of `masked_cards` under one keypair: the reveal cards and their proofs, in card order.
pub fn gpu_reveal_cards<R: CryptoRng + RngCore>(prng: &mut R, keypair: &Keypair, masked_cards: &[MaskedCard]) -> Option<Vec<(RevealCard, ChaumPedersenDLProof)>> {
    if masked_cards.is_empty() {
        return Some(Vec::new());
    }
    if masked_cards.len() > sys::UZK_CP_MAX_BATCH as usize {
        return None;
    }
    let e1: Vec<sys::EdPoint> = masked_cards.iter().map(|c| point_to_wire(&c.e1)).collect();
    let omegas: Vec<[u64; 4]> = masked_cards.iter().map(|_| scalar_to_wire(&Fr::rand(prng))).collect();
    let (reveals, pk, proofs) = sys::cp_reveal_prove_batch(&scalar_to_wire(&keypair.secret), &e1, &omegas).ok()?;
    if point_from_wire(&pk) != keypair.public {
        return None;                               // the keypair is not (sk, sk G): the reference asserts; here the caller's loop decides
    }
    let blob = sys::UZK_CP_PROOF_BYTES as usize;
    let mut out = Vec::with_capacity(masked_cards.len());
    for (reveal, bytes) in reveals.iter().zip(proofs.chunks_exact(blob)) {
        out.push((point_from_wire(reveal), ChaumPedersenDLProof::from_uncompress(bytes).ok()?));
    }
    Some(out)
}

/// `verify_reveal` for every (pk, masked card, reveal card, proof) of `batch`.
///   Some(Ok(()))        every proof is accepted
///   Some(Err(indices))  the rejected ones (a verdict of 1 .. 5)
///   None                the device could not serve the call: nothing was decided
pub fn gpu_verify_reveals_cp(batch: &[(&PublicKey, &MaskedCard, &RevealCard, &ChaumPedersenDLProof)]) -> Option<Result<(), Vec<usize>>> {
    if batch.is_empty() {
        return Some(Ok(()));
    }
    if batch.len() > sys::UZK_CP_MAX_BATCH as usize {
        return None;
    }
    let mut statements: Vec<sys::RevealStatement> = Vec::with_capacity(batch.len());
    let mut proofs: Vec<u8> = Vec::with_capacity(batch.len() * sys::UZK_CP_PROOF_BYTES as usize);
    for (pk, masked, reveal, proof) in batch {
        statements.push([point_to_wire(&masked.e1), point_to_wire(reveal), point_to_wire(pk)]);
        proofs.extend(proof.to_uncompress());
    }
    let verdict = sys::cp_reveal_verify_batch(&statements, &proofs).ok()?;
    let bad: Vec<usize> = verdict.iter().enumerate().filter(|(_, v)| **v != 0).map(|(i, _)| i).collect();
    if bad.is_empty() {
        Some(Ok(()))
    } else {
        Some(Err(bad))
    }
}
