//! shuffle/src/gpu_anemoi.rs -- Anemoi-Jive on the device (cargo feature `gpu`): batches of hashes, the stream cipher with its trace,
//! and the zk-friendly reveals of a deck.
//!
//! `AnemoiJive254::eval_variable_length_hash` and `eval_stream_cipher_with_trace` (uzkge/src/anemoi/mod.rs) run one input at a time:
//! 28 fifth roots of 254 bits per permutation.  `gpu_hash_batch` hands a batch of equally long inputs to `uzk_anemoi_hash_batch` (a
//! lobby's seed commitments, matchmaking/src/test.rs), `gpu_stream_cipher_with_trace` returns the `AnemoiStreamCipherTrace` of every
//! input through `uzk_anemoi_stream_batch` (zmatchmaking's witness: 49 outputs of a 2-element input, matchmaking/src/build_cs.rs),
//! `gpu_reveal_cards0` / `gpu_verify_reveals0` are `gpu_reveal_cards` / `gpu_verify_reveals_cp` (gpu_reveal.rs) for `reveal0` /
//! `verify_reveal0`: `uzk_cp_reveal_prove0_batch` / `uzk_cp_reveal_verify0_batch`.
//!
//! All of them return `None` when the device cannot serve the call (no GPU, a HIP failure, unequal lengths): the caller then runs the
//! reference's loop as before.  Nothing here panics on a device error.
//!
//! Layout: an element of `ark_bn254::Fr` goes over as its Montgomery limbs.  A trace block is 64 elements per permutation: before
//! (x0 x1 y0 y1), the state after each of the 14 rounds' S-boxes, after (include/uzkge_gpu.h).
use ark_bn254::Fr;
use ark_ec::CurveGroup;
use ark_ed_on_bn254::{EdwardsAffine, EdwardsProjective, Fq, Fr as EdFr};
use ark_ff::{BigInt, PrimeField, UniformRand};
use ark_std::rand::{CryptoRng, RngCore};
use uzkge::{
    anemoi::{AnemoiStreamCipherTrace, N_ANEMOI_ROUNDS},
    chaum_pedersen::dl::ChaumPedersenDLProof,
};
use uzkge_gpu_sys as sys;

use crate::{keygen::{Keypair, PublicKey}, MaskedCard, RevealCard};

fn elem_to_wire(v: &Fr) -> sys::Limbs {
    (v.0).0
}
fn elem_from_wire(w: &sys::Limbs) -> Fr {
    Fr::new_unchecked(BigInt(*w))
}
fn point_to_wire(p: &EdwardsProjective) -> sys::EdPoint {
    let a = p.into_affine();                       // the identity is (0, 1) on the wire; the library encodes it for the hash
    [(a.x.0).0, (a.y.0).0]
}
fn point_from_wire(w: &sys::EdPoint) -> EdwardsProjective {
    EdwardsAffine::new_unchecked(Fq::new_unchecked(BigInt(w[0])), Fq::new_unchecked(BigInt(w[1]))).into()
}
fn scalar_to_wire(s: &EdFr) -> [u64; 4] {
    s.into_bigint().0
}
/// the inputs of a batch, flattened; `None` when they are not equally long or there are none
fn flatten(inputs: &[Vec<Fr>]) -> Option<(Vec<sys::Limbs>, usize)> {
    let len = inputs.first()?.len();
    if inputs.len() > sys::UZK_ANEMOI_MAX_BATCH as usize || len > sys::UZK_ANEMOI_MAX_INPUT as usize || inputs.iter().any(|v| v.len() != len) {
        return None;
    }
    Some((inputs.iter().flat_map(|v| v.iter().map(elem_to_wire)).collect(), len))
}

/// `eval_variable_length_hash` of every input; the inputs of a call are equally long.
pub fn gpu_hash_batch(inputs: &[Vec<Fr>]) -> Option<Vec<Fr>> {
    if inputs.is_empty() {
        return Some(Vec::new());
    }
    let (wire, len) = flatten(inputs)?;
    let (out, _) = sys::anemoi_hash_batch(&wire, len, inputs.len(), false).ok()?;
    Some(out.iter().map(elem_from_wire).collect())
}

/// `eval_stream_cipher_with_trace(input, output_len)` of every input, in input order.
pub fn gpu_stream_cipher_with_trace(inputs: &[Vec<Fr>], output_len: usize) -> Option<Vec<AnemoiStreamCipherTrace<Fr, 2, N_ANEMOI_ROUNDS>>> {
    if inputs.is_empty() {
        return Some(Vec::new());
    }
    if output_len == 0 || output_len > sys::UZK_ANEMOI_MAX_OUTPUT as usize {
        return None;
    }
    let (wire, len) = flatten(inputs)?;
    let (out, blocks) = sys::anemoi_stream_batch(&wire, len, inputs.len(), output_len, true).ok()?;
    let blocks = blocks?;
    let perms = sys::anemoi_permutations(len, output_len);
    let pair = |b: &sys::AnemoiTraceBlock, at: usize| ([elem_from_wire(&b[at]), elem_from_wire(&b[at + 1])], [elem_from_wire(&b[at + 2]), elem_from_wire(&b[at + 3])]);
    let mut traces = Vec::with_capacity(inputs.len());
    for (i, input) in inputs.iter().enumerate() {
        let mut trace = AnemoiStreamCipherTrace::<Fr, 2, N_ANEMOI_ROUNDS>::default();
        trace.input = input.clone();
        for b in blocks.get(i * perms..(i + 1) * perms)? {
            trace.before_permutation.push(pair(b, 0));
            let mut mid = ([[Fr::from(0u64); 2]; N_ANEMOI_ROUNDS], [[Fr::from(0u64); 2]; N_ANEMOI_ROUNDS]);
            for r in 0..N_ANEMOI_ROUNDS {
                let (x, y) = pair(b, 4 + 4 * r);
                mid.0[r] = x;
                mid.1[r] = y;
            }
            trace.intermediate_values_before_constant_additions.push(mid);
            trace.after_permutation.push(pair(b, 60));
        }
        trace.output = out.get(i * output_len..(i + 1) * output_len)?.iter().map(elem_from_wire).collect();
        traces.push(trace);
    }
    Some(traces)
}

/// `reveal0` for every card of `masked_cards` under one keypair: the reveal cards and their proofs, in card order.  One omega per card
/// is drawn from `prng`, as `prove0` draws it.
pub fn gpu_reveal_cards0<R: CryptoRng + RngCore>(prng: &mut R, keypair: &Keypair, masked_cards: &[MaskedCard]) -> Option<Vec<(RevealCard, ChaumPedersenDLProof)>> {
    if masked_cards.is_empty() {
        return Some(Vec::new());
    }
    if masked_cards.len() > sys::UZK_CP_MAX_BATCH as usize {
        return None;
    }
    let e1: Vec<sys::EdPoint> = masked_cards.iter().map(|c| point_to_wire(&c.e1)).collect();
    let omegas: Vec<[u64; 4]> = masked_cards.iter().map(|_| scalar_to_wire(&EdFr::rand(prng))).collect();
    let (reveals, pk, proofs) = sys::cp_reveal_prove0_batch(&scalar_to_wire(&keypair.secret), &e1, &omegas).ok()?;
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

/// `verify_reveal0` for every (pk, masked card, reveal card, proof) of `batch`: `Some(Ok(()))` all accepted, `Some(Err(indices))` the
/// rejected ones, `None` the device could not serve the call.
pub fn gpu_verify_reveals0(batch: &[(&PublicKey, &MaskedCard, &RevealCard, &ChaumPedersenDLProof)]) -> Option<Result<(), Vec<usize>>> {
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
    let verdict = sys::cp_reveal_verify0_batch(&statements, &proofs).ok()?;
    let bad: Vec<usize> = verdict.iter().enumerate().filter(|(_, v)| **v != 0).map(|(i, _)| i).collect();
    if bad.is_empty() {
        Some(Ok(()))
    } else {
        Some(Err(bad))
    }
}
