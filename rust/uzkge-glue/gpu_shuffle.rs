//! shuffle/src/gpu_shuffle.rs -- masking a deck and the remask of a shuffle on the device (cargo feature `gpu`).
//!
//! `mask` / `verify_mask` (shuffle/src/mask.rs over uzkge/src/chaum_pedersen/dl.rs) handle one card: four scalar multiplications on
//! Baby Jubjub and a Keccak transcript each.  `eval_remark_with_trace` (uzkge/src/shuffle/remark.rs, called per card from
//! shuffle/src/build_cs.rs) rebuilds both tables -- 84 x 4 multiples of G and of the joint key -- for every card and converts to affine
//! 168 times per card.  `gpu_mask_cards`, `gpu_verify_masks` and `gpu_remark_deck` hand a whole deck to `uzk_cp_mask_prove_batch` /
//! `uzk_cp_mask_verify_batch` / `uzk_remark_batch` (include/uzkge_gpu.h): the tables are built once per key and stay on the device, a
//! card is two lanes of 84 additions.  What stays here is what only this side has: the draws (omegas and the remask bits from the
//! caller's rng, in card order -- the draws `prove` and `sample_random_scalar_bits` make), the permutation and the conversions.
//!
//! All three return `None` when the device cannot serve the call (no GPU, a HIP failure): the caller then runs the reference's loop
//! as before.  Nothing here panics on a device error.
//!
//! Layout: `ark_ed_on_bn254::Fq` is `ark_bn254::Fr` -- a coordinate's Montgomery limbs are the wire words; `ark_ed_on_bn254::Fr`
//! (the scalars, order L) goes over as the plain integer `into_bigint()`.  A digit is one byte per (card, iteration): bit 0 =
//! bits[0], bit 1 = bits[1], bit 2 = bits[2].
use ark_ec::CurveGroup;
use ark_ed_on_bn254::{EdwardsAffine, EdwardsProjective, Fq, Fr};
use ark_ff::{BigInt, Field, PrimeField, UniformRand};
use ark_std::rand::{CryptoRng, RngCore};
use uzkge::{
    chaum_pedersen::dl::ChaumPedersenDLProof,
    plonk::constraint_system::turbo::N_WIRE_SELECTORS,
    shuffle::{Permutation, RemarkTrace},
};
use uzkge_gpu_sys as sys;

use crate::{keygen::PublicKey, Card, MaskedCard};

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
fn digit_of(bits: &[bool; N_WIRE_SELECTORS]) -> u8 {
    (bits[0] as u8) | ((bits[1] as u8) << 1) | ((bits[2] as u8) << 2)
}

/// `mask` for every card of `cards` under the joint key with the caller's `rs` (init_masked_cards passes ones): the masked cards and
/// their proofs, in card order.  One omega per card is drawn from `prng`, as `prove` draws it.
pub fn gpu_mask_cards<R: CryptoRng + RngCore>(prng: &mut R, shared_key: &PublicKey, cards: &[Card], rs: &[Fr]) -> Option<Vec<(MaskedCard, ChaumPedersenDLProof)>> {
    if cards.is_empty() {
        return Some(Vec::new());
    }
    if cards.len() > sys::UZK_CP_MAX_BATCH as usize || rs.len() != cards.len() {
        return None;
    }
    let wire: Vec<sys::EdPoint> = cards.iter().map(point_to_wire).collect();
    let rs_wire: Vec<[u64; 4]> = rs.iter().map(scalar_to_wire).collect();
    let omegas: Vec<[u64; 4]> = cards.iter().map(|_| scalar_to_wire(&Fr::rand(prng))).collect();
    let (e1, e2, proofs) = sys::cp_mask_prove_batch(&point_to_wire(shared_key), &wire, &rs_wire, &omegas).ok()?;
    let blob = sys::UZK_CP_PROOF_BYTES as usize;
    let mut out = Vec::with_capacity(cards.len());
    for ((a, b), bytes) in e1.iter().zip(e2.iter()).zip(proofs.chunks_exact(blob)) {
        out.push((MaskedCard { e1: point_from_wire(a), e2: point_from_wire(b) }, ChaumPedersenDLProof::from_uncompress(bytes).ok()?));
    }
    Some(out)
}

/// `verify_mask` for every (card, masked card, proof) of `batch` under the joint key.
///   Some(Ok(()))        every proof is accepted
///   Some(Err(indices))  the rejected ones (a verdict of 1 .. 5)
///   None                the device could not serve the call: nothing was decided
pub fn gpu_verify_masks(shared_key: &PublicKey, batch: &[(&Card, &MaskedCard, &ChaumPedersenDLProof)]) -> Option<Result<(), Vec<usize>>> {
    if batch.is_empty() {
        return Some(Ok(()));
    }
    if batch.len() > sys::UZK_CP_MAX_BATCH as usize {
        return None;
    }
    let mut cards: Vec<sys::EdPoint> = Vec::with_capacity(batch.len());
    let mut e1: Vec<sys::EdPoint> = Vec::with_capacity(batch.len());
    let mut e2: Vec<sys::EdPoint> = Vec::with_capacity(batch.len());
    let mut proofs: Vec<u8> = Vec::with_capacity(batch.len() * sys::UZK_CP_PROOF_BYTES as usize);
    for (card, masked, proof) in batch {
        cards.push(point_to_wire(card));
        e1.push(point_to_wire(&masked.e1));
        e2.push(point_to_wire(&masked.e2));
        proofs.extend(proof.to_uncompress());
    }
    let verdict = sys::cp_mask_verify_batch(&point_to_wire(shared_key), &cards, &e1, &e2, &proofs).ok()?;
    let bad: Vec<usize> = verdict.iter().enumerate().filter(|(_, v)| **v != 0).map(|(i, _)| i).collect();
    if bad.is_empty() {
        Some(Ok(()))
    } else {
        Some(Err(bad))
    }
}

/// The remask of a whole deck for `build_cs`: the trace of every input card (what `eval_remark_with_trace` returns per card, in
/// input order) and the new deck, `out[i] = remasked[perm[i]]` with `perm[i]` the column of row i's one in `permutation`.
/// `bits[k]` are card k's 84 draws of `sample_random_scalar_bits`; `key` holds the tables of the joint key for the length of the game.
pub fn gpu_remark_deck(
    key: &sys::RemarkKey,
    deck: &[MaskedCard],
    bits: &[Vec<[bool; N_WIRE_SELECTORS]>],
    permutation: &Permutation<Fq>,
) -> Option<(Vec<RemarkTrace<Fq>>, Vec<MaskedCard>)> {
    let n = deck.len();
    let iters = sys::UZK_REMARK_ITERATIONS as usize;
    if n == 0 {
        return Some((Vec::new(), Vec::new()));
    }
    if n > sys::UZK_ED_MAX_BATCH as usize || bits.len() != n || bits.iter().any(|b| b.len() != iters) {
        return None;
    }
    let matrix = permutation.get_matrix();
    if matrix.len() != n {
        return None;
    }
    let mut perm: Vec<u32> = Vec::with_capacity(n);
    for row in matrix.iter() {
        perm.push(row.iter().position(|v| *v == Fq::ONE)? as u32);
    }
    let e1: Vec<sys::EdPoint> = deck.iter().map(|c| point_to_wire(&c.e1)).collect();
    let e2: Vec<sys::EdPoint> = deck.iter().map(|c| point_to_wire(&c.e2)).collect();
    let digits: Vec<u8> = bits.iter().flat_map(|card| card.iter().map(digit_of)).collect();
    let (o1, o2, trace) = key.remark_batch(&e1, &e2, &digits, Some(&perm), true).ok()?;
    let trace = trace?;
    let (zero, one) = (Fq::ZERO, Fq::ONE);
    let field = |w: &[u64; 4]| Fq::new_unchecked(BigInt(*w));
    let mut traces = Vec::with_capacity(n);
    for (k, card_bits) in bits.iter().enumerate() {
        let values: Vec<[Fq; 4]> = trace[k * iters..(k + 1) * iters].iter().map(|t| [field(&t[0]), field(&t[1]), field(&t[2]), field(&t[3])]).collect();
        let field_bits: Vec<[Fq; N_WIRE_SELECTORS]> = card_bits
            .iter()
            .map(|b| [if b[0] { one } else { zero }, if b[1] { one } else { zero }, if b[2] { one } else { -one }])
            .collect();
        let output = *values.last()?;
        traces.push(RemarkTrace { bits: field_bits, intermediate_values: values, output, n_round: iters });
    }
    let new_deck = o1.iter().zip(o2.iter()).map(|(a, b)| MaskedCard { e1: point_from_wire(a), e2: point_from_wire(b) }).collect();
    Some((traces, new_deck))
}

/// `build_cs` + `get_and_clear_witness` + `extend_witness` for one deck without leaving the device: the remask, the circuit's
/// variables and the gather by the wiring run as kernels over `circuit`'s resident layout (`uzk_shuffle_witness_batch`).  Returns
/// the device witness (for `uzk_prove_round1` with `inputs_on_device`; its `pi_values` are `verify_shuffle`'s online inputs) and the
/// new deck.  `None` when the device cannot serve the call: the caller then runs `build_cs` as before.
pub fn gpu_shuffle_witness(
    circuit: &sys::ShuffleCircuit,
    key: &sys::RemarkKey,
    deck: &[MaskedCard],
    bits: &[Vec<[bool; N_WIRE_SELECTORS]>],
    permutation: &Permutation<Fq>,
) -> Option<(sys::ShuffleWitness, Vec<MaskedCard>)> {
    let n = deck.len();
    let iters = sys::UZK_REMARK_ITERATIONS as usize;
    let matrix = permutation.get_matrix();
    if n == 0 || bits.len() != n || bits.iter().any(|b| b.len() != iters) || matrix.len() != n {
        return None;
    }
    let mut perm: Vec<u32> = Vec::with_capacity(n);
    for row in matrix.iter() {
        perm.push(row.iter().position(|v| *v == Fq::ONE)? as u32);
    }
    let e1: Vec<sys::EdPoint> = deck.iter().map(|c| point_to_wire(&c.e1)).collect();
    let e2: Vec<sys::EdPoint> = deck.iter().map(|c| point_to_wire(&c.e2)).collect();
    let digits: Vec<u8> = bits.iter().flat_map(|card| card.iter().map(digit_of)).collect();
    let w = circuit.witness_batch(key, &e1, &e2, &digits, Some(&perm)).ok()?;
    let new_deck = w.e1_out.iter().zip(w.e2_out.iter()).map(|(a, b)| MaskedCard { e1: point_from_wire(a), e2: point_from_wire(b) }).collect();
    Some((w, new_deck))
}
