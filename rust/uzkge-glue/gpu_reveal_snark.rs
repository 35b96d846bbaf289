//! shuffle/src/gpu_reveal_snark.rs -- the snark reveal path of a deck on the device (cargo feature `gpu-reveal-snark`).
//!
//! `reveal_card_with_snark` (shuffle/src/sdk.rs) proves one card: arkworks synthesises RevealCircuit (reveal_with_snark.rs) on the
//! CPU, 4869 variables, and runs Groth16::prove over them -- 52 times per player per deck.  `gpu_reveal_cards_with_snark` hands the
//! deck to `uzk_reveal_prove_snark_batch` (include/uzkge_gpu.h): the constraint system's matrices are the library's own, the
//! assignments are built on the device and the prover reads them there.  What stays here is what only this side has: the blinds r, s
//! (drawn from the caller's rng per card, r first, as create_random_proof draws them) and the conversions.
//!
//! `gpu_reveal_circuit` uploads a ProvingKey once (a game's lifetime); both return `None` when the device cannot serve the call (no
//! GPU, a HIP failure, a key of another circuit): the caller then runs the reference's loop as before.  Nothing here panics.
//!
//! Layout: `ark_ed_on_bn254::Fq` is `ark_bn254::Fr` -- a coordinate's Montgomery limbs are the wire words; the secret goes over as
//! the plain integer `into_bigint()`; G1 / G2 points are affine Montgomery limbs, infinity all zeros.
use ark_bn254::{Bn254, Fq as BaseFq, Fq2, Fr as ScalarFr, G1Affine, G2Affine};
use ark_ec::{AffineRepr, CurveGroup};
use ark_ed_on_bn254::{EdwardsAffine, EdwardsProjective, Fq, Fr};
use ark_ff::{BigInt, PrimeField, UniformRand};
use ark_groth16::{Proof, ProvingKey};
use ark_std::rand::{CryptoRng, RngCore};
use uzkge_gpu_sys as sys;

use crate::{keygen::Keypair, MaskedCard, RevealCard};

fn point_to_wire(p: &EdwardsProjective) -> sys::EdPoint {
    let a = p.into_affine();
    [(a.x.0).0, (a.y.0).0]
}
fn point_from_wire(x: &[u64; 4], y: &[u64; 4]) -> EdwardsProjective {
    EdwardsAffine::new_unchecked(Fq::new_unchecked(BigInt(*x)), Fq::new_unchecked(BigInt(*y))).into()
}
fn g1_to_wire(p: &G1Affine) -> sys::uzk_g1_affine {
    match p.xy() {
        Some((x, y)) => sys::uzk_g1_affine { x: (x.0).0, y: (y.0).0 },
        None => sys::uzk_g1_affine::default(),
    }
}
fn g2_to_wire(p: &G2Affine) -> sys::uzk_g2_affine {
    match p.xy() {
        Some((x, y)) => sys::uzk_g2_affine { x: [(x.c0.0).0, (x.c1.0).0], y: [(y.c0.0).0, (y.c1.0).0] },
        None => sys::uzk_g2_affine::default(),
    }
}
fn g1_from_wire(w: &sys::uzk_g1_affine) -> G1Affine {
    if w.x == [0u64; 4] && w.y == [0u64; 4] {
        return G1Affine::identity();
    }
    G1Affine::new_unchecked(BaseFq::new_unchecked(BigInt(w.x)), BaseFq::new_unchecked(BigInt(w.y)))
}
fn g2_from_wire(w: &sys::uzk_g2_affine) -> G2Affine {
    if w.x == [[0u64; 4]; 2] && w.y == [[0u64; 4]; 2] {
        return G2Affine::identity();
    }
    let f = |c: &[[u64; 4]; 2]| Fq2::new(BaseFq::new_unchecked(BigInt(c[0])), BaseFq::new_unchecked(BigInt(c[1])));
    G2Affine::new_unchecked(f(&w.x), f(&w.y))
}

/// The reveal circuit over `pk`'s points, resident on the device: once per game, not per card.
pub fn gpu_reveal_circuit(pk: &ProvingKey<Bn254>) -> Option<sys::RevealCircuit> {
    let a: Vec<_> = pk.a_query.iter().map(g1_to_wire).collect();
    let b1: Vec<_> = pk.b_g1_query.iter().map(g1_to_wire).collect();
    let l: Vec<_> = pk.l_query.iter().map(g1_to_wire).collect();
    let h: Vec<_> = pk.h_query.iter().map(g1_to_wire).collect();
    let b2: Vec<_> = pk.b_g2_query.iter().map(g2_to_wire).collect();
    if a.len() != sys::UZK_REVEAL_CS_VARS as usize || b1.len() != a.len() || b2.len() != a.len() || pk.vk.gamma_abc_g1.len() != sys::UZK_REVEAL_CS_INPUTS as usize {
        return None;
    }
    let desc = sys::uzk_g16_key_desc {
        n_vars: a.len() as u32,
        n_inputs: pk.vk.gamma_abc_g1.len() as u32,
        n_constraints: 0,
        reserved: 0,
        l_query_len: l.len() as u64,
        h_query_len: h.len() as u64,
        alpha_g1: g1_to_wire(&pk.vk.alpha_g1),
        beta_g1: g1_to_wire(&pk.beta_g1),
        delta_g1: g1_to_wire(&pk.delta_g1),
        beta_g2: g2_to_wire(&pk.vk.beta_g2),
        delta_g2: g2_to_wire(&pk.vk.delta_g2),
        a_query: a.as_ptr(),
        b_g1_query: b1.as_ptr(),
        l_query: l.as_ptr(),
        h_query: h.as_ptr(),
        b_g2_query: b2.as_ptr(),
        row_ptr: [std::ptr::null(); 3],
        col: [std::ptr::null(); 3],
        val: [std::ptr::null(); 3],
    };
    sys::RevealCircuit::create(&desc).ok()
}

/// `reveal_card_with_snark` for every card of `masked_cards` under one keypair: the reveal cards and their Groth16 proofs, in card
/// order.  The public inputs of proof i are masked_cards[i].e1, the reveal card and keypair.public, x then y each.
pub fn gpu_reveal_cards_with_snark<R: CryptoRng + RngCore>(
    prng: &mut R,
    circuit: &sys::RevealCircuit,
    keypair: &Keypair,
    masked_cards: &[MaskedCard],
) -> Option<Vec<(RevealCard, Proof<Bn254>)>> {
    if masked_cards.is_empty() {
        return Some(Vec::new());
    }
    if masked_cards.len() > sys::UZK_REVEAL_CS_MAX_BATCH as usize {
        return None;
    }
    let e1: Vec<sys::EdPoint> = masked_cards.iter().map(|c| point_to_wire(&c.e1)).collect();
    let mut r = Vec::with_capacity(e1.len());
    let mut s = Vec::with_capacity(e1.len());
    for _ in 0..e1.len() {
        r.push((ScalarFr::rand(prng).0).0);
        s.push((ScalarFr::rand(prng).0).0);
    }
    let sk: Fr = keypair.secret;
    let (statements, proofs) = circuit.prove_snark_batch(&sk.into_bigint().0, &e1, &r, &s).ok()?;
    let mut out = Vec::with_capacity(e1.len());
    for (st, p) in statements.iter().zip(proofs.iter()) {
        if point_from_wire(&st[4], &st[5]) != keypair.public {
            return None;                           // the keypair is not (sk, sk G): the caller's loop decides
        }
        out.push((point_from_wire(&st[2], &st[3]), Proof { a: g1_from_wire(&p.a), b: g2_from_wire(&p.b), c: g1_from_wire(&p.c) }));
    }
    Some(out)
}

/// `gpu_reveal_cards_with_snark` with every proof as the contract takes it: the eight words a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0,
/// c.x, c.y of `RevealedCardWithSnarkProof` (sdk.rs) as 0x-prefixed hex, cut from the blob the device encodes
/// (`uzk_reveal_prove_snark_batch_finish`): no point is decoded or re-encoded here.
pub fn gpu_reveal_cards_with_snark_hex<R: CryptoRng + RngCore>(
    prng: &mut R,
    circuit: &sys::RevealCircuit,
    keypair: &Keypair,
    masked_cards: &[MaskedCard],
) -> Option<Vec<(RevealCard, [String; 8])>> {
    if masked_cards.is_empty() {
        return Some(Vec::new());
    }
    if masked_cards.len() > sys::UZK_REVEAL_CS_MAX_BATCH as usize {
        return None;
    }
    let e1: Vec<sys::EdPoint> = masked_cards.iter().map(|c| point_to_wire(&c.e1)).collect();
    let mut r = Vec::with_capacity(e1.len());
    let mut s = Vec::with_capacity(e1.len());
    for _ in 0..e1.len() {
        r.push((ScalarFr::rand(prng).0).0);
        s.push((ScalarFr::rand(prng).0).0);
    }
    let sk: Fr = keypair.secret;
    let (statements, _, blobs) = circuit.prove_snark_finish(&sk.into_bigint().0, &e1, &r, &s).ok()?;
    let per = sys::UZK_G16_PROOF_BYTES as usize;
    let mut out = Vec::with_capacity(e1.len());
    for (st, blob) in statements.iter().zip(blobs.chunks_exact(per)) {
        if point_from_wire(&st[4], &st[5]) != keypair.public {
            return None;                           // the keypair is not (sk, sk G): the caller's loop decides
        }
        let words: [String; 8] = std::array::from_fn(|k| {
            let mut h = String::with_capacity(66);
            h.push_str("0x");
            for b in &blob[32 * k..32 * k + 32] {
                h.push_str(&format!("{:02x}", b));
            }
            h
        });
        out.push((point_from_wire(&st[2], &st[3]), words));
    }
    Some(out)
}
