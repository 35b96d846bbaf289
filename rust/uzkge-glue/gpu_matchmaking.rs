//! matchmaking/src/gpu_matchmaking.rs -- the witness of a batch of matches on the device (cargo feature `gpu`).
//!
//! `build_cs` (matchmaking/src/build_cs.rs) hashes the committed seed, runs the Anemoi stream cipher over (seed, random number) with
//! their traces, and replays `Matchmaking::generate_constraints` to fill 6 027 variables per match of 50 players; `prove_matchmaking`
//! then extends them by the wiring.  `gpu_match_witness` hands a whole batch to `uzk_match_witness_batch` (include/uzkge_gpu.h): the
//! two sponges, the divisions, the exchanges and the gather run as kernels over `circuit`'s resident layout, and the traces never leave
//! the device.  What stays here is what only this side has: the conversions, and the transcript, blinds and r_poly scalars of the
//! five rounds that follow.
//!
//! Returns `None` when the device cannot serve the call (no GPU, a HIP failure, a batch the library refuses): the caller then runs
//! `build_cs` as before.  Nothing here panics on a device error.
//!
//! Layout: an `ark_bn254::Fr`'s Montgomery limbs are the wire words.
use ark_bn254::Fr;
use ark_ff::BigInt;
use uzkge_gpu_sys as sys;

fn to_wire(v: &Fr) -> [u64; 4] {
    (v.0).0
}
fn from_wire(w: &[u64; 4]) -> Fr {
    Fr::new_unchecked(BigInt(*w))
}

/// One match as `prove_matchmaking` takes it: the players' inputs, the committed seed and the random number.
pub struct Match<'a> {
    pub inputs: &'a [Fr],
    pub committed_seed: &'a Fr,
    pub random_number: &'a Fr,
}

/// `build_cs` + `get_and_clear_witness` + `extend_witness` for every match of `batch` without leaving the device.  Returns the device
/// witnesses (for `uzk_prove_round1` with `inputs_on_device` and no wire selectors; `pi_values` are `verify_matchmaking`'s online
/// inputs), the matched order of every match and the commitment of every seed.
pub fn gpu_match_witness(circuit: &sys::MatchCircuit, batch: &[Match]) -> Option<(sys::MatchWitness, Vec<Vec<Fr>>, Vec<Fr>)> {
    let players = circuit.players() as usize;
    if batch.is_empty() || batch.len() > sys::UZK_MATCH_CS_MAX_BATCH as usize || batch.iter().any(|m| m.inputs.len() != players) {
        return None;
    }
    let inputs: Vec<[u64; 4]> = batch.iter().flat_map(|m| m.inputs.iter().map(to_wire)).collect();
    let seeds: Vec<[u64; 4]> = batch.iter().map(|m| to_wire(m.committed_seed)).collect();
    let randoms: Vec<[u64; 4]> = batch.iter().map(|m| to_wire(m.random_number)).collect();
    let w = circuit.witness_batch(&inputs, &seeds, &randoms).ok()?;
    let outputs = w.outputs.chunks_exact(players).map(|row| row.iter().map(from_wire).collect()).collect();
    let commitments = w.commitments.iter().map(from_wire).collect();
    Some((w, outputs, commitments))
}
