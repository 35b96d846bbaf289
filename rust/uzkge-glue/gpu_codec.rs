//! shuffle/src/gpu_codec.rs -- compressed points and keys decoded on the device (cargo feature `gpu-reveal-snark`).
//!
//! `load_groth16_pk` (shuffle/src/reveal_with_snark.rs) reads groth16_pk.bin with `deserialize_compressed_unchecked`: 22 801 G1 and
//! 4 872 G2 square roots on one CPU thread, unchecked because checking costs more still.  `gpu_load_reveal_key` hands the file's bytes
//! to `uzk_reveal_circuit_create_compressed` (include/uzkge_gpu.h, "the point codec"): every point is decoded on the device, strictly,
//! and with `validate` the G2 points are also held to the subgroup -- the result is the resident circuit `gpu_reveal_cards_with_snark`
//! (gpu_reveal_snark.rs) proves with, so no arkworks `ProvingKey` is ever built on this path.
//!
//! `gpu_points_from_hex` is `hex_to_point` (shuffle/src/utils.rs; Compress::Yes, Validate::Yes) over a slice of the SDK's key strings
//! in one call: the public keys of a table, a joint key, a deck.
//!
//! Both return `None` when the device cannot serve the call (no GPU, a HIP failure) or refuses an input (an encoding that is not
//! canonical, not a point, or outside the subgroup): the caller then runs the reference's function as before, which names the error.
//! Nothing here panics.
use ark_ed_on_bn254::{EdwardsAffine, EdwardsProjective, Fq};
use ark_ff::BigInt;
use uzkge_gpu_sys as sys;

fn point_from_wire(w: &sys::EdPoint) -> EdwardsProjective {
    EdwardsAffine::new_unchecked(Fq::new_unchecked(BigInt(w[0])), Fq::new_unchecked(BigInt(w[1]))).into()
}

/// The reveal circuit over the bytes of a compressed `ProvingKey<Bn254>`, resident on the device: once per game, not per card.
/// `validate`: also the subgroup check of the key's G2 points (what `deserialize_compressed` would add to `_unchecked`).
pub fn gpu_load_reveal_key(bytes: &[u8], validate: bool) -> Option<sys::RevealCircuit> {
    let layout = sys::codec::g16_pk_layout(bytes).ok()?;
    if layout.count[sys::UZK_PK_A_QUERY as usize] != sys::UZK_REVEAL_CS_VARS as u64 || layout.count[sys::UZK_PK_GAMMA_ABC_G1 as usize] != sys::UZK_REVEAL_CS_INPUTS as u64 {
        return None;                               // a key of another circuit
    }
    sys::RevealCircuit::from_compressed(bytes, validate).ok()
}

/// `hex_to_point` for every string: curve and subgroup checked on the device.  `None` if any string is not 32 hexadecimal bytes or any
/// point is refused.
pub fn gpu_points_from_hex(strings: &[&str]) -> Option<Vec<EdwardsProjective>> {
    if strings.is_empty() {
        return Some(Vec::new());
    }
    if strings.len() > sys::UZK_CODEC_MAX_BATCH as usize {
        return None;
    }
    let mut enc = Vec::with_capacity(32 * strings.len());
    for s in strings {
        let bytes = hex::decode(s.trim_start_matches("0x")).ok()?;
        if bytes.len() != 32 {
            return None;
        }
        enc.extend_from_slice(&bytes);
    }
    let (points, status) = sys::codec::ed_decompress(&enc, true).ok()?;
    if status.iter().any(|&s| s != 0) {
        return None;
    }
    Some(points.iter().map(point_from_wire).collect())
}
