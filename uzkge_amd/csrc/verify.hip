// Batch PlonK verification up to the pairing: M proofs under one verifier key are folded into the two G1 points of ONE check
//     e(L, [tau] G2) = e(R, G2),      L = sum_i rho_i left_i,   R = sum_i rho_i right_i
// (uzkge/src/plonk/verifier.rs:17-164 with batch_verify_diff_points, kzg_poly_commitment.rs:373-422, flattened to (base, scalar)
// products; tests/plonk_batch_ref.py is the restatement on Python integers).  Everything per proof runs on the device:
//
//   verify_decode      one workgroup per proof: 51 (41) big-endian words -> limbs, compared with p / r, into Montgomery form; the
//                      curve equation on the 16 (13) points; the proof's points go into the point arrays of the two MSMs
//   verify_transcript  Keccak-256 (padding byte 0x01) over the growing transcript of utils/transcript.rs, started from the key's
//                      cached sponge state; seven challenges.  Two forms: a proof's state spread over a half wave
//                      (verify_transcript_lanes, what a fold runs unless told otherwise) and one proof per lane (verify_transcript)
//   verify_scalars     one lane per proof: Z_H(zeta), L_1(zeta), PI(zeta) (one inversion: Montgomery's trick through a workspace),
//                      r(zeta), the scalars of r(X), the powers of the two batch challenges -> the weighted coefficient of every base
//   verify_reduce      one workgroup per base of the key: its coefficients summed over the batch (no atomics)
//   two MSMs           R over 45 + 16 M points, L over 2 M, through msm_run
//
// The transcript is a list of 32-byte words per challenge (VfSeg: where the words come from), built once per key on the host, so
// either transcript kernel is one loop over words.  Spread form: lane i < 25 of a half wave holds state word i, the permutation
// goes through cross-lane moves, no LDS.  Per-lane form: the state in registers (static indices only), the lanes waiting to be
// absorbed in the LDS, one column per thread, the permutation inlined at two places.
#include <cstring>

#include "ctx.hpp"
#include "handles.hpp"
#include "host_math.hpp"
#include "keccak.hpp"
#include "lane_tools.hpp"

namespace uzk {

constexpr uint32_t kVfFixed = 45;          // bases shared by the batch: the key's 44 commitments and g1_0
constexpr uint32_t kVfPerProof = 16;       // cm_w (5), cm_wsel (3), cm_t (5), cm_z, the two opening witnesses
constexpr uint32_t kVfWords = 51;          // row length of the decoded words
constexpr uint32_t kVfChallenges = 7;
enum { VF_Q = 0, VF_S = 9, VF_QB = 14, VF_PRK = 15, VF_QECC = 19, VF_PK = 20, VF_GEN = 32, VF_G0 = 44 };
enum { VS_W = 0, VS_WSEL = 5, VS_T = 8, VS_Z = 13, VS_OPEN = 14 };          // slots of a proof's own points
enum { VF_SRC_PROOF = 0, VF_SRC_PI = 1, VF_SRC_KEY = 2, VF_SRC_ZETA = 3, VF_SRC_ZETA_OMEGA = 4 };
constexpr uint32_t kVfRate = 17;           // lanes of the 136-byte rate
constexpr uint32_t kVfBuf = 20;            // a word of 4 lanes may start at lane 16
constexpr uint32_t kVfBlock = 64;

// word indices of PlonkProof::to_bytes_be (indexer.rs:539-590), with and without the "shuffle" feature
struct VfLayout {
    int n_words, n_points, cm_wsel, cm_t, cm_z, prk3, prk4, w, w_om, z_om, s, q_ecc, wsel, open0;
};
UZK_HD VfLayout vf_layout(bool shuffle) {
    return shuffle ? VfLayout{51, 16, 10, 16, 26, 28, 29, 30, 35, 38, 39, 43, 44, 47}
                   : VfLayout{41, 13, -1, 10, 20, 22, 23, 24, 29, 32, 33, -1, -1, 37};
}

struct VfSeg { uint32_t src, off, n; };    // n words from word `off` of the source
struct VfKey {
    Fp k[5], anemoi_g, anemoi_g_inv, edwards_a, root;
    uint32_t cs_log, n_pi, shuffle, pos;   // pos: lanes of the cached state still waiting in `tail`
    uint64_t sponge[25];
    uint64_t tail[kVfRate];
    uint64_t pcs_hdr[12];                  // "New PCS-Batch-Eval Protocol", r, cs_size + 2
    VfSeg prog[kVfChallenges][8];
    uint32_t nseg[kVfChallenges];
};

// ---- the sponge over Keccak-f[1600] (vf_keccak_f: keccak.hpp, shared with srscheck.hip) -----------------------------------------
UZK_HD uint64_t vf_bswap(uint64_t v) { return __builtin_bswap64(v); }

// The lanes waiting to be absorbed: lane l of this thread at buf[l * stride] (device: a column of the LDS; host: stride 1).
// vf_flush: pos >= 17 -- absorb a block, keep what lies beyond it.
UZK_HD void vf_flush(uint64_t (&s)[25], uint64_t* buf, uint32_t stride, uint32_t& pos) {
#pragma unroll
    for (uint32_t l = 0; l < kVfRate; ++l) s[l] ^= buf[l * stride];
    vf_keccak_f(s);
    for (uint32_t l = kVfRate; l < pos; ++l) buf[(l - kVfRate) * stride] = buf[l * stride];
    pos -= kVfRate;
}
// pad_lane: the message's last bytes (fewer than eight) followed by the byte 0x01; pos <= 16
UZK_HD void vf_finalize(uint64_t (&s)[25], uint64_t* buf, uint32_t stride, uint32_t pos, uint64_t pad_lane) {
    buf[pos * stride] = pad_lane;
    for (uint32_t l = pos + 1; l < kVfRate; ++l) buf[l * stride] = 0;
    buf[(kVfRate - 1) * stride] ^= 0x8000000000000000ull;
#pragma unroll
    for (uint32_t l = 0; l < kVfRate; ++l) s[l] ^= buf[l * stride];
    vf_keccak_f(s);
}

// a canonical element as the four lanes of its 32 big-endian bytes
UZK_HD void vf_be_lanes(const Fp& c, uint64_t (&l)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = vf_bswap(((uint64_t)c.v[7 - 2 * j] << 32) | c.v[6 - 2 * j]);
}

// ---- decode and check ---------------------------------------------------------------------------------------------------------
// One workgroup per proof, one thread per word.  flag: 1 = word >= its modulus; the point threads then add 2 = not on the curve.
// A proof with a nonzero status leaves infinities in the point arrays (and the scalar kernel leaves zeros).
__global__ __launch_bounds__(kVfBlock) void vf_decode_kernel(const uint8_t* __restrict__ proofs, uint32_t proof_bytes, int shuffle, Fp* __restrict__ words,
                                                             Affine* __restrict__ pts_r, Affine* __restrict__ pts_l, uint8_t* __restrict__ status) {
    __shared__ uint32_t flag[kVfBlock];
    __shared__ uint32_t verdict;
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const VfLayout L = vf_layout(shuffle != 0);
    Fp* row = words + (size_t)i * kVfWords;
    uint32_t f = 0;
    if (t < (uint32_t)L.n_words) {
        const Fp v = load_be32(proofs + (size_t)i * proof_bytes + 32u * t);
        const bool coord = t < (uint32_t)L.prk3 || t >= (uint32_t)L.open0;
        f = (coord ? below_modulus<FqCfg>(v) : below_modulus<FrCfg>(v)) ? 0u : 1u;
        row[t] = coord ? Fq::to_mont(v) : Fr::to_mont(v);
    }
    flag[t] = f;
    __syncthreads();
    // point p of the proof: words 2 p, 2 p + 1 up to cm_z, then the two opening witnesses
    const uint32_t lead = (uint32_t)L.prk3 / 2;
    const bool is_point = t < (uint32_t)L.n_points;
    const uint32_t pw = t < lead ? 2 * t : (uint32_t)L.open0 + 2 * (t - lead);
    Affine p;
    p.x = Fq::zero(); p.y = Fq::zero();
    uint32_t g = 0;
    if (is_point) {
        p.x = row[pw]; p.y = row[pw + 1];
        if (!(flag[pw] | flag[pw + 1]) && !affine_is_inf(p) && !g1_on_curve(p)) g = 2;
    }
    __syncthreads();
    flag[t] |= g;
    __syncthreads();
    if (t == 0) {
        uint32_t any = 0;
        for (uint32_t k = 0; k < kVfBlock; ++k) any |= flag[k];
        verdict = (any & 1) ? 1u : (any & 2) ? 2u : 0u;
        status[i] = (uint8_t)verdict;
    }
    __syncthreads();
    if (verdict != 0) { p.x = Fq::zero(); p.y = Fq::zero(); }
    Affine* own = pts_r + kVfFixed + (size_t)i * kVfPerProof;
    if (is_point) {
        // without wire selectors the points are cm_w (5), cm_t (5), cm_z, the witnesses: slots 0..4, 8..12, 13, 14, 15
        const uint32_t slot = shuffle ? t : (t < 5 ? t : t + 3);
        own[slot] = p;
        if (slot >= VS_OPEN) pts_l[(size_t)i * 2 + (slot - VS_OPEN)] = p;
    } else if (t < kVfPerProof) {
        Affine inf;
        inf.x = Fq::zero(); inf.y = Fq::zero();
        own[VS_WSEL + (t - (uint32_t)L.n_points)] = inf;
    }
}

// ---- transcript ---------------------------------------------------------------------------------------------------------------
// digest (lanes 0..3 read as a big-endian integer) mod r: below 2^256 < 6 r
UZK_HD Fp vf_challenge_of4(uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3) {
    const uint64_t w[4] = {vf_bswap(s3), vf_bswap(s2), vf_bswap(s1), vf_bswap(s0)};
    Fp c;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c.v[2 * j] = (uint32_t)w[j]; c.v[2 * j + 1] = (uint32_t)(w[j] >> 32); }
    for (int k = 0; k < 5; ++k) c = Fr::reduce_once(c);
    return c;
}
UZK_HD Fp vf_challenge_of(const uint64_t (&s)[25]) { return vf_challenge_of4(s[0], s[1], s[2], s[3]); }

__global__ __launch_bounds__(kVfBlock) void vf_transcript_kernel(const VfKey* __restrict__ key, const uint8_t* __restrict__ proofs, uint32_t proof_bytes,
                                                                 const Fp* __restrict__ pi, const uint8_t* __restrict__ status, Fp* __restrict__ chal, uint32_t m) {
    __shared__ uint64_t lanes[kVfBuf * kVfBlock];
    const uint32_t i = blockIdx.x * kVfBlock + threadIdx.x;
    const bool live = i < m && status[i < m ? i : 0] == 0;
    if (live) {
        uint64_t* buf = lanes + threadIdx.x;
        const uint64_t* blob = reinterpret_cast<const uint64_t*>(proofs + (size_t)i * proof_bytes);
        const Fp* my_pi = pi + (size_t)i * key->n_pi;
        uint64_t s[25];
#pragma unroll
        for (int l = 0; l < 25; ++l) s[l] = key->sponge[l];
        uint32_t pos = key->pos;
        for (uint32_t l = 0; l < pos; ++l) buf[l * kVfBlock] = key->tail[l];
        Fp zeta = Fr::zero(), zeta_omega = Fr::zero();            // canonical
#pragma unroll 1
        for (uint32_t h = 0; h < kVfChallenges; ++h) {
            const uint32_t nseg = key->nseg[h];
#pragma unroll 1
            for (uint32_t sg = 0; sg < nseg; ++sg) {
                const VfSeg seg = key->prog[h][sg];
#pragma unroll 1
                for (uint32_t w = 0; w < seg.n; ++w) {
                    uint64_t l4[4];
                    if (seg.src == VF_SRC_PROOF) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) l4[j] = blob[(size_t)(seg.off + w) * 4 + j];
                    } else if (seg.src == VF_SRC_PI) {
                        vf_be_lanes(Fr::from_mont(my_pi[seg.off + w]), l4);
                    } else if (seg.src == VF_SRC_KEY) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) l4[j] = key->pcs_hdr[(seg.off + w) * 4 + j];
                    } else {
                        vf_be_lanes(seg.src == VF_SRC_ZETA ? zeta : zeta_omega, l4);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) buf[(pos + j) * kVfBlock] = l4[j];
                    pos += 4;
                    if (pos >= kVfRate) vf_flush(s, buf, kVfBlock, pos);
                }
            }
            // the single byte 0x01 appended before gamma is the whole tail of that message
            vf_finalize(s, buf, kVfBlock, pos, h == 1 ? 0x0101ull : 0x01ull);
            const Fp c = vf_challenge_of(s);
            chal[(size_t)i * kVfChallenges + h] = Fr::to_mont(c);
            if (h == 3) {
                zeta = c;
                zeta_omega = Fr::from_mont(Fr::mul(Fr::to_mont(c), key->root));
            }
            // the challenge is the new state of the transcript
            uint64_t l4[4];
            vf_be_lanes(c, l4);
#pragma unroll
            for (int j = 0; j < 4; ++j) buf[j * kVfBlock] = l4[j];
            pos = 4;
#pragma unroll
            for (int l = 0; l < 25; ++l) s[l] = 0;
        }
    }
}

// ---- the same transcript with a proof's sponge state spread over lanes ------------------------------------------------------------
// One proof per half wave: lane i < 25 holds state word i = x + 5 y, lanes 0..19 also hold the message lane that waits at rate
// position i.  theta's column parities, rho / pi and chi's row neighbours go through cross-lane moves (nine 64-bit moves a round);
// no LDS, no barrier.  Every lane of a half wave runs the same control flow (one proof, one key); lanes 25..31 compute along with
// clamped sources and are never read.  The dependent chain per permutation is a few hundred cycles instead of a few thousand,
// and a batch of m proofs fills m / 2 waves instead of m / 64.
constexpr uint32_t kVfGroup = 32;
struct VfLaneMap { uint32_t up5, up10, up15, up20, left, right1, right2, pi_src, rot; };
// rotation of word i = x + 5 y (the rho offsets of the Keccak specification)
__constant__ uint8_t kVfRho[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
__device__ __forceinline__ VfLaneMap vf_lane_map(uint32_t lane) {
    const uint32_t i = lane < 25 ? lane : 0, x = i % 5, y = i / 5;
    VfLaneMap m;
    m.up5 = (i + 5) % 25; m.up10 = (i + 10) % 25; m.up15 = (i + 15) % 25; m.up20 = (i + 20) % 25;
    m.left = 5 * y + (x + 4) % 5; m.right1 = 5 * y + (x + 1) % 5; m.right2 = 5 * y + (x + 2) % 5;
    // pi: word (x', y') of the new state is the rotated word (x, y) of the old one with x' = y, y' = (2 x + 3 y) mod 5; for this lane
    // as (x', y'): y = x', x = 3 (y' - 3 y) mod 5 (2 * 3 = 1 mod 5)
    const uint32_t sy = x, sx = (3 * ((y + 15 - 3 * sy) % 5)) % 5;
    m.pi_src = sx + 5 * sy;
    m.rot = kVfRho[i];
    return m;
}
__device__ __forceinline__ uint64_t vf_lane_get(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, (int)kVfGroup), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, (int)kVfGroup);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t vf_keccak_f_lanes(uint64_t a, const VfLaneMap& m, uint32_t lane) {
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
                                 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
                                 0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
                                 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        const uint64_t c = a ^ vf_lane_get(a, m.up5) ^ vf_lane_get(a, m.up10) ^ vf_lane_get(a, m.up15) ^ vf_lane_get(a, m.up20);
        a ^= vf_lane_get(c, m.left) ^ vf_rol(vf_lane_get(c, m.right1), 1);
        const uint64_t rotated = m.rot ? (a << m.rot) | (a >> (64 - m.rot)) : a;
        // the source lane reads its own rotation: rotate where the word IS, then move it
        const uint64_t b = vf_lane_get(rotated, m.pi_src);
        a = b ^ (~vf_lane_get(b, m.right1) & vf_lane_get(b, m.right2));
        if (lane == 0) a ^= RC[r];
    }
    return a;
}
// pos >= 17: absorb a block; what waits beyond it moves to the front
__device__ __forceinline__ void vf_flush_lanes(uint64_t& a, uint64_t& pending, uint32_t& pos, const VfLaneMap& m, uint32_t lane) {
    if (lane < kVfRate) a ^= pending;
    a = vf_keccak_f_lanes(a, m, lane);
    pending = vf_lane_get(pending, lane + kVfRate < kVfGroup ? lane + kVfRate : lane);
    pos -= kVfRate;
}
__device__ __forceinline__ void vf_push_word_lanes(uint64_t& a, uint64_t& pending, uint32_t& pos, const uint64_t (&l4)[4], const VfLaneMap& m, uint32_t lane) {
    const uint32_t k = lane - pos;                                // this lane takes lane k of the word, if k < 4
    const uint64_t v = k == 0 ? l4[0] : k == 1 ? l4[1] : k == 2 ? l4[2] : l4[3];
    if (k < 4) pending = v;
    pos += 4;
    if (pos >= kVfRate) vf_flush_lanes(a, pending, pos, m, lane);
}

__global__ __launch_bounds__(kVfBlock) void vf_transcript_lanes_kernel(const VfKey* __restrict__ key, const uint8_t* __restrict__ proofs, uint32_t proof_bytes,
                                                                       const Fp* __restrict__ pi, const uint8_t* __restrict__ status, Fp* __restrict__ chal, uint32_t m) {
    const uint32_t gt = blockIdx.x * kVfBlock + threadIdx.x;
    const uint32_t i = gt / kVfGroup, lane = gt % kVfGroup;
    // whole half waves are live or dead together; a dead one runs nothing (the moves below stay inside a half wave)
    const bool live = i < m && status[i < m ? i : 0] == 0;
    if (live) {
        const VfLaneMap map = vf_lane_map(lane);
        const uint64_t* blob = reinterpret_cast<const uint64_t*>(proofs + (size_t)i * proof_bytes);
        const Fp* my_pi = pi + (size_t)i * key->n_pi;
        uint64_t a = lane < 25 ? key->sponge[lane] : 0;
        uint32_t pos = key->pos;
        uint64_t pending = lane < pos ? key->tail[lane < kVfRate ? lane : 0] : 0;
        Fp zeta = Fr::zero(), zeta_omega = Fr::zero();
#pragma unroll 1
        for (uint32_t h = 0; h < kVfChallenges; ++h) {
            const uint32_t nseg = key->nseg[h];
#pragma unroll 1
            for (uint32_t sg = 0; sg < nseg; ++sg) {
                const VfSeg seg = key->prog[h][sg];
#pragma unroll 1
                for (uint32_t w = 0; w < seg.n; ++w) {
                    uint64_t l4[4];
                    if (seg.src == VF_SRC_PROOF) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) l4[j] = blob[(size_t)(seg.off + w) * 4 + j];
                    } else if (seg.src == VF_SRC_PI) {
                        vf_be_lanes(Fr::from_mont(my_pi[seg.off + w]), l4);
                    } else if (seg.src == VF_SRC_KEY) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) l4[j] = key->pcs_hdr[(seg.off + w) * 4 + j];
                    } else {
                        vf_be_lanes(seg.src == VF_SRC_ZETA ? zeta : zeta_omega, l4);
                    }
                    vf_push_word_lanes(a, pending, pos, l4, map, lane);
                }
            }
            // padding: the byte 0x01 (after the single byte 0x01 in front of gamma) at `pos`, zeros, 0x80 in the last byte of the rate
            uint64_t last = lane == pos ? (h == 1 ? 0x0101ull : 0x01ull) : lane < pos ? pending : 0;
            if (lane == kVfRate - 1) last ^= 0x8000000000000000ull;
            if (lane < kVfRate) a ^= last;
            a = vf_keccak_f_lanes(a, map, lane);
            const Fp c = vf_challenge_of4(vf_lane_get(a, 0), vf_lane_get(a, 1), vf_lane_get(a, 2), vf_lane_get(a, 3));
            if (lane == 0) chal[(size_t)i * kVfChallenges + h] = Fr::to_mont(c);
            if (h == 3) {
                zeta = c;
                zeta_omega = Fr::from_mont(Fr::mul(Fr::to_mont(c), key->root));
            }
            uint64_t l4[4];
            vf_be_lanes(c, l4);
            pending = lane == 0 ? l4[0] : lane == 1 ? l4[1] : lane == 2 ? l4[2] : lane == 3 ? l4[3] : 0;
            pos = 4;
            a = 0;
        }
    }
}

// Keccak-256 of `count` messages (test hook): message i = bytes [offsets[i], offsets[i + 1]), one lane each
__global__ __launch_bounds__(kVfBlock) void vf_keccak_kernel(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets, uint32_t count,
                                                             uint8_t* __restrict__ out) {
    __shared__ uint64_t lanes[kVfBuf * kVfBlock];
    const uint32_t i = blockIdx.x * kVfBlock + threadIdx.x;
    const bool live = i < count;
    if (live) {
        uint64_t* buf = lanes + threadIdx.x;
        const uint8_t* src = msgs + offsets[i];
        const uint64_t len = offsets[i + 1] - offsets[i];
        uint64_t s[25];
#pragma unroll
        for (int l = 0; l < 25; ++l) s[l] = 0;
        uint32_t pos = 0;
#pragma unroll 1
        for (uint64_t at = 0; at + 8 <= len; at += 8) {
            uint64_t v = 0;
            for (int b = 0; b < 8; ++b) v |= (uint64_t)src[at + b] << (8 * b);
            buf[pos * kVfBlock] = v;
            pos += 1;
            if (pos >= kVfRate) vf_flush(s, buf, kVfBlock, pos);
        }
        uint64_t pad = 0;
        const uint32_t rest = (uint32_t)(len & 7);
        for (uint32_t b = 0; b < rest; ++b) pad |= (uint64_t)src[len - rest + b] << (8 * b);
        pad |= 0x01ull << (8 * rest);
        vf_finalize(s, buf, kVfBlock, pos, pad);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int b = 0; b < 8; ++b) out[(size_t)i * 32 + 8 * j + b] = (uint8_t)(s[j] >> (8 * b));
        }
    }
}

// ---- verifier scalars ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fp vf_pow5(const Fp& a) { const Fp a2 = Fr::sqr(a); return Fr::mul(Fr::sqr(a2), a); }

// One lane per proof.  Outputs, every one already times the proof's weight rho:
//   fixed[i][45]   coefficients of the key's commitments and of g1_0 (summed over the batch by vf_reduce_kernel)
//   sc_r[45 + 16 i ..)  coefficients of the proof's own points; sc_l[2 i ..) = rho, rho u
// Formulas: tests/plonk_verifier_oracle.py r_scalars / r_eval_zeta (helpers.rs:681-1002, 1182-1321), plonk_golden_verifier.py.
__global__ __launch_bounds__(kVfBlock) void vf_scalars_kernel(const VfKey* __restrict__ key, const Fp* __restrict__ words, const Fp* __restrict__ chal,
                                                              const Fp* __restrict__ pi, const Fp* __restrict__ rp, const Fp* __restrict__ lag,
                                                              const Fp* __restrict__ weights, const uint8_t* __restrict__ status, Fp* __restrict__ prefix,
                                                              Fp* __restrict__ fixed, Fp* __restrict__ sc_r, Fp* __restrict__ sc_l, uint32_t m) {
    const uint32_t i = blockIdx.x * kVfBlock + threadIdx.x;
    if (i >= m) return;                                           // no barrier and no cross-lane move below
    Fp* F = fixed + (size_t)i * kVfFixed;
    Fp* S = sc_r + kVfFixed + (size_t)i * kVfPerProof;
    Fp* SL = sc_l + (size_t)i * 2;
    if (status[i] != 0) {
        const Fp z = Fr::zero();
        for (uint32_t k = 0; k < kVfFixed; ++k) F[k] = z;
        for (uint32_t k = 0; k < kVfPerProof; ++k) S[k] = z;
        SL[0] = z; SL[1] = z;
        return;
    }
    const bool shuffle = key->shuffle != 0;
    const VfLayout L = vf_layout(shuffle);
    const Fp* W = words + (size_t)i * kVfWords;
    const Fp* C = chal + (size_t)i * kVfChallenges;
    const Fp one = Fr::one();
    const Fp rho = weights[i];
    const Fp beta = C[0], gamma = C[1], alpha = C[2], zeta = C[3], u = C[4];
    const uint32_t n_pi = key->n_pi;

    // Z_H(zeta), and 1 / (zeta - 1), 1 / (zeta - omega^row_j) by ONE inversion
    Fp zn = zeta;
    for (uint32_t k = 0; k < key->cs_log; ++k) zn = Fr::sqr(zn);
    const Fp zh = Fr::sub(zn, one);
    Fp* pre = prefix + (size_t)i * (n_pi + 1);
    Fp prod = one;
#pragma unroll 1
    for (uint32_t j = 0; j <= n_pi; ++j) {
        Fp d = Fr::sub(zeta, j == 0 ? one : rp[j - 1]);
        if (Fr::is_zero(d)) d = one;
        pre[j] = prod;
        prod = Fr::mul(prod, d);
    }
    Fp inv = fr_inv_lane(prod);
    Fp acc = Fr::zero();
#pragma unroll 1
    for (uint32_t j = n_pi; j >= 1; --j) {
        Fp d = Fr::sub(zeta, rp[j - 1]);
        const bool zero = Fr::is_zero(d);
        if (zero) d = one;
        const Fp dinv = Fr::mul(inv, pre[j]);
        inv = Fr::mul(inv, d);
        if (!zero) acc = Fr::add(acc, Fr::mul(Fr::mul(pi[(size_t)i * n_pi + j - 1], lag[j - 1]), dinv));
    }
    const Fp l1 = Fr::is_zero(Fr::sub(zeta, one)) ? Fr::zero() : Fr::mul(zh, inv);      // first_lagrange_poly
    const Fp pi_eval = Fr::mul(acc, zh);                                                 // eval_pi_poly

    Fp w[5], s[4], wo[3], ws[3];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = W[L.w + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = W[L.s + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) wo[k] = W[L.w_om + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ws[k] = shuffle ? W[L.wsel + k] : Fr::zero();
    const Fp prk3 = W[L.prk3], prk4 = W[L.prk4], z_om = W[L.z_om];
    const Fp qe = shuffle ? W[L.q_ecc] : Fr::zero();
    const Fp a = C[5], b = C[6];

    // ---- the commitments opened at zeta: rho a^j each; val_r = rho sum a^j v_j
    Fp pw = rho, val = Fr::zero(), cw[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) { cw[k] = pw; val = Fr::add(val, Fr::mul(pw, w[k])); pw = Fr::mul(pw, a); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { F[VF_S + k] = pw; val = Fr::add(val, Fr::mul(pw, s[k])); pw = Fr::mul(pw, a); }
    F[VF_PRK + 2] = pw; val = Fr::add(val, Fr::mul(pw, prk3)); pw = Fr::mul(pw, a);
    F[VF_PRK + 3] = pw; val = Fr::add(val, Fr::mul(pw, prk4)); pw = Fr::mul(pw, a);
    if (shuffle) {
        F[VF_QECC] = pw; val = Fr::add(val, Fr::mul(pw, qe)); pw = Fr::mul(pw, a);
#pragma unroll
        for (int k = 0; k < 3; ++k) { S[VS_WSEL + k] = pw; val = Fr::add(val, Fr::mul(pw, ws[k])); pw = Fr::mul(pw, a); }
    } else {
        F[VF_QECC] = Fr::zero();
        for (int k = 0; k < 3; ++k) S[VS_WSEL + k] = Fr::zero();
        for (int k = 0; k < 24; ++k) F[VF_PK + k] = Fr::zero();
    }
    const Fp ar = pw;                                              // rho a^J: the factor of every scalar of r(X)

    // ---- r(X)'s scalars (r_scalars) and r(zeta) (r_eval_zeta), walking up the powers of alpha
    const Fp w01 = Fr::mul(w[0], w[1]), w23 = Fr::mul(w[2], w[3]);
    F[VF_Q + 0] = Fr::mul(ar, w[0]); F[VF_Q + 1] = Fr::mul(ar, w[1]); F[VF_Q + 2] = Fr::mul(ar, w[2]); F[VF_Q + 3] = Fr::mul(ar, w[3]);
    F[VF_Q + 4] = Fr::mul(ar, w01); F[VF_Q + 5] = Fr::mul(ar, w23); F[VF_Q + 6] = ar;
    F[VF_Q + 7] = Fr::mul(ar, Fr::mul(Fr::mul(w01, w23), w[4]));
    F[VF_Q + 8] = Fr::neg(Fr::mul(ar, w[4]));
    const Fp a2 = Fr::sqr(alpha);
    Fp z_scalar = alpha, perm = Fr::mul(Fr::mul(alpha, z_om), beta), term1 = Fr::mul(alpha, z_om);
    const Fp beta_zeta = Fr::mul(beta, zeta);
#pragma unroll
    for (int k = 0; k < 5; ++k) z_scalar = Fr::mul(z_scalar, Fr::add(Fr::add(w[k], Fr::mul(key->k[k], beta_zeta)), gamma));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Fp f = Fr::add(Fr::add(w[k], Fr::mul(beta, s[k])), gamma);
        perm = Fr::mul(perm, f);
        term1 = Fr::mul(term1, f);
    }
    term1 = Fr::mul(term1, Fr::add(w[4], gamma));
    const Fp term2 = Fr::mul(l1, a2);
    z_scalar = Fr::add(z_scalar, term2);
    const Fp cz = Fr::add(Fr::mul(ar, z_scalar), Fr::mul(rho, u));       // cm_z: a^J s_z + u b^0
    F[VF_S + 4] = Fr::neg(Fr::mul(ar, perm));
    Fp ap = Fr::mul(a2, alpha);                                    // alpha^3
    Fp boolean = Fr::mul(Fr::mul(w[1], Fr::sub(w[1], one)), ap);
    ap = Fr::mul(ap, alpha);
    boolean = Fr::add(boolean, Fr::mul(Fr::mul(w[2], Fr::sub(w[2], one)), ap));
    ap = Fr::mul(ap, alpha);
    boolean = Fr::add(boolean, Fr::mul(Fr::mul(w[3], Fr::sub(w[3], one)), ap));
    F[VF_QB] = Fr::mul(ar, boolean);
    // the anemoi round: alpha^6 .. alpha^9
    const Fp g = key->anemoi_g, ginv = key->anemoi_g_inv;
    const Fp w3_w0 = Fr::add(w[3], w[0]), w2_w1 = Fr::add(w[2], w[1]);
    const Fp w3_2w0 = Fr::add(w3_w0, w[0]), w2_2w1 = Fr::add(w2_w1, w[1]);
    const Fp g2p1 = Fr::add(Fr::sqr(g), one);
    Fp r_eval = Fr::sub(Fr::add(term1, term2), pi_eval);
    {
        const Fp tmp = Fr::add(Fr::add(w3_w0, Fr::mul(g, w2_w1)), prk3);
        const Fp p5 = vf_pow5(Fr::sub(tmp, wo[2]));
        const Fp t3 = Fr::sub(Fr::add(p5, Fr::mul(g, Fr::sqr(tmp))), Fr::add(w3_2w0, Fr::mul(g, w2_2w1)));
        const Fp t5 = Fr::sub(Fr::add(Fr::add(p5, Fr::mul(g, Fr::sqr(wo[2]))), ginv), wo[0]);
        const Fp tmp2 = Fr::add(Fr::add(Fr::mul(g, w3_w0), Fr::mul(g2p1, w2_w1)), prk4);
        const Fp q5 = vf_pow5(Fr::sub(tmp2, w[4]));
        const Fp t4 = Fr::sub(Fr::add(q5, Fr::mul(g, Fr::sqr(tmp2))), Fr::add(Fr::mul(g, w3_2w0), Fr::mul(g2p1, w2_2w1)));
        const Fp t6 = Fr::sub(Fr::add(Fr::add(q5, Fr::mul(g, Fr::sqr(w[4]))), ginv), wo[1]);
        ap = Fr::mul(ap, alpha);                                   // alpha^6
        Fp apk = Fr::mul(ap, prk3);
        F[VF_PRK + 0] = Fr::mul(ar, apk);
        r_eval = Fr::add(r_eval, Fr::mul(apk, t3));
        ap = Fr::mul(ap, alpha);                                   // alpha^7
        apk = Fr::mul(ap, prk3);
        F[VF_PRK + 1] = Fr::mul(ar, apk);
        r_eval = Fr::add(r_eval, Fr::mul(apk, t4));
        ap = Fr::mul(ap, alpha);                                   // alpha^8
        r_eval = Fr::add(r_eval, Fr::mul(Fr::mul(ap, prk3), t5));
        ap = Fr::mul(ap, alpha);                                   // alpha^9
        r_eval = Fr::add(r_eval, Fr::mul(Fr::mul(ap, prk3), t6));
    }
    if (shuffle) {
        const Fp ea = key->edwards_a;
        const Fp n0 = Fr::sub(one, ws[0]), n1 = Fr::sub(one, ws[1]);
        Fp sel[4];
        sel[0] = Fr::sub(Fr::add(Fr::mul(n0, n1), qe), one);
        sel[1] = Fr::mul(ws[0], n1);
        sel[2] = Fr::mul(n0, ws[1]);
        sel[3] = Fr::mul(ws[0], ws[1]);
        const Fp a10 = Fr::mul(ap, alpha), a11 = Fr::mul(a10, alpha), a12 = Fr::mul(a11, alpha), a13 = Fr::mul(a12, alpha);
        Fp base[6];
        base[0] = Fr::sub(Fr::mul(Fr::mul(a11, w[0]), ea), Fr::mul(a10, w[1]));                                   // pk x
        base[1] = Fr::neg(Fr::add(Fr::mul(Fr::mul(a10, ws[2]), w[0]), Fr::mul(Fr::mul(a11, ws[2]), w[1])));       // pk y
        base[2] = Fr::sub(Fr::mul(Fr::mul(a10, w01), wo[0]), Fr::mul(Fr::mul(a11, w01), wo[1]));                  // pk dxy
        base[3] = Fr::sub(Fr::mul(Fr::mul(a13, w[2]), ea), Fr::mul(a12, w[3]));                                   // generator x
        base[4] = Fr::neg(Fr::add(Fr::mul(Fr::mul(a12, ws[2]), w[2]), Fr::mul(Fr::mul(a13, ws[2]), w[3])));       // generator y
        base[5] = Fr::sub(Fr::mul(Fr::mul(a12, w23), wo[2]), Fr::mul(Fr::mul(a13, w23), w[4]));                   // generator dxy
#pragma unroll
        for (int gi = 0; gi < 6; ++gi) {
            const Fp bs = Fr::mul(ar, base[gi]);
#pragma unroll
            for (int ij = 0; ij < 4; ++ij) F[VF_PK + 4 * gi + ij] = Fr::mul(bs, sel[ij]);
        }
        const Fp sel_sum = Fr::add(Fr::add(sel[0], sel[1]), Fr::add(sel[2], sel[3]));
        const Fp mix = Fr::add(Fr::add(Fr::mul(a10, wo[0]), Fr::mul(a11, wo[1])), Fr::add(Fr::mul(a12, wo[2]), Fr::mul(a13, w[4])));
        const Fp a14 = Fr::mul(a13, alpha), a15 = Fr::mul(a14, alpha), a16 = Fr::mul(a15, alpha);
        const Fp nqe = Fr::sub(one, qe);
        const Fp t7 = Fr::mul(Fr::mul(ws[2], mix), sel_sum);
        const Fp t8 = Fr::mul(a14, Fr::add(Fr::mul(Fr::mul(qe, ws[0]), n0), Fr::mul(nqe, ws[0])));
        const Fp t9 = Fr::mul(a15, Fr::add(Fr::mul(Fr::mul(qe, ws[1]), n1), Fr::mul(nqe, ws[1])));
        const Fp t10 = Fr::mul(Fr::mul(Fr::mul(a16, qe), Fr::sub(one, ws[2])), Fr::add(one, ws[2]));
        r_eval = Fr::sub(r_eval, Fr::add(Fr::add(t7, t8), Fr::add(t9, t10)));
    }
    val = Fr::add(val, Fr::mul(ar, r_eval));
    // the chunks of t: -Z_H(zeta) zeta^((n + 2) c)
    {
        const Fp factor = Fr::mul(zn, Fr::sqr(zeta));
        Fp e = Fr::mul(ar, zh);
#pragma unroll
        for (int c = 0; c < 5; ++c) { S[VS_T + c] = Fr::neg(e); e = Fr::mul(e, factor); }
    }
    // ---- the commitments opened at zeta omega: rho u b^j; val_o
    Fp pb = Fr::mul(rho, u), val_o = Fr::mul(pb, z_om);
    const Fp ru = pb;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pb = Fr::mul(pb, b);
        cw[k] = Fr::add(cw[k], pb);
        val_o = Fr::add(val_o, Fr::mul(pb, wo[k]));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) S[VS_W + k] = cw[k];
    S[VS_Z] = cz;
    F[VF_G0] = Fr::neg(Fr::add(val, val_o));
    const Fp rz = Fr::mul(rho, zeta);
    S[VS_OPEN] = rz;
    S[VS_OPEN + 1] = Fr::mul(Fr::mul(ru, zeta), key->root);
    SL[0] = rho;
    SL[1] = ru;
}

// out[base] = sum_i fixed[i][base]: one workgroup per base
__global__ __launch_bounds__(256) void vf_reduce_kernel(const Fp* __restrict__ fixed, uint32_t m, Fp* __restrict__ out) {
    __shared__ Fp part[256];
    const uint32_t base = blockIdx.x, t = threadIdx.x;
    Fp acc = Fr::zero();
    for (uint32_t i = t; i < m; i += 256) acc = Fr::add(acc, fixed[(size_t)i * kVfFixed + base]);
    part[t] = acc;
    __syncthreads();
    for (uint32_t step = 128; step > 0; step >>= 1) {
        if (t < step) part[t] = Fr::add(part[t], part[t + step]);
        __syncthreads();
    }
    if (t == 0) out[base] = part[0];
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------
struct VfEntry {
    int device = 0;
    uint32_t cs_size = 0, n_pi = 0, shuffle = 0;
    VfKey* d_key = nullptr;
    Fp* d_consts = nullptr;        // pi_root_powers (n_pi), pi_lagrange (n_pi)
    Affine* d_bases = nullptr;     // kVfFixed points
};
static HandleTable<VfEntry> g_vf(5ull << 59);

static bool vf_lookup(uint64_t h, VfEntry* out) { return g_vf.get(h, out); }
// frees the key's device memory; the calling thread's current device is left as it was
static void vf_free(const VfEntry& e) {
    DeviceGuard on(e.device);
    if (e.d_key) (void)hipFree(e.d_key);
    if (e.d_consts) (void)hipFree(e.d_consts);
    if (e.d_bases) (void)hipFree(e.d_bases);
}
static uint32_t vf_proof_bytes(uint32_t shuffle) { return 32u * (uint32_t)vf_layout(shuffle != 0).n_words; }

// host side of the sponge (stride 1): the bytes every proof under this key starts with
struct HostSponge {
    uint64_t s[25] = {0}, buf[kVfBuf] = {0};
    uint32_t pos = 0;
    void word(const uint8_t* be32) {
        for (int j = 0; j < 4; ++j) { uint64_t v; std::memcpy(&v, be32 + 8 * j, 8); buf[pos + j] = v; }
        pos += 4;
        if (pos >= kVfRate) vf_flush(s, buf, 1, pos);
    }
    void lane(uint64_t v) { buf[pos++] = v; if (pos >= kVfRate) vf_flush(s, buf, 1, pos); }
    void element(const Fp& canonical) { uint64_t l[4]; vf_be_lanes(canonical, l); for (int j = 0; j < 4; ++j) lane(l[j]); }
    void u64(uint64_t v) { lane(0); lane(0); lane(0); lane(vf_bswap(v)); }
    void label(const char* text) {                                // append_message of fewer than 32 bytes: left-padded with zeros
        uint8_t w[32] = {0};
        const size_t len = std::strlen(text);
        std::memcpy(w + 32 - len, text, len);
        word(w);
    }
    void point(const Affine& p) { element(Fq::from_mont(p.x)); element(Fq::from_mont(p.y)); }
};

int vf_key_check(const uzk_vk_desc* d) {
    if (d->n_pi > UZK_VERIFY_MAX_PI) { set_error("uzk_vk_create: %u public inputs (at most %d)", d->n_pi, UZK_VERIFY_MAX_PI); return UZK_ERR_PARAMETER; }
    if (d->cs_size < 2 || (d->cs_size & (d->cs_size - 1)) != 0 || d->cs_size > (1u << 28)) {
        set_error("uzk_vk_create: cs_size %u is not a power of two in 2 .. 2^28", d->cs_size);
        return UZK_ERR_PARAMETER;
    }
    if (d->transcript_prefix_len > 256 || d->transcript_prefix_len % 8 != 0) {
        set_error("uzk_vk_create: a transcript prefix of %u bytes (at most 256, a multiple of 8: the transcript holds 32-byte slots)", d->transcript_prefix_len);
        return UZK_ERR_PARAMETER;
    }
    if (d->transcript_prefix_len > 0 && !d->transcript_prefix) { set_error("uzk_vk_create: transcript_prefix is null"); return UZK_ERR_PARAMETER; }
    if (d->n_pi > 0 && (!d->pi_root_powers || !d->pi_lagrange)) { set_error("uzk_vk_create: the constants of %u public inputs are null", d->n_pi); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

static void vf_fixed_bases(const uzk_vk_desc* d, Affine* out) {
    auto put = [&](uint32_t at, const uzk_g1_affine* src, uint32_t count) { std::memcpy(out + at, src, count * sizeof(Affine)); };
    std::memset(out, 0, kVfFixed * sizeof(Affine));
    put(VF_Q, d->cm_q, 9); put(VF_S, d->cm_s, 5); put(VF_QB, &d->cm_qb, 1); put(VF_PRK, d->cm_prk, 4); put(VF_G0, &d->g1_0, 1);
    if (d->shuffle) { put(VF_QECC, &d->cm_q_ecc, 1); put(VF_PK, d->cm_shuffle_public_key, 12); put(VF_GEN, d->cm_shuffle_generator, 12); }
}

int vf_key_create(Ctx& c, const uzk_vk_desc* d, uint64_t* out) {
    const bool shuffle = d->shuffle != 0;
    const VfLayout L = vf_layout(shuffle);
    VfKey k;
    std::memset(&k, 0, sizeof k);
    auto fp = [](const uint64_t* p) { Fp r; std::memcpy(&r, p, sizeof r); return r; };
    for (int j = 0; j < 5; ++j) k.k[j] = fp(d->k[j]);
    k.anemoi_g = fp(d->anemoi_g); k.anemoi_g_inv = fp(d->anemoi_g_inv); k.edwards_a = fp(d->edwards_a); k.root = fp(d->root);
    while ((1u << k.cs_log) < d->cs_size) ++k.cs_log;
    k.n_pi = d->n_pi;
    k.shuffle = shuffle ? 1 : 0;
    // the caller's prefix, then transcript_init_plonk up to the public inputs (plonk/transcript.rs:9-31)
    HostSponge sp;
    for (uint32_t at = 0; at < d->transcript_prefix_len; at += 8) { uint64_t v; std::memcpy(&v, d->transcript_prefix + at, 8); sp.lane(v); }
    sp.label("PLONK");
    sp.u64(d->cs_size);
    sp.element(Fr::modulus());
    Affine bases[kVfFixed];
    vf_fixed_bases(d, bases);
    for (int j = 0; j < 14; ++j) sp.point(bases[VF_Q + j]);        // cm_q (9), cm_s (5)
    sp.element(Fr::from_mont(k.root));
    for (int j = 0; j < 5; ++j) sp.element(Fr::from_mont(k.k[j]));
    std::memcpy(k.sponge, sp.s, sizeof k.sponge);
    std::memcpy(k.tail, sp.buf, sizeof k.tail);
    k.pos = sp.pos;
    {   // init_pcs_batch_eval_transcript (pcs.rs:228-246) up to the point
        HostSponge hdr;
        hdr.label("New PCS-Batch-Eval Protocol");
        hdr.element(Fr::modulus());
        hdr.u64((uint64_t)d->cs_size + 2);
        std::memcpy(k.pcs_hdr, hdr.buf, sizeof k.pcs_hdr);
    }
    // what each challenge absorbs (compute_challenges, verifier.rs:166-222; PolyComScheme::batch)
    auto seg = [&](int h, uint32_t src, int off, uint32_t n) { k.prog[h][k.nseg[h]++] = VfSeg{src, (uint32_t)off, n}; };
    seg(0, VF_SRC_PI, 0, d->n_pi);
    seg(0, VF_SRC_PROOF, 0, shuffle ? 16 : 10);                    // cm_w, cm_wsel
    seg(2, VF_SRC_PROOF, L.cm_z, 2);
    seg(3, VF_SRC_PROOF, L.cm_t, 10);
    seg(4, VF_SRC_PROOF, L.w, 5);
    seg(4, VF_SRC_PROOF, L.s, 4);
    if (shuffle) seg(4, VF_SRC_PROOF, L.wsel, 3);
    seg(4, VF_SRC_PROOF, L.prk3, 2);
    seg(4, VF_SRC_PROOF, L.z_om, 1);
    if (shuffle) seg(4, VF_SRC_PROOF, L.q_ecc, 1);
    seg(4, VF_SRC_PROOF, L.w_om, 3);
    seg(5, VF_SRC_KEY, 0, 3); seg(5, VF_SRC_ZETA, 0, 1);
    seg(6, VF_SRC_KEY, 0, 3); seg(6, VF_SRC_ZETA_OMEGA, 0, 1);

    VfEntry e;
    e.device = c.device; e.cs_size = d->cs_size; e.n_pi = d->n_pi; e.shuffle = k.shuffle;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&e.d_key), sizeof k);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e.d_bases), sizeof bases);
    if (err == hipSuccess && d->n_pi) err = hipMalloc(reinterpret_cast<void**>(&e.d_consts), (size_t)2 * d->n_pi * sizeof(Fp));
    if (err == hipSuccess) err = hipMemcpyAsync(e.d_key, &k, sizeof k, hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess) err = hipMemcpyAsync(e.d_bases, bases, sizeof bases, hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess && d->n_pi) err = hipMemcpyAsync(e.d_consts, d->pi_root_powers, (size_t)d->n_pi * sizeof(Fp), hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess && d->n_pi) err = hipMemcpyAsync(e.d_consts + d->n_pi, d->pi_lagrange, (size_t)d->n_pi * sizeof(Fp), hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c.stream);  // the staging copies are locals
    if (err != hipSuccess) {
        (void)hipGetLastError();
        vf_free(e);
        set_error("uzk_vk_create: %s", hipGetErrorString(err));
        return UZK_ERR_DEVICE;
    }
    *out = g_vf.insert(e);
    return UZK_OK;
}

bool vf_key_known(uint64_t h, uint32_t* cs_size, uint32_t* n_pi, uint32_t* proof_bytes, int* device) {
    VfEntry e;
    if (!vf_lookup(h, &e)) return false;
    if (cs_size) *cs_size = e.cs_size;
    if (n_pi) *n_pi = e.n_pi;
    if (proof_bytes) *proof_bytes = vf_proof_bytes(e.shuffle);
    if (device) *device = e.device;
    return true;
}

// The caller makes sure no fold over this key is still running.
int vf_key_release(uint64_t h) {
    VfEntry e;
    if (!g_vf.take(h, &e)) { set_error("uzk_vk_release: unknown verifier key %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    vf_free(e);
    return UZK_OK;
}

void vf_release_all() { g_vf.drain(vf_free); }

int vf_key_set_public_key(Ctx& c, uint64_t h, const Affine* pk) {
    VfEntry e;
    if (!vf_lookup(h, &e)) { set_error("uzk_vk_set_public_key: unknown verifier key %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    if (!e.shuffle) { set_error("uzk_vk_set_public_key: the key was made without the shuffle members"); return UZK_ERR_PARAMETER; }
    if (e.device != c.device) { set_error("uzk_vk_set_public_key: the key lives on device %d, the calling context on device %d", e.device, c.device); return UZK_ERR_PARAMETER; }
    UZK_HIP(hipMemcpyAsync(e.d_bases + VF_PK, pk, 12 * sizeof(Affine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// Which transcript kernel a fold runs: the spread form unless uzk_tune("verify_transcript", 1) asks for one proof per lane.
// One proof per lane keeps m / 64 waves busy on a chain of a hundred dependent permutations; spread over half waves the same
// batch is m / 2 waves (2048 at UZK_VERIFY_MAX_BATCH, for 1024 SIMDs).  tools/verify_shape.py times both forms.
static bool vf_transcript_spread(const Ctx& c) { return c.tune_verify_transcript != 1; }

// ---- the fold -----------------------------------------------------------------------------------------------------------------
int vf_fold_run(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pi, uint32_t m, const Fp* weights, Jac* left_out, Jac* right_out,
                uint8_t* status_out, Fp* challenges_out) {
    VfEntry e;
    if (!vf_lookup(h, &e)) { set_error("uzk_verify_fold: unknown verifier key %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    if (e.device != c.device) { set_error("uzk_verify_fold: the key lives on device %d, the calling context on device %d", e.device, c.device); return UZK_ERR_PARAMETER; }
    const uint32_t pb = vf_proof_bytes(e.shuffle);
    const size_t n_r = kVfFixed + (size_t)kVfPerProof * m, n_l = (size_t)2 * m;
    WsCarver cv;
    const auto a_proofs = cv.array<uint8_t>((size_t)m * pb);
    const auto a_pi = cv.array<Fp>((size_t)m * e.n_pi), a_rho = cv.array<Fp>(m), a_words = cv.array<Fp>((size_t)m * kVfWords),
               a_chal = cv.array<Fp>((size_t)m * kVfChallenges);
    const auto a_status = cv.array<uint8_t>(m);
    const auto a_prefix = cv.array<Fp>((size_t)m * (e.n_pi + 1)), a_fixed = cv.array<Fp>((size_t)m * kVfFixed);
    const auto a_pts_r = cv.array<Affine>(n_r);
    const auto a_sc_r = cv.array<Fp>(n_r);
    const auto a_pts_l = cv.array<Affine>(n_l);
    const auto a_sc_l = cv.array<Fp>(n_l);
    UZK_TRY(cv.reserve(c.verify_ws));
    uint8_t *d_proofs = cv(a_proofs), *d_status = cv(a_status);
    Fp *d_pi = cv(a_pi), *d_rho = cv(a_rho), *d_words = cv(a_words), *d_chal = cv(a_chal), *d_prefix = cv(a_prefix), *d_fixed = cv(a_fixed);
    Affine *d_pts_r = cv(a_pts_r), *d_pts_l = cv(a_pts_l);
    Fp *d_sc_r = cv(a_sc_r), *d_sc_l = cv(a_sc_l);
    const Fp one = Fr::one();
    UZK_HIP(hipMemcpyAsync(d_proofs, proofs, (size_t)m * pb, hipMemcpyHostToDevice, c.stream));
    if (e.n_pi) UZK_HIP(hipMemcpyAsync(d_pi, pi, (size_t)m * e.n_pi * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_rho, weights ? weights : &one, (size_t)m * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_pts_r, e.d_bases, kVfFixed * sizeof(Affine), hipMemcpyDeviceToDevice, c.stream));
    const unsigned lanes_grid = (m + kVfBlock - 1) / kVfBlock;
    UZK_LAUNCH(c, "verify_decode", vf_decode_kernel, dim3(m), dim3(kVfBlock), 0, c.stream, d_proofs, pb, (int)e.shuffle, d_words, d_pts_r, d_pts_l, d_status);
    if (vf_transcript_spread(c))
        UZK_LAUNCH(c, "verify_transcript_lanes", vf_transcript_lanes_kernel, dim3((m * kVfGroup + kVfBlock - 1) / kVfBlock), dim3(kVfBlock), 0, c.stream, e.d_key,
                   d_proofs, pb, d_pi, d_status, d_chal, m);
    else
        UZK_LAUNCH(c, "verify_transcript", vf_transcript_kernel, dim3(lanes_grid), dim3(kVfBlock), 0, c.stream, e.d_key, d_proofs, pb, d_pi, d_status, d_chal, m);
    UZK_LAUNCH(c, "verify_scalars", vf_scalars_kernel, dim3(lanes_grid), dim3(kVfBlock), 0, c.stream, e.d_key, d_words, d_chal, d_pi, e.d_consts, e.d_consts + e.n_pi,
               d_rho, d_status, d_prefix, d_fixed, d_sc_r, d_sc_l, m);
    UZK_LAUNCH(c, "verify_reduce", vf_reduce_kernel, dim3(kVfFixed), dim3(256), 0, c.stream, d_fixed, m, d_sc_r);
    UZK_HIP(hipMemcpyAsync(status_out, d_status, m, hipMemcpyDeviceToHost, c.stream));
    if (challenges_out) UZK_HIP(hipMemcpyAsync(challenges_out, d_chal, (size_t)m * kVfChallenges * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    if (c.prof_on) UZK_HIP(hipStreamSynchronize(c.stream));        // so that the two host sections below time the MSMs alone
    int rc;
    {
        HostScope hs(c, "host_verify_msm_r");
        rc = msm_run(c, d_pts_r, ScalarView::dense(d_sc_r, n_r), n_r, 1, right_out, 0, 0, 0);
    }
    if (rc == UZK_OK) {
        HostScope hs(c, "host_verify_msm_l");
        rc = msm_run(c, d_pts_l, ScalarView::dense(d_sc_l, n_l), n_l, 1, left_out, 0, 0, 0);
    }
    // also on failure: the copies into status_out / challenges_out are queued on this stream and must not outlive the call
    const hipError_t se = hipStreamSynchronize(c.stream);
    UZK_TRY(rc);
    UZK_HIP(se);
    return UZK_OK;
}

int vf_keccak_test(Ctx& c, const uint8_t* msgs, const uint64_t* offsets, uint32_t count, uint8_t* out) {
    const size_t total = offsets[count];
    WsCarver cv;
    const auto a_msg = cv.array<uint8_t>(total + 8);
    const auto a_off = cv.array<uint64_t>((size_t)(count + 1));
    const auto a_out = cv.array<uint8_t>((size_t)count * 32);
    UZK_TRY(cv.reserve(c.verify_ws));
    uint8_t *d_msg = cv(a_msg), *d_out = cv(a_out);
    uint64_t* d_off = cv(a_off);
    if (total) UZK_HIP(hipMemcpyAsync(d_msg, msgs, total, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_off, offsets, a_off.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, "verify_keccak_test", vf_keccak_kernel, dim3((count + kVfBlock - 1) / kVfBlock), dim3(kVfBlock), 0, c.stream, d_msg, d_off, count,
               d_out);
    UZK_HIP(hipMemcpyAsync(out, d_out, a_out.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

}  // namespace uzk
