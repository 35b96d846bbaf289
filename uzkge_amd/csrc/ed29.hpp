// Baby Jubjub (ark_ed_on_bn254): the twisted Edwards curve  x^2 + y^2 = 1 + d x^2 y^2  over BN254's scalar field, a = 1,
// d = 168696 / 168700 -- the curve zshuffle's cards and keys live on.  d is a non-square, so the unified addition law is COMPLETE:
// one formula serves addition, doubling, the identity (0, 1) and the points of order 2, 4 and 8; there is no exceptional branch.
//
// Coordinates are extended (X : Y : Z : T), x = X / Z, y = Y / Z, T = X Y / Z (Hisil-Wong-Carter-Dawson 2008, the unified law):
//     A = X1 X2   B = Y1 Y2   C = d T1 T2   D = Z1 Z2   E = (X1 + Y1)(X2 + Y2) - A - B   F = D - C   G = D + C   H = B - A
//     X3 = E F    Y3 = G H    T3 = E H      Z3 = F G                                       (ten products, three carry steps)
// on the typed lazy limbs of lz29.hpp in 2^261-form: every coordinate is Lz<Fr29, 1, 2> (normalized limbs, value < 2 M) between
// additions, and the compiler checks each product's limb and value contract (tools/lz29_inventory.py lists the instantiations).
// Z is never 0 on points of the curve.  Wire form: x then y, each the canonical Montgomery words of Fr (radix 2^256) -- the element
// encoding of the Groth16 reveal proof's public signals.
//
// The scalar side: the prime subgroup has order L (251 bits, 8 L = #E); a Chaum-Pedersen challenge is a Keccak digest mod L and a
// response is omega + c sk mod L.  That arithmetic is plain C++ on eight 32-bit words (one reduction and one multiply-add per proof).
#pragma once
#include "keccak.hpp"
#include "lz29.hpp"

namespace uzk {

struct EdAffine {          // wire
    Fp x, y;
};

// ---- integers of 256 bits, little-endian 32-bit words (Fp is only the container here: nothing is in Montgomery form) ---------------
UZK_HD Fp ed_words(const uint32_t (&w)[8]) { Fp r; for (int i = 0; i < 8; ++i) r.v[i] = w[i]; return r; }
UZK_HD bool u256_geq(const Fp& a, const Fp& b) {
    uint64_t br = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)a.v[i] - b.v[i] - br; br = (t >> 32) & 1; }
    return br == 0;
}
UZK_HD Fp u256_sub(const Fp& a, const Fp& b) {
    Fp r;
    uint64_t br = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)a.v[i] - b.v[i] - br; r.v[i] = (uint32_t)t; br = (t >> 32) & 1; }
    return r;
}
UZK_HD Fp u256_add(const Fp& a, const Fp& b) {       // the callers keep the sum below 2^256
    Fp r;
    uint64_t c = 0;
    for (int i = 0; i < 8; ++i) { c += (uint64_t)a.v[i] + b.v[i]; r.v[i] = (uint32_t)c; c >>= 32; }
    return r;
}
UZK_HD Fp u256_shl(const Fp& a, int s) {              // 0 <= s < 32, the caller keeps the result below 2^256
    Fp r;
    for (int i = 7; i > 0; --i) r.v[i] = s ? (a.v[i] << s) | (a.v[i - 1] >> (32 - s)) : a.v[i];
    r.v[0] = a.v[0] << s;
    return r;
}
UZK_HD bool ed_coord_canonical(const Fp& a) { return !u256_geq(a, Field<FrCfg>::modulus()); }

// the order of the prime subgroup
UZK_HD Fp ed_order() {
    const uint32_t l[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
    return ed_words(l);
}
// any 256-bit integer mod L: floor(2^256 / L) = 42 < 64 and 32 L < 2^256, so six conditional subtractions of L 2^k do it
UZK_HD Fp ed_mod_order(Fp v) {
    const Fp l = ed_order();
    for (int k = 5; k >= 0; --k) {
        const Fp t = u256_shl(l, k);
        if (u256_geq(v, t)) v = u256_sub(v, t);
    }
    return v;
}
// (w + c s) mod L for w, s, c below L: double-and-add over the 251 bits of c, every intermediate below 2 L < 2^252
UZK_HD Fp ed_muladd_order(const Fp& w, const Fp& c, const Fp& s) {
    const Fp l = ed_order();
    Fp acc;
    for (int i = 0; i < 8; ++i) acc.v[i] = 0;
    for (int i = 250; i >= 0; --i) {
        acc = u256_add(acc, acc);
        if (u256_geq(acc, l)) acc = u256_sub(acc, l);
        if ((c.v[i >> 5] >> (i & 31)) & 1) {
            acc = u256_add(acc, s);
            if (u256_geq(acc, l)) acc = u256_sub(acc, l);
        }
    }
    acc = u256_add(acc, w);
    if (u256_geq(acc, l)) acc = u256_sub(acc, l);
    return acc;
}

// the generator (EdOnBN254.sol generator(), ark_ed_on_bn254's GENERATOR) and d, Montgomery words
UZK_HD EdAffine ed_generator() {
    const uint32_t gx[8] = {0x1c922693u, 0xd593702cu, 0x4e950979u, 0x3ee58c70u, 0x12c11053u, 0x5bf3ba64u, 0x5c2ca5bfu, 0x06871f85u};
    const uint32_t gy[8] = {0x0866238bu, 0x8dc402f8u, 0x8cbc4f56u, 0x81ec0115u, 0x79b88518u, 0xdb2d6838u, 0xaa94dda4u, 0x23790403u};
    EdAffine g;
    g.x = ed_words(gx); g.y = ed_words(gy);
    return g;
}
UZK_HD Fp ed_d_wire() {
    const uint32_t d[8] = {0x9fb08e74u, 0xe7a66d1du, 0xe17629dcu, 0xd775bbd5u, 0x286ef1e7u, 0x70ccd097u, 0x398fdf98u, 0x00045809u};
    return ed_words(d);
}

// ---- the Chaum-Pedersen transcript of a DL proof -----------------------------------------------------------------------------------
// Keccak-256 of 448 bytes: pad32(label), pad32("DL"), then x and y of g, h, u, v, a, b as 32-byte big-endian words -- the parameters
// (g, h), the statement (u, v) and the commitments of uzkge/src/chaum_pedersen/dl.rs (Transcript::new + its appends;
// utils/transcript.rs left-pads short messages with zeros).  A reveal is g = e1, h = G, u = reveal, v = pk under "Revealing"; a mask is
// g = G, h = pk, u = e1, v = e2 - card under "Masking".  w: the twelve coordinates as PLAIN canonical integers.  Returns the digest
// read as a big-endian integer, not reduced.
struct CpLabel {
    uint64_t lane2, lane3;             // bytes 16 .. 31 of the first word as two little-endian sponge lanes (labels of up to 16 bytes)
};
// "Revealing" = 52 65 76 65 61 6c 69 6e 67: the last nine bytes of the first word
UZK_HD CpLabel cp_label_revealing() { return CpLabel{0x52ull << 56, 0x676e696c61657665ull}; }
// "Masking" = 4d 61 73 6b 69 6e 67: the last seven
UZK_HD CpLabel cp_label_masking() { return CpLabel{0, 0x676e696b73614d00ull}; }
UZK_HD Fp cp_transcript_digest(const Fp (&w)[12], const CpLabel label = cp_label_revealing()) {
    uint64_t lanes[56];
    for (int i = 0; i < 8; ++i) lanes[i] = 0;
    lanes[2] = label.lane2;
    lanes[3] = label.lane3;
    lanes[7] = 0x4c44ull << 48;                                      // "DL" = 44 4c: the last two bytes of the second word
#pragma unroll
    for (int j = 0; j < 12; ++j) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint64_t chunk = ((uint64_t)w[j].v[7 - 2 * t] << 32) | w[j].v[6 - 2 * t];   // most significant first
            lanes[8 + 4 * j + t] = __builtin_bswap64(chunk);
        }
    }
    uint64_t st[25];
    for (int i = 0; i < 25; ++i) st[i] = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {                                   // three full blocks of the 136-byte rate
#pragma unroll
        for (int i = 0; i < 17; ++i) st[i] ^= lanes[17 * b + i];
        vf_keccak_f(st);
    }
    for (int i = 0; i < 5; ++i) st[i] ^= lanes[51 + i];             // 40 bytes, then the padding 01 .. 80
    st[5] ^= 0x01ull;
    st[16] ^= 0x80ull << 56;
    vf_keccak_f(st);
    Fp r;
    for (int t = 0; t < 4; ++t) {
        const uint64_t chunk = __builtin_bswap64(st[t]);
        r.v[7 - 2 * t] = (uint32_t)(chunk >> 32);
        r.v[6 - 2 * t] = (uint32_t)chunk;
    }
    return r;
}

#if defined(__HIP_DEVICE_COMPILE__)

namespace ed {
using Z = LzOps<Fr29>;
using C = Lz<Fr29, 1, 2>;          // a coordinate between additions

struct P {
    C x, y, z, t;
};

__device__ __forceinline__ C one() { return Z::relax<1, 2>(Z::one()); }
__device__ __forceinline__ C zero() { return Z::relax<1, 2>(Z::zero()); }
// a canonical wire element in the loop-carried form: re-limbed (value < 32 M), then one product by 1
__device__ __forceinline__ C ld(const Fp& w) { return Z::mul(Z::ld(w), Z::one()); }
// -a in the loop-carried form
__device__ __forceinline__ C neg(const C& a) { return Z::mul(Z::sub(Z::zero(), a), Z::one()); }
template <int K, int V>
__device__ __forceinline__ bool is_zero(const Lz<Fr29, K, V>& a) { return Fr::is_zero(Z::canon(a)); }

__device__ __forceinline__ P identity() {
    P r;
    r.x = zero(); r.y = one(); r.z = one(); r.t = zero();
    return r;
}
__device__ __forceinline__ P from_affine(const EdAffine& a) {
    P r;
    r.x = ld(a.x); r.y = ld(a.y); r.z = one(); r.t = Z::mul(r.x, r.y);
    return r;
}
__device__ __forceinline__ P neg(const P& p) {
    P r;
    r.x = neg(p.x); r.y = p.y; r.z = p.z; r.t = neg(p.t);
    return r;
}
// the unified, complete addition: also the doubling (p + p) and every case with the identity or a point of small order
__device__ __forceinline__ P add(const P& p, const P& q) {
    const auto a = Z::mul(p.x, q.x);
    const auto b = Z::mul(p.y, q.y);
    const auto c = Z::mul(Z::mul(p.t, q.t), Z::ld(ed_d_wire()));
    const auto d = Z::mul(p.z, q.z);
    const auto s = Z::mul(Z::add(p.x, p.y), Z::add(q.x, q.y));
    const auto e = Z::norm(Z::sub(s, Z::add(a, b)));
    const auto f = Z::norm(Z::sub(d, c));
    const auto g = Z::add(d, c);
    const auto h = Z::norm(Z::sub(b, a));
    P r;
    r.x = Z::mul(e, f); r.y = Z::mul(g, h); r.t = Z::mul(e, h); r.z = Z::mul(f, g);
    return r;
}
__device__ __forceinline__ bool is_identity(const P& p) { return is_zero(p.x) && is_zero(Z::sub(p.y, p.z)); }
// p == the affine point (ax, ay), compared without an inversion: X = ax Z and Y = ay Z
__device__ __forceinline__ bool eq_affine(const P& p, const C& ax, const C& ay) {
    return is_zero(Z::sub(p.x, Z::mul(ax, p.z))) && is_zero(Z::sub(p.y, Z::mul(ay, p.z)));
}
// x^2 + y^2 = 1 + d x^2 y^2
__device__ __forceinline__ bool on_curve(const C& x, const C& y) {
    const auto xx = Z::sqr(x), yy = Z::sqr(y);
    const auto rhs = Z::add(Z::one(), Z::mul(Z::mul(xx, yy), Z::ld(ed_d_wire())));
    return is_zero(Z::sub(Z::add(xx, yy), rhs));
}
// k p for a 256-bit integer k: double-and-add from the top bit, one control flow per wave when the lanes share k
__device__ __forceinline__ P mul(const P& base, const Fp& k) {
    P acc = identity();
#pragma unroll 1
    for (int i = 255; i >= 0; --i) {
        acc = add(acc, acc);
        if ((k.v[i >> 5] >> (i & 31)) & 1) acc = add(acc, base);
    }
    return acc;
}
// r p + c q' for q' given through the table t1 = p, t2 = q', t3 = p + q': Straus / Shamir over the joint bits, one doubling chain
__device__ __forceinline__ P mul2(const P& t1, const P& t2, const P& t3, const Fp& r, const Fp& c) {
    P acc = identity();
#pragma unroll 1
    for (int i = 255; i >= 0; --i) {
        acc = add(acc, acc);
        const uint32_t sel = ((r.v[i >> 5] >> (i & 31)) & 1) | (((c.v[i >> 5] >> (i & 31)) & 1) << 1);
        if (sel) acc = add(acc, sel == 1 ? t1 : sel == 2 ? t2 : t3);
    }
    return acc;
}
// a^(q - 2); 0 for a = 0 (Z of a point of the curve is never 0)
__device__ __forceinline__ C inv(const C& a) {
    Fp e = Fr::modulus();
    e.v[0] -= 2;                                                   // the low word of q ends in ...0001: no borrow
    C acc = one();
#pragma unroll 1
    for (int i = 253; i >= 0; --i) {
        acc = Z::sqr(acc);
        if ((e.v[i >> 5] >> (i & 31)) & 1) acc = Z::mul(acc, a);
    }
    return acc;
}
__device__ __forceinline__ EdAffine to_affine(const P& p) {
    const C zi = inv(p.z);
    EdAffine r;
    r.x = Z::to_wire(Z::mul(p.x, zi)); r.y = Z::to_wire(Z::mul(p.y, zi));
    return r;
}
// 0 on the curve and in the prime subgroup; 1 a coordinate word >= q; 2 off the curve; 3 [L] P != identity
__device__ __forceinline__ uint32_t classify(const EdAffine& a) {
    if (!ed_coord_canonical(a.x) || !ed_coord_canonical(a.y)) return 1;
    const P p = from_affine(a);
    if (!on_curve(p.x, p.y)) return 2;
    return is_identity(mul(p, ed_order())) ? 0 : 3;
}
}  // namespace ed

#endif   // __HIP_DEVICE_COMPILE__

}  // namespace uzk
