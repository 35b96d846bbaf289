// The small tools that run inside ONE lane, on the wire's 8 x 32-bit words, and that every module around the MSMs needs: a power with a
// fixed exponent (inversion, square root), a coordinate against its modulus, the two curve equations, a 32-byte big-endian word, a G1
// scalar multiplication, the affine maps with the inversion in the lane, [r] Q = O on G2, and the walk back of Montgomery's trick.
// None of it is on a hot path: a lane spends 254 squarings where these are called, once per call or per run of points.  Each is
// defined here and nowhere else.  Infinity is all zeros in affine form, ZZ == 0 / Z == 0 otherwise.
//
// Everything but the G2 part compiles for the host too (plain C++: tests/cpp/lane_tools_host.cpp).
#pragma once
#include "ec.hpp"
#if defined(__HIPCC__)
#include "g2_29.hpp"
#define UZK_LANE __host__ __device__ inline        // the compiler decides about inlining: these hold a 254-step loop
#else
#define UZK_LANE inline
#endif

namespace uzk {

// ---- a^e for a 254-bit exponent in canonical little-endian words, most significant bit first ------------------------------------------
template <class F>
UZK_HD Fp wire_pow(const Fp& a, const uint32_t (&e)[8]) {
    Fp acc = F::one();
#pragma unroll 1
    for (int i = 253; i >= 0; --i) {
        acc = F::sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = F::mul(acc, a);
    }
    return acc;
}
// The exponents are derived from the moduli at compile time, so a kernel reads them as constants (a table filled in the lane is
// indexed by the loop and lands in the LDS: 2 KiB a wave and a slower build of a window table).
struct WireExp { uint32_t w[8]; };
template <class C>
constexpr WireExp exponent_of_inverse() {                         // M - 2
    WireExp e{};
    for (int i = 0; i < 8; ++i) e.w[i] = C::M[i];
    e.w[0] -= 2;                                                   // both moduli are odd and their low words are above 2: no borrow
    return e;
}
constexpr WireExp exponent_of_fq_sqrt() {                         // (p + 1) / 4
    WireExp e{};
    for (int i = 0; i < 8; ++i) e.w[i] = FqCfg::M[i];
    e.w[0] += 1;                                                   // the low word of p ends in ...fd47: no carry
    for (int i = 0; i < 8; ++i) e.w[i] = (e.w[i] >> 2) | (i < 7 ? e.w[i + 1] << 30 : 0u);
    return e;
}
UZK_LANE Fp fq_inv_lane(const Fp& a) {                            // a^(p - 2); 0 -> 0
    constexpr WireExp e = exponent_of_inverse<FqCfg>();
    return wire_pow<Fq>(a, e.w);
}
UZK_LANE Fp fr_inv_lane(const Fp& a) {                            // a^(r - 2); 0 -> 0
    constexpr WireExp e = exponent_of_inverse<FrCfg>();
    return wire_pow<Fr>(a, e.w);
}
// the square root of a where it has one (p = 3 mod 4); the caller squares it to find out
UZK_LANE Fp fq_sqrt_candidate(const Fp& a) {
    constexpr WireExp e = exponent_of_fq_sqrt();
    return wire_pow<Fq>(a, e.w);
}

// ---- field and curve checks ---------------------------------------------------------------------------------------------------------
template <class C>
UZK_HD bool below_modulus(const Fp& a) {
    uint64_t br = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)a.v[i] - C::M[i] - br; br = (t >> 32) & 1; }
    return br != 0;
}
UZK_HD Fp g1_b() { const Fp one = Fq::one(); return Fq::add(Fq::add(one, one), one); }              // the curve's constant 3
UZK_HD Fp g1_rhs(const Fp& x, const Fp& b) { return Fq::add(Fq::mul(Fq::sqr(x), x), b); }           // x^3 + b
UZK_HD bool g1_on_curve(const Affine& p) { const Fp b = g1_b(); return Fq::eq(Fq::sqr(p.y), g1_rhs(p.x, b)); }

// ---- 32 big-endian bytes to and from canonical words; p is 4-byte aligned, Montgomery form is the caller's business ---------------------
UZK_HD Fp load_be32(const uint8_t* p) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p);
    Fp v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.v[j] = __builtin_bswap32(src[7 - j]);
    return v;
}
UZK_HD void store_be32(uint8_t* p, const Fp& v) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[7 - j] = __builtin_bswap32(v.v[j]);
}

// ---- s * base over the 254 bits of a canonical s (not in Montgomery form), base affine or XYZZ ------------------------------------------
UZK_HD void g1_add_base(XYZZ& acc, const Affine& base) { xyzz_madd(acc, base, false); }
UZK_HD void g1_add_base(XYZZ& acc, const XYZZ& base) { xyzz_add(acc, base); }
template <class Base>
UZK_HD XYZZ g1_mul_lane(const Base& base, const Fp& s) {
    XYZZ acc = xyzz_inf();
#pragma unroll 1
    for (int k = 253; k >= 0; --k) {
        acc = xyzz_dbl(acc);
        if ((s.v[k >> 5] >> (k & 31)) & 1) g1_add_base(acc, base);
    }
    return acc;
}

// ---- canonical affine points, one inversion each; the caller negates ------------------------------------------------------------------
UZK_LANE Affine xyzz_to_affine_lane(const XYZZ& p) {
    Affine r;
    r.x = Fq::zero(); r.y = r.x;
    if (!xyzz_is_inf(p)) {
        const Fp inv = fq_inv_lane(Fq::mul(p.zz, p.zzz));
        r.x = Fq::mul(p.x, Fq::mul(inv, p.zzz));                   // X / ZZ
        r.y = Fq::mul(p.y, Fq::mul(inv, p.zz));                    // Y / ZZZ
    }
    return r;
}
UZK_LANE Affine jac_to_affine_lane(const Jac& p) {
    Affine r;
    r.x = Fq::zero(); r.y = r.x;
    if (!Fq::is_zero(p.z)) {
        const Fp zi = fq_inv_lane(p.z), zi2 = Fq::sqr(zi);
        r.x = Fq::mul(p.x, zi2);                                   // X / Z^2
        r.y = Fq::mul(p.y, Fq::mul(zi2, zi));                      // Y / Z^3
    }
    return r;
}

// ---- the walk back of Montgomery's trick ------------------------------------------------------------------------------------------------
// Entries lo .. hi - 1, `stride` apart: out holds the Jacobian-like (X ZZ, Y ZZZ), tmp_z its Z = ZZ, tmp_p the product of the Z before
// it; prod is the product of them all (an infinity was entered as (0, 0) with Z = 1).  One inversion, then five products per entry
// going down: out becomes (X / Z^2, Y / Z^3).
template <class I>
UZK_HD void normalise_run(Affine* out, const Fp* tmp_z, const Fp* tmp_p, I lo, I hi, const Fp& prod, size_t stride = 1) {
    Fp inv = fq_inv_lane(prod);
    for (I j = hi; j-- > lo;) {
        const size_t at = (size_t)j * stride;
        const Fp zi = Fq::mul(inv, tmp_p[at]);                     // 1 / z_j
        inv = Fq::mul(inv, tmp_z[at]);
        const Fp zi2 = Fq::sqr(zi);
        Affine xy = out[at];
        xy.x = Fq::mul(xy.x, zi2);
        xy.y = Fq::mul(xy.y, Fq::mul(zi2, zi));
        out[at] = xy;
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
// ---- G2: the twist's equation and the subgroup, on the lazy limbs of g2_29.hpp ---------------------------------------------------------
// the twist's constant 3 / (9 + u) = (27 / 82, -3 / 82), canonical words
__device__ __forceinline__ Fq2w g2_twist_b() {
    Fq2w b;
    const uint32_t c0[8] = {0x24a138e5u, 0x3267e6dcu, 0x59dbefa3u, 0xb5b4c5e5u, 0x1be06ac3u, 0x81be1899u, 0xceb8aaaeu, 0x2b149d40u};
    const uint32_t c1[8] = {0x85c315d2u, 0xe4a2bd06u, 0xe52d1852u, 0xa74fa084u, 0xeed8fdf4u, 0xcd2cafadu, 0x3af0fed4u, 0x009713b0u};
    Fp a0, a1;
#pragma unroll
    for (int i = 0; i < 8; ++i) { a0.v[i] = c0[i]; a1.v[i] = c1[i]; }
    b.c0 = Fq::to_mont(a0); b.c1 = Fq::to_mont(a1);
    return b;
}
__device__ __forceinline__ bool g2_on_twist(const G2Affine& p) {
    using namespace q2;
    const auto X = ldr(p.x), Y = ldr(p.y);
    const auto rhs = add(mul(sqr(X), X), ldr(g2_twist_b()));
    return is_zero(sub(sqr(Y), rhs));
}
// [r] Q = O: the bits of r are the same for every lane, so a wave runs one control flow
__device__ __forceinline__ bool g2_in_subgroup(const G2P& q) {
    if (q.inf) return true;
    G2P acc = g2p_inf();
#pragma unroll 1
    for (int k = 253; k >= 0; --k) {
        g2p_dbl(acc);
        if ((FrCfg::M[k >> 5] >> (k & 31)) & 1) g2p_add(acc, q);
    }
    return acc.inf;
}
#endif

}  // namespace uzk
