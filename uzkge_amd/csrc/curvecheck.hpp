// The point checks that the Groth16 fold (g16verify.hip) and the pairing product (pairing.hip) share: a coordinate against its modulus,
// a G1 point on y^2 = x^3 + 3, a G2 point on the twist y^2 = x^3 + 3 / (9 + u).  Infinity (all zeros) is the caller's case.  And the Fq
// inversion of the affine maps that run in a lane (g16verify.hip, groth16.hip, g2msm.hip).
#pragma once
#include "ec.hpp"
#include "g2_29.hpp"

namespace uzk {

template <class C>
UZK_HD bool gv_below_modulus(const Fp& a) {
    uint64_t br = 0;
    for (int i = 0; i < 8; ++i) { const uint64_t t = (uint64_t)a.v[i] - C::M[i] - br; br = (t >> 32) & 1; }
    return br != 0;
}

UZK_HD bool gv_g1_on_curve(const Affine& p) {
    const Fp one = Fq::one();
    const Fp three = Fq::add(Fq::add(one, one), one);
    return Fq::eq(Fq::sqr(p.y), Fq::add(Fq::mul(Fq::sqr(p.x), p.x), three));
}

__device__ inline Fp gv_fq_inv(const Fp& a) {                     // a^(p - 2)
    Fp e = Fq::modulus();
    e.v[0] -= 2;                                                   // the low word of p ends in ...fd47
    Fp acc = Fq::one();
#pragma unroll 1
    for (int i = 253; i >= 0; --i) {
        acc = Fq::sqr(acc);
        if ((e.v[i >> 5] >> (i & 31)) & 1) acc = Fq::mul(acc, a);
    }
    return acc;
}

#if defined(__HIP_DEVICE_COMPILE__)
// the twist's constant 3 / (9 + u) = (27 / 82, -3 / 82), canonical words
__device__ __forceinline__ Fq2w gv_twist_b() {
    Fq2w b;
    const uint32_t c0[8] = {0x24a138e5u, 0x3267e6dcu, 0x59dbefa3u, 0xb5b4c5e5u, 0x1be06ac3u, 0x81be1899u, 0xceb8aaaeu, 0x2b149d40u};
    const uint32_t c1[8] = {0x85c315d2u, 0xe4a2bd06u, 0xe52d1852u, 0xa74fa084u, 0xeed8fdf4u, 0xcd2cafadu, 0x3af0fed4u, 0x009713b0u};
    Fp a0, a1;
#pragma unroll
    for (int i = 0; i < 8; ++i) { a0.v[i] = c0[i]; a1.v[i] = c1[i]; }
    b.c0 = Fq::to_mont(a0); b.c1 = Fq::to_mont(a1);
    return b;
}
__device__ __forceinline__ bool gv_g2_on_twist(const G2Affine& p) {
    using namespace q2;
    const auto X = ldr(p.x), Y = ldr(p.y);
    const auto rhs = add(mul(sqr(X), X), ldr(gv_twist_b()));
    return is_zero(sub(sqr(Y), rhs));
}
#endif

}  // namespace uzk
