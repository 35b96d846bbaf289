// BN254 G2 (the twist y^2 = x^3 + 3 / (9 + u) over Fq2) on the lazy 29-bit limbs: the bucket accumulator of the G2 MSM and the full
// XYZZ additions of its reductions.  The curve constant appears in no formula (a = 0), so the code is the G1 group law of ec29.hpp /
// ec29l.hpp over q2:: elements; every special case is a branch taken in place (there is no second kernel for degenerate tasks).
//
// Wire forms (canonical Montgomery words, radix 2^256): affine (x, y) with infinity = all zeros ((0, 0) is not on the twist), XYZZ
// (x, y, zz, zzz) with infinity <=> zz = 0.
//
// G2Acc, the accumulator of the mixed addition: X, Y in 2^261-form with values < 16 M, ZZ, ZZZ in 2^266-form with values < 2 M.  A base
// point is used as it arrives (2^256-form, q2::ldp): x2 ZZ and y2 ZZZ then land in 2^261-form by themselves, ZZ PP and ZZZ PPP stay
// in 2^266-form -- no conversion product per loaded point (the arrangement of ec29.hpp).  The bounds are the fixed point of the
// formulas below (X3 < 15 M, Y3 < 7 M, ZZ3, ZZZ3 < 2 M); the types check them.
// G2P, a full XYZZ point: all four in 2^261-form, values < 16 M; loaded from the wire with one reduction per coordinate.
#pragma once
#include "fq2_29.hpp"

namespace uzk {

struct G2Affine { Fq2w x, y; };
struct G2Jac { Fq2w x, y, z; };
struct G2XYZZ { Fq2w x, y, zz, zzz; };

#if defined(__HIP_DEVICE_COMPILE__)

namespace g2 {
using namespace q2;
using CoA = E2<1, 16>;      // X, Y of the accumulator; every coordinate of a G2P
using CoZ = E2<1, 2>;       // ZZ, ZZZ of the accumulator
}

struct G2Acc {
    g2::CoA x, y;
    g2::CoZ zz, zzz;
    bool inf;
};
struct G2P {
    g2::CoA x, y, zz, zzz;
    bool inf;
};

__device__ __forceinline__ bool fq2w_is_zero(const Fq2w& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.c0.v[i] | a.c1.v[i];
    return o == 0;
}
__device__ __forceinline__ Fq2w fq2w_neg(const Fq2w& a) { Fq2w r; r.c0 = Fq::neg(a.c0); r.c1 = Fq::neg(a.c1); return r; }
__device__ __forceinline__ Fq2w fq2w_zero() { Fq2w r; r.c0 = Fq::zero(); r.c1 = Fq::zero(); return r; }

__device__ __forceinline__ G2Acc g2acc_inf() {
    G2Acc a;
    a.x = g2::relax<1, 16>(g2::zero()); a.y = a.x;
    a.zz = g2::relax<1, 2>(g2::zero()); a.zzz = a.zz;
    a.inf = true;
    return a;
}
// affine point (finite) -> accumulator: ZZ = ZZZ = 1 in 2^266-form
__device__ __forceinline__ void g2acc_set(G2Acc& a, const Fq2w& x, const Fq2w& y) {
    using namespace g2;
    a.x = relax<1, 16>(ldr(x));
    a.y = relax<1, 16>(ldr(y));
    a.zz.a.v = F::constant(Fq29Cfg::R266); a.zz.b.v = F::zero();
    a.zzz = a.zz;
    a.inf = false;
}
// 2 (x, y) for a finite affine point (mdbl-2008-s) -> accumulator forms
__device__ __forceinline__ void g2acc_set_double(G2Acc& a, const Fq2w& x, const Fq2w& y) {
    using namespace g2;
    const auto X = ldr(x), Y = ldr(y);
    const auto U = norm(add(Y, Y));
    const auto V = sqr(U);
    const auto W = mul(U, V);
    const auto S = mul(X, V);
    const auto X2 = sqr(X);
    const auto M3 = norm(add(add(X2, X2), X2));
    const auto X3 = norm(sub(sqr(M3), add(S, S)));
    const auto D = norm(sub(S, X3));
    const auto Y3 = sub(mul(M3, D), mul(W, Y));
    a.x = fit<16>(X3);
    a.y = fit<16>(Y3);
    a.zz = fit<2>(mul_fq(V, Fq29Cfg::R266));           // V 2^261 -> V 2^266
    a.zzz = fit<2>(mul_fq(W, Fq29Cfg::R266));
    a.inf = false;
}
// acc += p (-p if `negate`), madd-2008-s; complete: accumulator at infinity, p at infinity, p == acc (doubling), p == -acc (infinity)
__device__ __forceinline__ void g2acc_madd(G2Acc& a, const G2Affine& p, bool negate) {
    using namespace g2;
    if (fq2w_is_zero(p.y)) return;                     // infinity is (0, 0); no point of the order-r subgroup has y = 0
    const Fq2w py = negate ? fq2w_neg(p.y) : p.y;
    if (a.inf) { g2acc_set(a, p.x, py); return; }
    const auto U2 = mul(ldp(p.x), a.zz), S2 = mul(ldp(py), a.zzz);
    const auto P = norm(sub(U2, a.x)), R = norm(sub(S2, a.y));
    if (is_zero(P)) {                                  // same x: p = +-acc
        if (is_zero(R)) g2acc_set_double(a, p.x, py);
        else a = g2acc_inf();
        return;
    }
    const auto PP = sqr(P);
    const auto PPP = mul(P, PP), Q = mul(a.x, PP);
    const auto X3 = norm(sub(sqr(R), add(PPP, add(Q, Q))));
    const auto D = norm(sub(Q, X3));
    const auto Y3 = sub(mul(R, D), mul(a.y, PPP));
    a.zz = fit<2>(mul(a.zz, PP));
    a.zzz = fit<2>(mul(a.zzz, PPP));
    a.x = fit<16>(X3);
    a.y = fit<16>(Y3);
}
__device__ __forceinline__ G2XYZZ g2acc_store(const G2Acc& a) {
    using namespace g2;
    G2XYZZ r;
    if (a.inf) { r.x = fq2w_zero(); r.y = r.x; r.zz = r.x; r.zzz = r.x; return r; }
    r.x = to_wire(a.x); r.y = to_wire(a.y);
    r.zz = to_wire_266(a.zz); r.zzz = to_wire_266(a.zzz);
    return r;
}

// ---- full XYZZ points ----
__device__ __forceinline__ G2P g2p_inf() {
    G2P r;
    r.x = g2::relax<1, 16>(g2::zero()); r.y = r.x; r.zz = r.x; r.zzz = r.x;
    r.inf = true;
    return r;
}
__device__ __forceinline__ G2P g2p_load(const G2XYZZ& w) {
    using namespace g2;
    if (fq2w_is_zero(w.zz)) return g2p_inf();
    G2P r;
    r.x = relax<1, 16>(ldr(w.x)); r.y = relax<1, 16>(ldr(w.y)); r.zz = relax<1, 16>(ldr(w.zz)); r.zzz = relax<1, 16>(ldr(w.zzz));
    r.inf = false;
    return r;
}
__device__ __forceinline__ G2P g2p_from_affine(const G2Affine& p) {
    using namespace g2;
    if (fq2w_is_zero(p.y)) return g2p_inf();
    G2P r;
    r.x = relax<1, 16>(ldr(p.x)); r.y = relax<1, 16>(ldr(p.y));
    r.zz.a = Z::template relax<1, 16>(Z::one()); r.zz.b = Z::template relax<1, 16>(Z::zero());
    r.zzz = r.zz;
    r.inf = false;
    return r;
}
__device__ __forceinline__ G2XYZZ g2p_store(const G2P& p) {
    using namespace g2;
    G2XYZZ r;
    if (p.inf) { r.x = fq2w_zero(); r.y = r.x; r.zz = r.x; r.zzz = r.x; return r; }
    r.x = to_wire(p.x); r.y = to_wire(p.y); r.zz = to_wire(p.zz); r.zzz = to_wire(p.zzz);
    return r;
}
// 2 a (dbl-2008-s-1); infinity stays
__device__ __forceinline__ void g2p_dbl(G2P& a) {
    using namespace g2;
    if (a.inf) return;
    const auto U = norm(add(a.y, a.y));
    const auto V = sqr(U);
    const auto W = mul(U, V);
    const auto S = mul(a.x, V);
    const auto X2 = sqr(a.x);
    const auto M3 = norm(add(add(X2, X2), X2));
    const auto X3 = fit<16>(sub(sqr(M3), add(S, S)));
    const auto D = norm(sub(S, X3));
    const auto Y3 = sub(mul(M3, D), mul(W, a.y));
    a.zz = fit<16>(mul(V, a.zz));
    a.zzz = fit<16>(mul(W, a.zzz));
    a.x = X3;
    a.y = fit<16>(Y3);
}
// acc += q (add-2008-s), complete
__device__ __forceinline__ void g2p_add(G2P& acc, const G2P& q) {
    using namespace g2;
    if (q.inf) return;
    if (acc.inf) { acc = q; return; }
    const auto U1 = mul(acc.x, q.zz), U2 = mul(q.x, acc.zz), S1 = mul(acc.y, q.zzz), S2 = mul(q.y, acc.zzz);
    const auto P = norm(sub(U2, U1)), R = norm(sub(S2, S1));
    if (is_zero(P)) {
        if (is_zero(R)) g2p_dbl(acc);
        else acc = g2p_inf();
        return;
    }
    const auto PP = sqr(P);
    const auto PPP = mul(P, PP), Q = mul(U1, PP);
    const auto X3 = fit<16>(sub(sqr(R), add(PPP, add(Q, Q))));
    const auto D = norm(sub(Q, X3));
    const auto Y3 = sub(mul(R, D), mul(S1, PPP));
    acc.zz = fit<16>(mul(mul(acc.zz, q.zz), PP));
    acc.zzz = fit<16>(mul(mul(acc.zzz, q.zzz), PPP));
    acc.x = X3;
    acc.y = fit<16>(Y3);
}
__device__ __forceinline__ G2P g2p_from_acc(const G2Acc& a) { return g2p_load(g2acc_store(a)); }

#endif   // __HIP_DEVICE_COMPILE__

}  // namespace uzk
