// Host-side BN254 G2 arithmetic: Fq2 = Fq[u] / (u^2 + 1) over host_ec64.hpp's 4 x 64-bit F, Jacobian points over it.  Used by the
// Horner combination of the G2 MSM's window sums, uzk_g2_fold and uzk_g2_to_affine.  Same bytes as the wire (c0 then c1, Montgomery
// words), so values move by memcpy.  Host code only.
#pragma once
#include "g2_29.hpp"
#include "host_ec64.hpp"
#include "host_math.hpp"

namespace uzk {
namespace h64 {

struct F2 {
    F a, b;
};
inline F2 f2_from(const Fq2w& w) { return F2{from_fp(w.c0), from_fp(w.c1)}; }
inline Fq2w f2_to(const F2& x) { Fq2w w; w.c0 = to_fp(x.a); w.c1 = to_fp(x.b); return w; }
inline F2 f2_zero() { return F2{zero(), zero()}; }
inline F2 f2_one() { return F2{from_fp(Fq::one()), zero()}; }
inline bool is_zero(const F2& x) { return is_zero(x.a) && is_zero(x.b); }
inline F2 add(const F2& x, const F2& y) { return F2{add(x.a, y.a), add(x.b, y.b)}; }
inline F2 sub(const F2& x, const F2& y) { return F2{sub(x.a, y.a), sub(x.b, y.b)}; }
inline F2 dbl(const F2& x) { return add(x, x); }
// Karatsuba: three products
inline F2 mul(const F2& x, const F2& y) {
    const F t0 = mul(x.a, y.a), t1 = mul(x.b, y.b);
    const F t2 = mul(add(x.a, x.b), add(y.a, y.b));
    return F2{sub(t0, t1), sub(sub(t2, t0), t1)};
}
inline F2 sqr(const F2& x) {
    const F t = mul(x.a, x.b);
    return F2{mul(add(x.a, x.b), sub(x.a, x.b)), add(t, t)};
}
// 1 / (a + b u) = (a - b u) / (a^2 + b^2)
inline F2 inv(const F2& x) {
    const F n = add(sqr(x.a), sqr(x.b));
    const F ni = from_fp(fq_inv(to_fp(n)));
    return F2{mul(x.a, ni), sub(zero(), mul(x.b, ni))};
}

struct J2 {         // Jacobian; infinity <=> Z == 0
    F2 x, y, z;
};
inline J2 j2_inf() { return J2{f2_one(), f2_one(), f2_zero()}; }
inline J2 j2_from(const G2Jac& p) { return J2{f2_from(p.x), f2_from(p.y), f2_from(p.z)}; }
inline G2Jac j2_to(const J2& p) {
    const J2 q = is_zero(p.z) ? j2_inf() : p;
    G2Jac r;
    r.x = f2_to(q.x); r.y = f2_to(q.y); r.z = f2_to(q.z);
    return r;
}
inline J2 j2_from_affine(const G2Affine& p) {
    const F2 y = f2_from(p.y);
    if (is_zero(y)) return j2_inf();
    return J2{f2_from(p.x), y, f2_one()};
}
// (X ZZ, Y ZZZ, ZZ) is a Jacobian representative of the XYZZ point
inline J2 j2_from_xyzz(const G2XYZZ& p) {
    const F2 zz = f2_from(p.zz);
    if (is_zero(zz)) return j2_inf();
    return J2{mul(f2_from(p.x), zz), mul(f2_from(p.y), f2_from(p.zzz)), zz};
}
// dbl-2009-l (a = 0); infinity stays infinity
inline J2 j2_dbl(const J2& p) {
    const F2 A = sqr(p.x), B = sqr(p.y), C = sqr(B);
    const F2 D = dbl(sub(sub(sqr(add(p.x, B)), A), C));
    const F2 E = add(dbl(A), A), Fv = sqr(E);
    J2 r;
    r.x = sub(Fv, dbl(D));
    r.y = sub(mul(E, sub(D, r.x)), dbl(dbl(dbl(C))));
    r.z = dbl(mul(p.y, p.z));
    return r;
}
// add-2007-bl, complete by branches
inline J2 j2_add(const J2& p, const J2& q) {
    if (is_zero(p.z)) return q;
    if (is_zero(q.z)) return p;
    const F2 Z1Z1 = sqr(p.z), Z2Z2 = sqr(q.z);
    const F2 U1 = mul(p.x, Z2Z2), U2 = mul(q.x, Z1Z1);
    const F2 S1 = mul(mul(p.y, q.z), Z2Z2), S2 = mul(mul(q.y, p.z), Z1Z1);
    const F2 H = sub(U2, U1), Rh = sub(S2, S1);
    if (is_zero(H)) return is_zero(Rh) ? j2_dbl(p) : j2_inf();
    const F2 I = sqr(dbl(H)), Jv = mul(H, I), r = dbl(Rh), V = mul(U1, I);
    J2 o;
    o.x = sub(sub(sqr(r), Jv), dbl(V));
    o.y = sub(mul(r, sub(V, o.x)), dbl(mul(S1, Jv)));
    o.z = mul(sub(sub(sqr(add(p.z, q.z)), Z1Z1), Z2Z2), H);
    return o;
}
inline G2Affine j2_to_affine(const J2& p) {
    G2Affine r;
    if (is_zero(p.z)) { std::memset(&r, 0, sizeof r); return r; }
    const F2 zi = inv(p.z), zi2 = sqr(zi);
    r.x = f2_to(mul(p.x, zi2));
    r.y = f2_to(mul(p.y, mul(zi2, zi)));
    return r;
}

}  // namespace h64
}  // namespace uzk
