// Fq12 = Fq2[w] / (w^6 - xi), xi = 9 + u, on the lazy 29-bit limbs (fq2_29.hpp), ONE ELEMENT SPREAD OVER A LANE GROUP: lane k of a group
// holds the Fq2 coefficient of w^k (six of the group's eight lanes; the other two run along with writes masked off, so that every
// barrier is reached by every lane).  Wire form: six Fq2 wire elements, the coefficient of w^0 first -- the layout of
// oracle/bn254_pairing.py's Fq12 and of uzk_gt.
//
// A coefficient is an E2<1, 2> (2^261-form, normalized limbs, value < 2 M) between operations: the fixed point of the Fq2 product's
// bound (q2::mul_v(2, 2) = 2).  Sums of products grow lazily and are reduced once per output coefficient (q2::fit<2>).  Only typed
// operations are used: every bound below is checked by the compiler (lz29.hpp), and tools/lz29_inventory.py lists the signatures.
//
// Exchange: the operands of a product are published in the group's block of the LDS and every lane computes ITS coefficient
//     c_k = sum_i a_i b'_(k - i),   b'_j = b_j for j >= 0 and xi b_(j + 6) for j < 0;
// the second operand is published as a table of twelve entries (b_j, then xi b_j), so the wrapped terms cost an address and no
// branch.  The block has two sides: an operation writes the side that the one before it did not read, then one barrier, then it
// reads -- one barrier per operation, and a side is overwritten only after a barrier that every reader of it has passed.
//
//   f12_mul, f12_sqr     6 Fq2 products per lane
//   f12_sparse           the product with l0 + l1 w + l3 w^3 (a line of the Miller loop): 3 per lane
//   f12_conj             the p^6 map, w -> -w (the inverse in the cyclotomic subgroup): no exchange
//   f12_frob<j>          the p^j map, j = 1, 2, 3: conj^j of the coefficient times gamma_j,k = xi^(k (p^j - 1) / 6): no exchange; the
//                        constants are computed by the host at start-up (Fq12Consts, pairing.hip)
//   f12_inv              a^-1 = conj(a) t' t'' / N with t = a conj(a) in Fq6, t' = t^(p^2), t'' = t^(p^4), N = t t' t'' in Fq2: four
//                        products, two Frobenius maps and ONE Fq inversion (Fermat, every lane the same one).  The inverse of 0 is 0.
//   f12_cyc              Granger-Scott's square of an element of the cyclotomic subgroup: 2 per lane
#pragma once
#include "fq2_29.hpp"

namespace uzk {

struct Fq12w {
    Fq2w c[6];
};
// what the kernels need beside their operands; filled by the host (pairing.hip, pairing_consts())
struct Fq12Consts {
    Fq2w gamma[3][6];      // gamma[j - 1][k] = xi^(k (p^j - 1) / 6)
    Fq2w twist_b3;         // 3 b' = 9 / xi, the doubling step's constant
};

#if defined(__HIP_DEVICE_COMPILE__)

namespace q12 {
using q2::E2;
using q2::Z;
using El = E2<1, 2>;
constexpr int kGroup = 8;          // lanes of a group; 6 of them hold a coefficient

struct Sh {
    El a[2][6];
    El b[2][12];
    El keep[3];         // for the caller: values every lane of the group reads now and then (the Miller loop's Q and 3 b')
    Lz<Fq29, 1, 4> base[2];   // and two elements of Fq (xP, -yP)
};
struct Lane {
    Sh* sh;
    int k;              // this lane's coefficient (0 for the two idle lanes: their reads are valid, their writes masked)
    bool act;
    int side;           // the side of the block that was written last
};

__device__ __forceinline__ El el_zero() { return q2::relax<1, 2>(q2::zero()); }
__device__ __forceinline__ El el_one() {
    El r; r.a = Z::relax<1, 2>(Z::one()); r.b = Z::relax<1, 2>(Z::zero()); return r;
}
__device__ __forceinline__ El f12_one(const Lane& L) { return L.k == 0 ? el_one() : el_zero(); }

// (9 + u) x = (9 x0 - x1) + (x0 + 9 x1) u
__device__ __forceinline__ El xi_mul(const El& x) {
    const auto x2 = q2::add(x, x);
    const auto x4 = q2::norm(q2::add(x2, x2));
    const auto x9 = q2::add(q2::add(x4, x4), x);          // K = 3, V = 18
    E2<6, 21> r;
    r.a = Z::sub(x9.a, x.b);
    r.b = Z::relax<6, 21>(Z::add(x9.b, x.a));
    return q2::fit<2>(r);
}

__device__ __forceinline__ void put_a(const Lane& L, const El& x) {
    if (L.act) L.sh->a[L.side ^ 1][L.k] = x;
}
__device__ __forceinline__ void put_b(const Lane& L, const El& y) {
    if (L.act) {
        L.sh->b[L.side ^ 1][L.k] = y;
        L.sh->b[L.side ^ 1][L.k + 6] = xi_mul(y);
    }
}
// reached by every lane of the workgroup: callers hold no lane back
__device__ __forceinline__ void turn(Lane& L) {
    __syncthreads();
    L.side ^= 1;
}

__device__ __forceinline__ int wrap_ix(int k, int i) { return k >= i ? k - i : k - i + 12; }
// coefficient k of a b, a = a[0 .. 6), b as its table of twelve
__device__ __forceinline__ El mul_coeff(const El* a, const El* tb, int k) {
    const auto m0 = q2::mul(a[0], tb[k]);
    const auto m1 = q2::mul(a[1], tb[wrap_ix(k, 1)]);
    const auto m2 = q2::mul(a[2], tb[wrap_ix(k, 2)]);
    const auto m3 = q2::mul(a[3], tb[wrap_ix(k, 3)]);
    const auto m4 = q2::mul(a[4], tb[wrap_ix(k, 4)]);
    const auto m5 = q2::mul(a[5], tb[wrap_ix(k, 5)]);
    return q2::fit<2>(q2::add(q2::add(q2::add(m0, m1), q2::add(m2, m3)), q2::add(m4, m5)));
}

__device__ __forceinline__ El f12_mul(Lane& L, const El& x, const El& y) {
    put_a(L, x);
    put_b(L, y);
    turn(L);
    return mul_coeff(L.sh->a[L.side], L.sh->b[L.side], L.k);
}
__device__ __forceinline__ El f12_sqr(Lane& L, const El& x) {
    put_b(L, x);
    turn(L);
    return mul_coeff(L.sh->b[L.side], L.sh->b[L.side], L.k);
}
// x (l0 + l1 w + l3 w^3): c_k = x_k l0 + x_(k - 1) l1 + x_(k - 3) l3, the wrapped ones times xi
__device__ __forceinline__ El f12_sparse(Lane& L, const El& x, const El& l0, const El& l1, const El& l3) {
    put_a(L, x);
    turn(L);
    const El* a = L.sh->a[L.side];
    const El t1 = L.k >= 1 ? l1 : xi_mul(l1);
    const El t3 = L.k >= 3 ? l3 : xi_mul(l3);
    const int k1 = L.k >= 1 ? L.k - 1 : L.k + 5, k3 = L.k >= 3 ? L.k - 3 : L.k + 3;
    return q2::fit<2>(q2::add(q2::add(q2::mul(x, l0), q2::mul(a[k1], t1)), q2::mul(a[k3], t3)));
}
__device__ __forceinline__ El f12_conj(const Lane& L, const El& x) {
    const E2<4, 4> r = (L.k & 1) ? q2::neg(x) : q2::relax<4, 4>(x);
    return q2::fit<2>(r);
}
template <int J>
__device__ __forceinline__ El f12_frob(const Lane& L, const El& x, const Fq12Consts* cst) {
    static_assert(J >= 1 && J <= 3, "Frobenius maps p, p^2, p^3");
    const El g = q2::ldr(cst->gamma[J - 1][L.k]);
    if constexpr (J & 1) return q2::fit<2>(q2::mul(q2::norm(q2::conj(x)), g));
    else return q2::fit<2>(q2::mul(x, g));
}

// Granger-Scott: the pairs (a0, a3), (a1, a4), (a2, a5) are three elements x + y s of Fq4 = Fq2[s] / (s^2 - xi);
// with (x + y s)^2 = t + t' s:  a0' = 3 t03 - 2 a0, a3' = 3 t03' + 2 a3, a2' = 3 t14 - 2 a2, a5' = 3 t14' + 2 a5,
// a4' = 3 t25 - 2 a4, a1' = 3 xi t25' + 2 a1.  Lane k squares the pair it needs (x = a_px, px = 0, 2, 1, 0, 2, 1).
__device__ __forceinline__ El f12_cyc(Lane& L, const El& x) {
    put_b(L, x);
    turn(L);
    const El* tb = L.sh->b[L.side];
    const int r3 = L.k >= 3 ? L.k - 3 : L.k;
    const int px = r3 == 0 ? 0 : 3 - r3;
    const bool even = (L.k & 1) == 0;
    const int iv = even ? px : (L.k == 1 ? px + 9 : px + 3);
    const auto p = q2::mul(tb[px], tb[iv]);                       // even: x^2; odd: x y (times xi in lane 1)
    const auto q = q2::mul(tb[px + 9], tb[px + 3]);               // xi y^2 (the odd lanes do not use it)
    const auto x2 = q2::add(x, x);
    const auto s = q2::add(p, q);
    const auto s3 = q2::norm(q2::add(q2::add(s, s), s));          // 3 (x^2 + xi y^2)
    const auto p2 = q2::add(p, p);
    const auto p6 = q2::norm(q2::add(q2::add(p2, p2), p2));       // 3 (2 x y)
    const auto re = q2::sub(s3, x2);
    const auto ro = q2::add(p6, x2);
    using T = E2<decltype(re)::limb_k, decltype(re)::val_v>;
    const T r = even ? re : q2::relax<T::limb_k, T::val_v>(ro);
    return q2::fit<2>(r);
}

// a^(p - 2) in Fq: 0 -> 0
__device__ inline Lz<Fq29, 1, 2> fq_inv(const Lz<Fq29, 1, 2>& a) {
    Lz<Fq29, 1, 2> acc = Z::relax<1, 2>(Z::one());
#pragma unroll 1
    for (int i = 253; i >= 0; --i) {
        acc = Z::sqr(acc);
        const uint32_t word = FqCfg::M[i >> 5] - (i < 32 ? 2u : 0u);       // the low word of p ends in ...fd47
        if ((word >> (i & 31)) & 1) acc = Z::mul(acc, a);
    }
    return acc;
}

__device__ __forceinline__ El f12_inv(Lane& L, const El& x, const Fq12Consts* cst) {
    const El c = f12_conj(L, x);
    const El t = f12_mul(L, x, c);
    const El t1 = f12_frob<2>(L, t, cst);
    const El t2 = f12_frob<2>(L, t1, cst);
    const El m = f12_mul(L, t1, t2);
    const El nk = f12_mul(L, t, m);                               // N, in coefficient 0
    put_a(L, nk);
    turn(L);
    const El n = L.sh->a[L.side][0];
    const auto d = fq_inv(Z::mul2(n.a, n.a, n.b, n.b));
    El ninv;
    ninv.a = Z::mul(n.a, d);
    ninv.b = Z::mul(Z::norm(Z::sub(Z::zero(), n.b)), d);
    return q2::fit<2>(q2::mul(f12_mul(L, c, m), ninv));
}

// ---- the final exponentiation (every element below the easy part is in the cyclotomic subgroup) ----
__device__ __forceinline__ El f12_easy(Lane& L, const El& f, const Fq12Consts* cst) {
    const El g = f12_mul(L, f12_conj(L, f), f12_inv(L, f, cst));  // f^(p^6 - 1)
    return f12_mul(L, f12_frob<2>(L, g, cst), g);                 // ^(p^2 + 1)
}
constexpr uint64_t kBnX = 0x44e992b44a6909f1ull;                 // the curve's parameter x: 63 bits, 28 ones
__device__ __forceinline__ El f12_pow_x(Lane& L, const El& a) {
    El r = a;
#pragma unroll 1
    for (int i = 61; i >= 0; --i) {
        r = f12_cyc(L, r);
        if ((kBnX >> i) & 1) r = f12_mul(L, r, a);                // the bit is the same for every lane
    }
    return r;
}
__device__ __forceinline__ El f12_pow6(Lane& L, const El& a) { return f12_cyc(L, f12_mul(L, f12_cyc(L, a), a)); }
// f^((p^4 - p^2 + 1) / r), EXACTLY, from the base-p expansion of the exponent:
//   p^3 + (6 x^2 + 1) p^2 + (-36 x^3 - 18 x^2 - 12 x + 1) p + (-36 x^3 - 30 x^2 - 18 x - 2)
__device__ __forceinline__ El f12_hard(Lane& L, const El& f, const Fq12Consts* cst) {
    const El fx = f12_pow_x(L, f);
    const El fx2 = f12_pow_x(L, fx);
    const El fx3 = f12_pow_x(L, fx2);
    const El a = f12_pow6(L, fx), b = f12_pow6(L, fx2), c36 = f12_pow6(L, f12_pow6(L, fx3));
    const El a2 = f12_cyc(L, a), b2 = f12_cyc(L, b);
    const El b3 = f12_mul(L, b2, b);
    const El t = f12_mul(L, f12_mul(L, c36, b3), a2);             // f^(36 x^3 + 18 x^2 + 12 x)
    const El y1 = f12_mul(L, f12_conj(L, t), f);
    const El y0 = f12_conj(L, f12_mul(L, f12_mul(L, f12_mul(L, t, b2), a), f12_cyc(L, f)));
    const El y2 = f12_mul(L, b, f);
    El r = f12_mul(L, y0, f12_frob<1>(L, y1, cst));
    r = f12_mul(L, r, f12_frob<2>(L, y2, cst));
    return f12_mul(L, r, f12_frob<3>(L, f, cst));
}

}  // namespace q12

#endif   // __HIP_DEVICE_COMPILE__

}  // namespace uzk
