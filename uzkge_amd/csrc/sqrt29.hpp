// Square roots in the three fields a compressed point needs, on the typed lazy limbs of lz29.hpp, one lane per element: Fq (G1's y),
// Fq2 (G2's y) and Fr (Baby Jubjub's x).  Every lane of a wave walks the same constant exponent from a table it reads at the same
// index (3-bit windows, the table entry chosen by compares: anemoi29.hpp's chain), and the loops below have the same trip counts in
// every lane, so a wave runs one control flow whatever it is given.  All values are in 2^261-form; the running power of a chain is
// Lz<F, 1, 2>, which a square or a product of two such values returns to (the compiler checks each line).
//
//   Fq    p = 3 mod 4:  t = a^((p - 3) / 4) in ONE chain, root = a t, and a is a square iff root^2 = a -- no Legendre chain.  For a
//         nonzero square t is also 1 / root (a t^2 = a^((p - 1) / 2) = 1).
//   Fq2   the norm method (tests/g2_ref.py f2_sqrt): n = sqrt(a0^2 + a1^2), then x0 = sqrt((a0 + n) / 2) or sqrt((a0 - n) / 2) --
//         their product is -a1^2 / 4, a non-square, so exactly one of the two is a square -- and x1 = a1 / (2 x0) = a1 t / 2 with the t
//         of x0's chain: no inversion.  With a1 = 0 the two candidates are a0 and -a0 (the root is real, or lies on the u axis).  The
//         two candidates are two independent chains walked side by side in the lane.  Three chain lengths in all; the square of the
//         result against a decides.
//   Fr    r - 1 = 2^28 m.  For x^2 v = u with a = u v:  w = a^((m - 1) / 2) in one chain, b = a w^2 = a^m lies in the subgroup of order
//         2^28, and with s^2 = 1 / b the root is u w s ((u w s)^2 v = u^2 w^2 v / (a w^2) = u: the division costs nothing).  s comes from
//         the discrete logarithm of b over the table rho^-(2^k) of the NTT's 2^28-th root, seven bits at a time (Pohlig-Hellman in two
//         levels): 42 squarings bring b into the subgroup of order 2^7 for each of the four windows, 21 more find a window's bits, and
//         every bit multiplies by a table entry under a select -- 126 squarings and 84 products for every lane alike, against
//         Tonelli-Shanks' up to 27 * 28 / 2 squarings with a trip count of its own in every lane.
//         tools/gen_sqrt_consts.py has the same steps on Python integers.
#pragma once
#include "fq2_29.hpp"

namespace uzk {

#if defined(__HIPCC__)
#include "sqrt_consts.inc"
#endif

#if defined(__HIP_DEVICE_COMPILE__)

namespace sq {
template <class F> using Ch = Lz<F, 1, 2>;
using Cq = Ch<Fq29>;
using Cr = Ch<Fr29>;

template <class F>
__device__ __forceinline__ Ch<F> sel(bool c, const Ch<F>& a, const Ch<F>& b) {
    Ch<F> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v.l[i] = c ? a.v.l[i] : b.v.l[i];
    return r;
}
// the same element with a value below 2 M: one product by 1
template <class F, int K, int V>
__device__ __forceinline__ auto red(const Lz<F, K, V>& a) { return LzOps<F>::mul(a, LzOps<F>::one()); }
template <class F, int K, int V>
__device__ __forceinline__ bool is_zero(const Lz<F, K, V>& a) { return Field<typename WireCfg<typename F::Cfg>::type>::is_zero(LzOps<F>::canon(a)); }
template <class F>
__device__ __forceinline__ bool eq(const Ch<F>& a, const Ch<F>& b) { return is_zero(LzOps<F>::sub(a, b)); }

template <class F>
__device__ __forceinline__ Ch<F> pick(const Ch<F> (&t)[7], uint32_t d) {
    Ch<F> r = t[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) {
#pragma unroll
        for (int i = 0; i < 9; ++i) r.v.l[i] = d == (uint32_t)(k + 1) ? t[k].v.l[i] : r.v.l[i];
    }
    return r;
}
// a^e for the constant e whose 3-bit windows are digits[0 .. WINDOWS) (lowest first, the top one TOP): every lane reads the same digit
template <class F, int WINDOWS, int TOP>
__device__ __forceinline__ Ch<F> pow1(const Ch<F>& a, const uint8_t* digits) {
    using Z = LzOps<F>;
    Ch<F> t[7];
    t[0] = a;
#pragma unroll
    for (int k = 1; k < 7; ++k) t[k] = Z::mul(t[k - 1], a);
    Ch<F> p = t[TOP - 1];
#pragma unroll 1
    for (int w = WINDOWS - 2; w >= 0; --w) {
#pragma unroll
        for (int s = 0; s < kSqrtWindow; ++s) p = Z::sqr(p);
        const uint32_t d = digits[w];
        if (d) p = Z::mul(p, pick(t, d));
    }
    return p;
}
// a^e and b^e: the two chains side by side
template <class F, int WINDOWS, int TOP>
__device__ __forceinline__ void pow2(const Ch<F>& a, const Ch<F>& b, const uint8_t* digits, Ch<F>* ra, Ch<F>* rb) {
    using Z = LzOps<F>;
    Ch<F> ta[7], tb[7];
    ta[0] = a; tb[0] = b;
#pragma unroll
    for (int k = 1; k < 7; ++k) { ta[k] = Z::mul(ta[k - 1], a); tb[k] = Z::mul(tb[k - 1], b); }
    Ch<F> pa = ta[TOP - 1], pb = tb[TOP - 1];
#pragma unroll 1
    for (int w = WINDOWS - 2; w >= 0; --w) {
#pragma unroll
        for (int s = 0; s < kSqrtWindow; ++s) { pa = Z::sqr(pa); pb = Z::sqr(pb); }
        const uint32_t d = digits[w];
        if (d) { pa = Z::mul(pa, pick(ta, d)); pb = Z::mul(pb, pick(tb, d)); }
    }
    *ra = pa; *rb = pb;
}

// root = a^((p + 1) / 4); true iff root^2 = a (a is a square, 0 included).  inv_out: a^((p - 3) / 4), 1 / root for a nonzero square.
__device__ __forceinline__ bool fq_sqrt(const Cq& a, Cq* root, Cq* inv_out = nullptr) {
    using Z = LzOps<Fq29>;
    const Cq t = pow1<Fq29, kFqSqrtWindows, kFqSqrtTopDigit>(a, kFqSqrtDigits);
    *root = Z::mul(a, t);
    if (inv_out) *inv_out = t;
    return eq(Z::sqr(*root), a);
}

// x with x^2 = a in Fq2; true iff there is one
__device__ __forceinline__ bool fq2_sqrt(const q2::E2<1, 2>& a, q2::E2<1, 2>* root) {
    using Z = LzOps<Fq29>;
    Lz<Fq29, 1, 1> half;
    half.v = Fq29::constant(kFqHalf);
    const bool real = is_zero(a.b);
    Cq n;
    (void)fq_sqrt(Z::mul2(a.a, a.a, a.b, a.b), &n);                 // not a square: the last comparison fails whatever comes out
    Cq cp = Z::mul(Z::add(a.a, n), half), cm = Z::mul(Z::sub(a.a, n), half);
    cp = sel(real, a.a, cp);
    cm = sel(real, red(Z::sub(Z::zero(), a.a)), cm);
    Cq tp, tm;
    pow2<Fq29, kFqSqrtWindows, kFqSqrtTopDigit>(cp, cm, kFqSqrtDigits, &tp, &tm);
    const Cq rp = Z::mul(cp, tp), rm = Z::mul(cm, tm);
    const bool plus = eq(Z::sqr(rp), cp);
    const Cq x0 = sel(plus, rp, rm);
    const Cq x1 = Z::mul(Z::mul(a.b, sel(plus, tp, tm)), half);     // a1 / (2 x0)
    const Cq zero = Z::template relax<1, 2>(Z::zero());
    q2::E2<1, 2> x;
    x.a = real ? sel(plus, rp, zero) : x0;
    x.b = real ? sel(plus, zero, rm) : x1;
    *root = x;
    return q2::is_zero(q2::sub(q2::sqr(x), a));
}

// x with x^2 v = u in Fr (v != 0); true iff there is one
__device__ __forceinline__ bool fr_sqrt_ratio(const Cr& u, const Cr& v, Cr* root) {
    using Z = LzOps<Fr29>;
    const Cr one = Z::relax<1, 2>(Z::one());
    const Cr a = Z::mul(u, v);
    const Cr w = pow1<Fr29, kFrSqrtWindows, kFrSqrtTopDigit>(a, kFrSqrtDigits);
    Cr b = Z::mul(Z::mul(a, w), w);
    Cr s = one;
#pragma unroll 1
    for (int j = 0; j < kFrTwoAdicity / kFrDlogWindow; ++j) {
        Cr c = b;
#pragma unroll 1
        for (int k = kFrTwoAdicity - kFrDlogWindow * (j + 1); k > 0; --k) c = Z::sqr(c);
#pragma unroll 1
        for (int i = 0; i < kFrDlogWindow; ++i) {
            Cr d = c;
#pragma unroll 1
            for (int k = kFrDlogWindow - 1 - i; k > 0; --k) d = Z::sqr(d);
            const bool bit = !eq(d, one);
            const int k = kFrDlogWindow * j + i;
            Lz<Fr29, 1, 1> gc, gb, gs;
#pragma unroll
            for (int l = 0; l < 9; ++l) {
                gc.v.l[l] = kFrRootInv[kFrTwoAdicity - kFrDlogWindow + i][l];
                gb.v.l[l] = kFrRootInv[k][l];
                gs.v.l[l] = kFrRootInv[k > 0 ? k - 1 : 0][l];
            }
            c = sel(bit, Z::mul(c, gc), c);
            b = sel(bit, Z::mul(b, gb), b);
            s = sel(bit && k > 0, Z::mul(s, gs), s);               // bit 0 set: no root, and the last comparison says so
        }
    }
    *root = Z::mul(Z::mul(u, w), s);
    return eq(Z::mul(Z::sqr(*root), v), u);
}
}  // namespace sq

#endif   // __HIP_DEVICE_COMPILE__

}  // namespace uzk
