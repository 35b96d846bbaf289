// Fq2 = Fq[u] / (u^2 + 1) on the lazy 29-bit limbs with the bounds in the type (lz29.hpp): an element is two Lz of one bound.
// Wire form: c0 then c1, each the canonical 8 x 32-bit Montgomery words of Fq (radix 2^256) -- arkworks' Fq2 as it lies in memory.
//
// The product comes in two forms ("G2 MSM", has their emitted instruction counts):
//   mul       two dual products  c0 = a0 b0 + a1 (-b1),  c1 = a0 b1 + a1 b0: four multiplications, TWO reductions, results normalized;
//   mul_kara  Karatsuba: three products over lazy sums, then c0 = t0 - t1, c1 = t2 - t0 - t1 and a carry step each.
// Both are 486 multiply-adds; the dual form has no carry steps, one subtraction instead of three, and leaves normalized limbs, so
// it is the one the group law uses.  The square is the complex one: (a0 + a1)(a0 - a1), 2 a0 a1 -- two products.
#pragma once
#include "lz29.hpp"

namespace uzk {

struct Fq2w {          // wire
    Fp c0, c1;
};

#if defined(__HIP_DEVICE_COMPILE__)

namespace q2 {
using F = Fq29;
using Z = LzOps<Fq29>;

template <int K, int V>
struct E2 {
    Lz<Fq29, K, V> a, b;
    static constexpr int limb_k = K, val_v = V;
};

// canonical wire element -> 2^261-form by re-limbing (value < 32 M)
__device__ __forceinline__ E2<1, 32> ld(const Fq2w& w) { E2<1, 32> r; r.a = Z::ld(w.c0); r.b = Z::ld(w.c1); return r; }
// the same, then one reduction: value < 2 M (what the accumulator does to a coordinate it keeps)
__device__ __forceinline__ E2<1, 2> ldr(const Fq2w& w) {
    E2<1, 2> r;
    r.a.v = F::reduce(F::from_fp_x32(w.c0)); r.b.v = F::reduce(F::from_fp_x32(w.c1));
    return r;
}
// the wire words taken as they are (2^256-form): a product with a 2^266-form operand lands in 2^261-form
__device__ __forceinline__ E2<1, 1> ldp(const Fq2w& w) { E2<1, 1> r; r.a = Z::ldp(w.c0); r.b = Z::ldp(w.c1); return r; }
__device__ __forceinline__ E2<1, 1> zero() { E2<1, 1> r; r.a = Z::zero(); r.b = Z::zero(); return r; }

template <int Ka, int Va, int Kb, int Vb>
__device__ __forceinline__ E2<Ka + Kb, Va + Vb> add(const E2<Ka, Va>& x, const E2<Kb, Vb>& y) {
    E2<Ka + Kb, Va + Vb> r; r.a = Z::add(x.a, y.a); r.b = Z::add(x.b, y.b); return r;
}
template <int Ka, int Va, int Kb, int Vb>
__device__ __forceinline__ E2<Ka + Kb + 2, Va + Vb + 1> sub(const E2<Ka, Va>& x, const E2<Kb, Vb>& y) {
    E2<Ka + Kb + 2, Va + Vb + 1> r; r.a = Z::sub(x.a, y.a); r.b = Z::sub(x.b, y.b); return r;
}
template <int K, int V>
__device__ __forceinline__ E2<K + 3, V + 2> neg(const E2<K, V>& x) { return sub(zero(), x); }
template <int K, int V>
__device__ __forceinline__ E2<1, V> norm(const E2<K, V>& x) { E2<1, V> r; r.a = Z::norm(x.a); r.b = Z::norm(x.b); return r; }
template <int K2, int V2, int K, int V>
__device__ __forceinline__ E2<K2, V2> relax(const E2<K, V>& x) {
    E2<K2, V2> r; r.a = Z::template relax<K2, V2>(x.a); r.b = Z::template relax<K2, V2>(x.b); return r;
}
// value < 32 M -> normalized, value < 2 M (Field29::reduce, contract in fp29.hpp: limbs < 2^32 - 2^3 holds for every K <= 7)
template <int K, int V>
__device__ __forceinline__ E2<1, 2> red(const E2<K, V>& x) {
    static_assert(V <= 32, "reduce() takes values below 32 M");
    static_assert(K <= 7, "reduce() takes limbs below 2^32 - 2^3: K (2^29 + 2^6) stays below that up to K = 7");
    E2<1, 2> r; r.a.v = F::reduce(x.a.v); r.b.v = F::reduce(x.b.v); return r;
}
// the loop-carried form of a value: bound VT, normalized -- a carry step when the bound holds, a reduction when it does not
template <int VT, int K, int V>
__device__ __forceinline__ E2<1, VT> fit(const E2<K, V>& x) {
    if constexpr (V <= VT && K == 1) return relax<1, VT>(x);
    else if constexpr (V <= VT) return relax<1, VT>(norm(x));
    else return relax<1, VT>(red(x));
}

constexpr int mul_v(int va, int vb) { return 1 + (va * vb + va * (vb + 2) + 168) / 169; }
// (a0 + a1 u)(b0 + b1 u) = (a0 b0 - a1 b1) + (a0 b1 + a1 b0) u by two dual products
template <int Va, int Vb>
__device__ __forceinline__ E2<1, mul_v(Va, Vb)> mul(const E2<1, Va>& x, const E2<1, Vb>& y) {
    E2<1, mul_v(Va, Vb)> r;
    r.a = Z::mul2(x.a, y.a, x.b, Z::sub(Z::zero(), y.b));
    r.b = Z::template relax<1, mul_v(Va, Vb)>(Z::mul2(x.a, y.b, x.b, y.a));
    return r;
}
constexpr int kara_v(int va, int vb) { return Z::prod_v(2 * va, 2 * vb) + 2 * Z::prod_v(va, vb) + 1; }
template <int Va, int Vb>
__device__ __forceinline__ E2<1, kara_v(Va, Vb)> mul_kara(const E2<1, Va>& x, const E2<1, Vb>& y) {
    const auto t0 = Z::mul(x.a, y.a), t1 = Z::mul(x.b, y.b);
    const auto t2 = Z::mul(Z::add(x.a, x.b), Z::add(y.a, y.b));
    E2<1, kara_v(Va, Vb)> r;
    r.a = Z::template relax<1, kara_v(Va, Vb)>(Z::norm(Z::sub(t0, t1)));
    r.b = Z::norm(Z::sub(t2, Z::add(t0, t1)));
    return r;
}
constexpr int sqr_v(int v) { return Z::prod_v(2 * v, 2 * v + 1); }
template <int V>
__device__ __forceinline__ E2<1, sqr_v(V)> sqr(const E2<1, V>& x) {
    E2<1, sqr_v(V)> r;
    r.a = Z::mul(Z::add(x.a, x.b), Z::norm(Z::sub(x.a, x.b)));
    r.b = Z::template relax<1, sqr_v(V)>(Z::mul(Z::add(x.a, x.a), x.b));
    return r;
}
// a coordinate (x, y)-wise product with an Fq constant in plain limbs (e.g. 2^266 mod M: 2^261-form -> 2^266-form)
template <int V>
__device__ __forceinline__ E2<1, Z::prod_v(V, 1)> mul_fq(const E2<1, V>& x, const uint32_t (&c)[9]) {
    Lz<Fq29, 1, 1> k; k.v = F::constant(c);
    E2<1, Z::prod_v(V, 1)> r; r.a = Z::mul(x.a, k); r.b = Z::mul(x.b, k); return r;
}
// the product with an element of Fq (2^261-form): two products
template <int V, int Vb>
__device__ __forceinline__ E2<1, Z::prod_v(V, Vb)> mul_base(const E2<1, V>& x, const Lz<Fq29, 1, Vb>& k) {
    E2<1, Z::prod_v(V, Vb)> r; r.a = Z::mul(x.a, k); r.b = Z::mul(x.b, k); return r;
}
// a0 - a1 u (the p-power map of Fq2)
template <int K, int V>
__device__ __forceinline__ E2<K + 3, V + 2> conj(const E2<K, V>& x) {
    E2<K + 3, V + 2> r; r.a = Z::template relax<K + 3, V + 2>(x.a); r.b = Z::sub(Z::zero(), x.b); return r;
}
// 0 in Fq2?  Exact for every value below 32 M: one reduction (< 2 M), then the three candidates 0, M, 2 M.  The second component is
// only looked at when the first is zero.
template <int K, int V>
__device__ __forceinline__ bool is_zero(const E2<K, V>& x) {
    static_assert(V <= 32, "reduce() takes values below 32 M");
    static_assert(K <= 7, "reduce() takes limbs below 2^32 - 2^3: K (2^29 + 2^6) stays below that up to K = 7");
    if (!F::is_zero_mod_small(F::reduce(x.a.v))) return false;
    return F::is_zero_mod_small(F::reduce(x.b.v));
}
// 2^261-form -> canonical wire words
template <int K, int V>
__device__ __forceinline__ Fq2w to_wire(const E2<K, V>& x) { Fq2w w; w.c0 = Z::to_wire(x.a); w.c1 = Z::to_wire(x.b); return w; }
// 2^266-form, value < 2 M -> canonical wire words by exact division by 2^10 (fp29.hpp to_fp_div)
__device__ __forceinline__ Fq2w to_wire_266(const E2<1, 2>& x) {
    Fq2w w;
    w.c0 = Fq::canon(F::template to_fp_div<10>(x.a.v)); w.c1 = Fq::canon(F::template to_fp_div<10>(x.b.v));
    return w;
}
}  // namespace q2

#endif   // __HIP_DEVICE_COMPILE__

}  // namespace uzk
