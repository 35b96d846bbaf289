// Anemoi-Jive over BN254's scalar field (uzkge/src/anemoi: AnemoiJive254 -- 2 columns, 14 rounds, alpha = 5, g = 5, delta = 1 / g):
// the permutation and the rate-3 sponge on the typed lazy limbs of lz29.hpp, one lane per item.
//
// One round (anemoi/mod.rs anemoi_permutation):
//     x_i += C[r][i], y_i += D[r][i]                      the keys, generated from the pi rule (tools/gen_anemoi_consts.py)
//     x <- M x,  y <- M (y1, y0)    M = [[1, g], [g, g^2 + 1]]:  m0 = x0 + g x1,  m1 = g m0 + x1   (and the same on y1, y0)
//     y += x,  x += y
//     per column   t = x - g y^2;   y -= t^(1/5);   x = t + g y^2 + delta
// and after round 14 the linear layer once more.  The cost is the root: 1/5 mod (r - 1) has 254 bits, so a root is 254 squarings and,
// over 3-bit windows, at most 85 products by one of t .. t^7 (six more to build them) -- about 340 products, twice per round, ~9.6e3 a
// permutation against 14 for everything else in a round.  The exponent is a constant: the windows come from a table every lane reads at
// the same index, the table entry is chosen by compares against that uniform digit (selects, no indexed register array, no scratch),
// so a wave runs one control flow.  The two columns' roots are two independent product chains walked side by side in the same lane.
//
// Types.  All values are in 2^261-form.  The state between rounds is St = Lz<Fr29, 1, 8>; the chain of a root runs in
// Ch = Lz<Fr29, 1, 2>.  How the bounds close (the compiler checks each line):
//     X = norm(state + key)                           <1, 9>
//     m0 = norm(X0 + 5 X1) <1, 54>,  m1 = norm(5 m0 + X1) <1, 279>       5 a = ((a + a) + (a + a)) + a: three additions, limbs < 5 * 2^29
//     y0' = m0 + n0 <2, 108>  y1' = m1 + n1 <2, 558>  x0' = m0 + y0' <3, 162>  x1' = m1 + y1' <3, 837>      (837 M still fits nine limbs)
//     one product by 1 each                           x <1, 6>, y <1, 5>
//     t = norm(x - G y^2) <1, 9>,  T1 = t * 1 <1, 2>,  u = T1^(1/5) <1, 2>,  y'' = norm(y - u) <1, 8>,  x'' = norm(T1 + G y''^2 + delta) <1, 5>
// g = 5 by ADDITIONS in the linear layer (its operands are carried sums anyway and the product by 1 that follows reduces the value),
// by a PRODUCT with the constant G in the S-box: there 5 y^2 by additions has limbs < 5 * 2^29, which the subtraction's offset cannot
// cover without a carry step, and leaves a value bound (< 10 M, then < 13 M for x'') that the next round's 93-fold sum no longer fits
// in nine limbs -- it would need the reducing product anyway.  DESIGN 3.16 has the instruction counts.
//
// The sponge (eval_variable_length_hash, eval_stream_cipher): rate 3, a chunk adds to x0, x1, y0; a nonempty input whose length is a
// multiple of 3 is absorbed as it is and sigma = 1, otherwise a 1 and zeros are appended and sigma = 0; sigma goes to y1 AFTER the
// last absorbing permutation, so a stream cipher's later permutations see it.  Outputs are x0, x1, y0 per squeeze.
#pragma once
#include "lz29.hpp"

namespace uzk {

// how many permutations absorb `len` elements, and how many one item runs in all (out_len == 0: a hash)
UZK_HD uint32_t anemoi_absorbs(uint32_t len) { return (len % 3 == 0 && len > 0) ? len / 3 : len / 3 + 1; }
UZK_HD uint32_t anemoi_permutations(uint32_t len, uint32_t out_len) {
    const uint32_t a = anemoi_absorbs(len);
    return out_len <= 3 ? a : a + out_len / 3 - 1 + (out_len % 3 ? 1 : 0);
}
constexpr uint32_t kAnemoiTraceElems = 64;         // per permutation: before (4), after each round's S-box (14 x 4), after (4)

// A point of Baby Jubjub as chaum_pedersen/dl.rs prove0 / verify0 feed it to the hash: into_affine().xy().unwrap_or_default().
// SUPPOSED, not verified: the reference's arkworks fork could not be read; in upstream arkworks xy() of the identity is None, so
// the identity (0, 1) enters the hash as (0, 0).  This function is the only place that knows.  x, y: canonical Montgomery words.
UZK_HD void anemoi_cp_point_words(const Fp& x, const Fp& y, Fp* out_x, Fp* out_y) {
    const bool identity = Field<FrCfg>::is_zero(x) && Field<FrCfg>::eq(y, Field<FrCfg>::one());
    *out_x = x;
    *out_y = identity ? Field<FrCfg>::zero() : y;
}

#if defined(__HIPCC__)
#include "anemoi_consts.inc"
#endif

#if defined(__HIP_DEVICE_COMPILE__)

namespace anemoi {
using Z = LzOps<Fr29>;
using St = Lz<Fr29, 1, 8>;          // a word of the state between rounds
using Ch = Lz<Fr29, 1, 2>;          // the running power inside a root
using K1 = Lz<Fr29, 1, 1>;          // a canonical constant

struct State {
    St x0, x1, y0, y1;
};

__device__ __forceinline__ K1 cst(const uint32_t (&c)[9]) { K1 r; r.v = Fr29::constant(c); return r; }
__device__ __forceinline__ K1 key(uint32_t round, int word) {
    K1 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v.l[i] = kAnemoiKeys[round][word][i];
    return r;
}
// the same element with a value below 2 M + ..: one product by 1
template <int K, int V>
__device__ __forceinline__ auto red(const Lz<Fr29, K, V>& a) { return Z::mul(a, Z::one()); }
// a canonical wire element as a word of the state
__device__ __forceinline__ St ld(const Fp& w) { return Z::relax<1, 8>(red(Z::ld(w))); }
template <int V>
__device__ __forceinline__ Lz<Fr29, 5, 5 * V> times5(const Lz<Fr29, 1, V>& a) {
    const auto a2 = Z::add(a, a);
    return Z::add(Z::add(a2, a2), a);
}

// M on (a, b) = (x0, x1) or (y1, y0), then y += x, x += y; the four results reduced by one product each.  In: normalized, < 9 M.
__device__ __forceinline__ void linear(const Lz<Fr29, 1, 9>& x0, const Lz<Fr29, 1, 9>& x1, const Lz<Fr29, 1, 9>& y0, const Lz<Fr29, 1, 9>& y1,
                                       Lz<Fr29, 1, 6>* ox0, Lz<Fr29, 1, 6>* ox1, Lz<Fr29, 1, 5>* oy0, Lz<Fr29, 1, 5>* oy1) {
    const auto m0 = Z::norm(Z::add(x0, times5(x1)));
    const auto m1 = Z::norm(Z::add(times5(m0), x1));
    const auto n0 = Z::norm(Z::add(y1, times5(y0)));
    const auto n1 = Z::norm(Z::add(times5(n0), y0));
    const auto s0 = Z::add(m0, n0);                                // y after y += x
    const auto s1 = Z::add(m1, n1);
    *oy0 = Z::relax<1, 5>(red(s0));
    *oy1 = Z::relax<1, 5>(red(s1));
    *ox0 = Z::relax<1, 6>(red(Z::add(m0, s0)));
    *ox1 = Z::relax<1, 6>(red(Z::add(m1, s1)));
}

__device__ __forceinline__ Ch pick(const Ch (&t)[7], uint32_t d) {
    Ch r = t[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) {
#pragma unroll
        for (int i = 0; i < 9; ++i) r.v.l[i] = d == (uint32_t)(k + 1) ? t[k].v.l[i] : r.v.l[i];
    }
    return r;
}
// a^(1/5) and b^(1/5): fixed 3-bit windows of the constant exponent from the top, the two chains side by side
__device__ __forceinline__ void root2(const Ch& a, const Ch& b, Ch* ra, Ch* rb) {
    Ch ta[7], tb[7];
    ta[0] = a; tb[0] = b;
#pragma unroll
    for (int k = 1; k < 7; ++k) { ta[k] = Z::mul(ta[k - 1], a); tb[k] = Z::mul(tb[k - 1], b); }
    Ch pa = ta[kAnemoiTopDigit - 1], pb = tb[kAnemoiTopDigit - 1];
#pragma unroll 1
    for (int w = kAnemoiWindows - 2; w >= 0; --w) {
#pragma unroll
        for (int s = 0; s < kAnemoiWindow; ++s) { pa = Z::sqr(pa); pb = Z::sqr(pb); }
        const uint32_t d = kAnemoiDigits[w];                        // the same for every lane
        if (d) { pa = Z::mul(pa, pick(ta, d)); pb = Z::mul(pb, pick(tb, d)); }
    }
    *ra = pa; *rb = pb;
}

// the S-boxes of both columns; (x, y) as linear() leaves them
__device__ __forceinline__ void sboxes(const Lz<Fr29, 1, 6>& x0, const Lz<Fr29, 1, 6>& x1, const Lz<Fr29, 1, 5>& y0, const Lz<Fr29, 1, 5>& y1, State* out) {
    const K1 g = cst(kAnemoiG), delta = cst(kAnemoiDelta);
    const Ch t0 = red(Z::norm(Z::sub(x0, Z::mul(Z::sqr(y0), g))));
    const Ch t1 = red(Z::norm(Z::sub(x1, Z::mul(Z::sqr(y1), g))));
    Ch u0, u1;
    root2(t0, t1, &u0, &u1);
    out->y0 = Z::norm(Z::sub(y0, u0));
    out->y1 = Z::norm(Z::sub(y1, u1));
    out->x0 = Z::relax<1, 8>(Z::norm(Z::add(Z::add(t0, Z::mul(Z::sqr(out->y0), g)), delta)));
    out->x1 = Z::relax<1, 8>(Z::norm(Z::add(Z::add(t1, Z::mul(Z::sqr(out->y1), g)), delta)));
}

__device__ __forceinline__ void put4(Fp* dst, const State& s) {
    dst[0] = Z::to_wire(s.x0); dst[1] = Z::to_wire(s.x1); dst[2] = Z::to_wire(s.y0); dst[3] = Z::to_wire(s.y1);
}

// One permutation in place.  trace: null, or the 64 elements of this permutation (before, the state after each round's S-box, after).
__device__ __forceinline__ void permute(State* s, Fp* trace) {
    if (trace) put4(trace, *s);
    Lz<Fr29, 1, 6> x0, x1;
    Lz<Fr29, 1, 5> y0, y1;
#pragma unroll 1
    for (uint32_t r = 0; r < 14; ++r) {
        linear(Z::norm(Z::add(s->x0, key(r, 0))), Z::norm(Z::add(s->x1, key(r, 1))), Z::norm(Z::add(s->y0, key(r, 2))), Z::norm(Z::add(s->y1, key(r, 3))),
               &x0, &x1, &y0, &y1);
        sboxes(x0, x1, y0, y1, s);
        if (trace) put4(trace + 4 + 4 * r, *s);
    }
    linear(Z::relax<1, 9>(s->x0), Z::relax<1, 9>(s->x1), Z::relax<1, 9>(s->y0), Z::relax<1, 9>(s->y1), &x0, &x1, &y0, &y1);
    s->x0 = Z::relax<1, 8>(x0); s->x1 = Z::relax<1, 8>(x1); s->y0 = Z::relax<1, 8>(y0); s->y1 = Z::relax<1, 8>(y1);
    if (trace) put4(trace + 60, *s);
}

__device__ __forceinline__ State zero_state() {
    State s;
    s.x0 = s.x1 = s.y0 = s.y1 = Z::relax<1, 8>(Z::zero());
    return s;
}
// state word + a canonical wire element (or the constant 1), back in the state's type
__device__ __forceinline__ St plus(const St& a, const Fp& w) { return Z::relax<1, 8>(red(Z::add(a, Z::ld(w)))); }
__device__ __forceinline__ St plus_one(const St& a) { return Z::relax<1, 8>(red(Z::add(a, Z::one()))); }

// Element k of the padded input of `len` elements read through `at(k)` (canonical Montgomery words): the input, then 1, then zeros.
// The sponge of one item: absorbs, then squeezes until out_len outputs are written (out_len == 0: the hash, one output, x0).
// trace: null or P x 64 elements.
template <class At>
__device__ __forceinline__ void sponge(At at, uint32_t len, uint32_t out_len, Fp* out, Fp* trace) {
    const uint32_t absorbs = anemoi_absorbs(len), total = anemoi_permutations(len, out_len);
    const bool sigma = len % 3 == 0 && len > 0;
    const uint32_t want = out_len ? out_len : 1;
    State s = zero_state();
    uint32_t written = 0;
#pragma unroll 1
    for (uint32_t p = 0; p < total; ++p) {
        if (p < absorbs) {
            // (at most one of a chunk's three elements is the appended 1, the ones behind it are 0)
            const uint32_t k = 3 * p;
            if (k < len) s.x0 = plus(s.x0, at(k)); else if (k == len) s.x0 = plus_one(s.x0);
            if (k + 1 < len) s.x1 = plus(s.x1, at(k + 1)); else if (k + 1 == len) s.x1 = plus_one(s.x1);
            if (k + 2 < len) s.y0 = plus(s.y0, at(k + 2)); else if (k + 2 == len) s.y0 = plus_one(s.y0);
        }
        permute(&s, trace ? trace + (size_t)p * kAnemoiTraceElems : nullptr);
        if (p + 1 == absorbs && sigma) s.y1 = plus_one(s.y1);
        if (p + 1 >= absorbs) {
            if (written < want) out[written++] = Z::to_wire(s.x0);
            if (written < want) out[written++] = Z::to_wire(s.x1);
            if (written < want) out[written++] = Z::to_wire(s.y0);
        }
    }
}
}  // namespace anemoi

#endif   // __HIP_DEVICE_COMPILE__

}  // namespace uzk
