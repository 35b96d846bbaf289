// The pairing product on the device: prod_i e(P_i, Q_i) over BN254 by the optimal ate pairing, bit for bit the element of
// oracle/bn254_pairing.py (whose Python-integer restatement of THIS algorithm is tests/pairing_ref.py).
//
//   pairing_check    one lane per pair: every coordinate against p, P on y^2 = x^3 + 3, Q on the twist (lane_tools.hpp, the checks of
//                    g16v_decode); a status byte per pair.  Subgroup membership of Q is the caller's business.
//   pairing_miller   one pair per group of eight lanes, eight pairs per workgroup of one wave (fq12_29.hpp: lane k of a group holds the
//                    coefficient of w^k of f).  The loop runs over the 65 bits of 6 x + 2 in plain binary (64 doublings, 36
//                    additions -- the bits are the same for every pair, so a wave runs one control flow), then the two Frobenius
//                    steps with pi(Q) and -pi^2(Q).  T is kept in homogeneous projective coordinates, in every lane of the group (the
//                    point arithmetic is ~10 Fq2 products a step against the 9 a lane spends on f, and keeping it in place saves the
//                    exchange): no inversion; every line differs from the affine one by a factor in Fq2, which the final
//                    exponentiation removes.  A pair with P or Q at infinity (or a bad status) contributes 1.
//   pairing_prod     a tree of radix 8: a group multiplies eight consecutive values (missing ones are 1); no atomics
//   pairing_finalexp one group: f^((p^6 - 1)(p^2 + 1)) with one inversion, then the hard part exactly (fq12_29.hpp f12_hard)
//
// Every barrier is reached by every lane: lanes without work (the two idle lanes of a group, groups past the last pair) run along on
// valid dummy operands with their writes masked.
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/uzkge_gpu_test.h"
#include "ctx.hpp"
#include "fq12_29.hpp"
#include "handles.hpp"
#include "host_g2.hpp"
#include "lane_tools.hpp"

namespace uzk {

constexpr uint32_t kPairBlock = 64;
constexpr uint32_t kPairsPerBlock = kPairBlock / 8;              // = UZK_PAIRING_PAIRS_PER_WAVE: a workgroup is one wave
constexpr uint32_t kProdRadix = 8;
[[maybe_unused]] constexpr uint64_t kAteLow = 0x9d797039be763ba8ull;   // 6 x + 2 = 2^64 + this
static_assert(kPairsPerBlock == UZK_PAIRING_PAIRS_PER_WAVE, "the header states the pairs of a wave");
enum { PC_OK = 0, PC_NOT_CANONICAL = 1, PC_OFF_CURVE = 2 };

__global__ __launch_bounds__(kPairBlock) void pairing_check_kernel(const Affine* __restrict__ p, const G2Affine* __restrict__ q, uint8_t* __restrict__ status,
                                                                    uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n) return;                                            // no barrier below
    const Affine a = p[i];
    const G2Affine b = q[i];
    uint32_t st = PC_OK;
    if (!(below_modulus<FqCfg>(a.x) && below_modulus<FqCfg>(a.y) && below_modulus<FqCfg>(b.x.c0) && below_modulus<FqCfg>(b.x.c1) &&
          below_modulus<FqCfg>(b.y.c0) && below_modulus<FqCfg>(b.y.c1))) st = PC_NOT_CANONICAL;
    else if (!affine_is_inf(a) && !g1_on_curve(a)) st = PC_OFF_CURVE;
    else if (!(fq2w_is_zero(b.x) && fq2w_is_zero(b.y)) && !g2_on_twist(b)) st = PC_OFF_CURVE;
    status[i] = (uint8_t)st;
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
namespace q12 {
using Base = Lz<Fq29, 1, 4>;       // xP and -yP

// T = 2 T (Costello-Lange-Naehrig's doubling, every coordinate times 4: no halving) and the tangent at P:
// l0 = 2 Y Z (-yP), l1 = 3 X^2 xP, l3 = 3 b' Z^2 - Y^2
__device__ __forceinline__ void dbl_step(const Sh* sh, El& x, El& y, El& z, El& l0, El& l1, El& l3) {
    const El b3 = sh->keep[2];
    const auto b = q2::sqr(y);
    const auto c = q2::sqr(z);
    const auto e = q2::mul(c, b3);
    const auto f = q2::add(q2::add(e, e), e);
    const auto h = q2::fit<2>(q2::sub(q2::sqr(q2::norm(q2::add(y, z))), q2::add(b, c)));
    const auto j = q2::sqr(x);
    const auto xy = q2::mul(x, y);
    const auto e2 = q2::sqr(q2::norm(q2::add(e, e)));            // 4 e^2
    const auto bpf = q2::sqr(q2::norm(q2::add(b, f)));
    x = q2::fit<2>(q2::mul(q2::norm(q2::add(xy, xy)), q2::norm(q2::sub(b, f))));
    y = q2::fit<2>(q2::sub(bpf, q2::add(q2::add(e2, e2), e2)));
    const auto bh = q2::mul(b, h);
    const auto bh2 = q2::add(bh, bh);
    z = q2::fit<2>(q2::add(bh2, bh2));
    l0 = q2::fit<2>(q2::mul_base(h, sh->base[1]));
    l1 = q2::fit<2>(q2::mul_base(q2::norm(q2::add(q2::add(j, j), j)), sh->base[0]));
    l3 = q2::fit<2>(q2::sub(e, b));
}
// T = T + Q (Q affine) and the chord at P, negated: l0 = lambda (-yP), l1 = theta xP, l3 = lambda yQ - theta xQ
__device__ __forceinline__ void add_step(const Sh* sh, El& x, El& y, El& z, const El& qx, const El& qy, El& l0, El& l1, El& l3) {
    const auto theta = q2::norm(q2::sub(y, q2::mul(qy, z)));
    const auto lam = q2::norm(q2::sub(x, q2::mul(qx, z)));
    const auto c = q2::sqr(theta);
    const auto d = q2::sqr(lam);
    const auto e = q2::mul(lam, d);
    const auto f = q2::mul(z, c);
    const auto g = q2::mul(x, d);
    const auto h = q2::norm(q2::sub(q2::add(e, f), q2::add(g, g)));
    const auto y3 = q2::sub(q2::mul(theta, q2::norm(q2::sub(g, h))), q2::mul(e, y));
    l0 = q2::fit<2>(q2::mul_base(lam, sh->base[1]));
    l1 = q2::fit<2>(q2::mul_base(theta, sh->base[0]));
    l3 = q2::fit<2>(q2::sub(q2::mul(lam, qy), q2::mul(theta, qx)));
    x = q2::fit<2>(q2::mul(lam, h));
    y = q2::fit<2>(y3);
    z = q2::fit<2>(q2::mul(z, e));
}

// this lane's coefficient of the Miller value of (P, Q); both finite and checked (or dummies whose result is dropped)
__device__ __forceinline__ El miller(Lane& L, const Affine& P, const G2Affine& Q, const Fq12Consts* cst) {
    Fq2w pw;
    pw.c0 = P.x; pw.c1 = P.y;
    const El pxy = q2::ldr(pw);                                    // (xP, yP) as one pair of limbs vectors
    const Base xp = Z::relax<1, 4>(pxy.a), nyp = Z::norm(Z::sub(Z::zero(), pxy.b));
    El tx = q2::ldr(Q.x), ty = q2::ldr(Q.y), tz = el_one();
    // Q is needed at 38 of the 102 steps, the constant and P once a step: they wait in the group's block of the LDS, not in 90
    // registers of every lane
    if (L.act && L.k == 0) {
        L.sh->keep[0] = tx; L.sh->keep[1] = ty; L.sh->keep[2] = q2::ldr(cst->twist_b3);
        L.sh->base[0] = xp; L.sh->base[1] = nyp;
    }
    __syncthreads();
    El f = f12_one(L);
    El l0, l1, l3;
#pragma unroll 1
    for (int i = 63; i >= 0; --i) {
        dbl_step(L.sh, tx, ty, tz, l0, l1, l3);
        f = f12_sqr(L, f);
        f = f12_sparse(L, f, l0, l1, l3);
        if ((kAteLow >> i) & 1) {                                  // the same bit in every lane of the grid
            const El qx = L.sh->keep[0], qy = L.sh->keep[1];
            add_step(L.sh, tx, ty, tz, qx, qy, l0, l1, l3);
            f = f12_sparse(L, f, l0, l1, l3);
        }
    }
    const El qx = L.sh->keep[0], qy = L.sh->keep[1];
    // pi(Q) = (conj(x) gamma_1,2, conj(y) gamma_1,3),  -pi^2(Q) = (x gamma_2,2, -y gamma_2,3)
    {
        const El q1x = q2::fit<2>(q2::mul(q2::norm(q2::conj(qx)), q2::ldr(cst->gamma[0][2])));
        const El q1y = q2::fit<2>(q2::mul(q2::norm(q2::conj(qy)), q2::ldr(cst->gamma[0][3])));
        add_step(L.sh, tx, ty, tz, q1x, q1y, l0, l1, l3);
        f = f12_sparse(L, f, l0, l1, l3);
    }
    {
        const El q2x = q2::fit<2>(q2::mul(qx, q2::ldr(cst->gamma[1][2])));
        const El q2y = q2::fit<2>(q2::mul(q2::norm(q2::neg(qy)), q2::ldr(cst->gamma[1][3])));
        add_step(L.sh, tx, ty, tz, q2x, q2y, l0, l1, l3);
        f = f12_sparse(L, f, l0, l1, l3);
    }
    return f;
}
}  // namespace q12
#endif

// out[i] = the Miller value of pair i (1 for a pair with a point at infinity or a nonzero status); status may be null
__global__ __launch_bounds__(kPairBlock) void pairing_miller_kernel(const Affine* __restrict__ p, const G2Affine* __restrict__ q, const uint8_t* __restrict__ status,
                                                                     uint32_t n, const Fq12Consts* __restrict__ cst, Fq12w* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace q12;
    __shared__ Sh sh[kPairsPerBlock];
    const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const uint32_t pair = blockIdx.x * kPairsPerBlock + g;
    const bool have = pair < n;
    const uint32_t src = have ? pair : 0;                          // n >= 1: a group past the end runs pair 0 and drops it
    Lane L{&sh[g], lane < 6 ? (int)lane : 0, lane < 6, 0};
    const Affine P = p[src];
    const G2Affine Q = q[src];
    const bool unit = affine_is_inf(P) || (fq2w_is_zero(Q.x) && fq2w_is_zero(Q.y)) || (status && status[src] != 0);
    const El f = miller(L, P, Q, cst);
    if (have && L.act) out[pair].c[L.k] = q2::to_wire(unit ? f12_one(L) : f);
#endif
}

// out[g] = in[8 g] ... in[8 g + 7] (those below n)
__global__ __launch_bounds__(kPairBlock) void pairing_prod_kernel(const Fq12w* __restrict__ in, uint32_t n, Fq12w* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace q12;
    __shared__ Sh sh[kPairsPerBlock];
    const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const uint32_t item = blockIdx.x * kPairsPerBlock + g;
    const uint32_t first = item * kProdRadix;
    Lane L{&sh[g], lane < 6 ? (int)lane : 0, lane < 6, 0};
    El acc = first < n ? q2::ldr(in[first].c[L.k]) : f12_one(L);
#pragma unroll 1
    for (uint32_t t = 1; t < kProdRadix; ++t) {                    // every group takes every turn: the barriers are the workgroup's
        const El v = first + t < n ? q2::ldr(in[first + t].c[L.k]) : f12_one(L);
        acc = f12_mul(L, acc, v);
    }
    if (first < n && L.act) out[item].c[L.k] = q2::to_wire(acc);
#endif
}

// one group, eight lanes
__global__ __launch_bounds__(8) void pairing_finalexp_kernel(const Fq12w* __restrict__ in, const Fq12Consts* __restrict__ cst, Fq12w* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace q12;
    __shared__ Sh sh[1];
    const uint32_t lane = threadIdx.x;
    Lane L{&sh[0], lane < 6 ? (int)lane : 0, lane < 6, 0};
    const El f = q2::ldr(in->c[L.k]);
    const El r = f12_hard(L, f12_easy(L, f, cst), cst);
    if (L.act) out->c[L.k] = q2::to_wire(r);
#endif
}

// uzk_test_fq12_kat: one element per group
__global__ __launch_bounds__(kPairBlock) void pairing_kat_kernel(int op, const Fq12w* __restrict__ a, const Fq12w* __restrict__ b, Fq12w* __restrict__ out, uint32_t n,
                                                                  const Fq12Consts* __restrict__ cst) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace q12;
    __shared__ Sh sh[kPairsPerBlock];
    const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const uint32_t item = blockIdx.x * kPairsPerBlock + g;
    const uint32_t src = item < n ? item : 0;
    Lane L{&sh[g], lane < 6 ? (int)lane : 0, lane < 6, 0};
    const El x = q2::ldr(a[src].c[L.k]), y = q2::ldr(b[src].c[L.k]);
    El r = x;
    switch (op) {                                                  // the same op in every lane: the barriers inside are uniform
        case 0: r = f12_mul(L, x, y); break;
        case 1: r = f12_sqr(L, x); break;
        case 2: r = f12_sparse(L, x, q2::ldr(b[src].c[0]), q2::ldr(b[src].c[1]), q2::ldr(b[src].c[3])); break;
        case 3: r = f12_conj(L, x); break;
        case 4: r = f12_frob<1>(L, x, cst); break;
        case 5: r = f12_frob<2>(L, x, cst); break;
        case 6: r = f12_frob<3>(L, x, cst); break;
        case 7: r = f12_inv(L, x, cst); break;
        case 8: r = f12_cyc(L, x); break;
        case 9: r = f12_easy(L, x, cst); break;
        case 10: r = f12_hard(L, x, cst); break;
        default: break;
    }
    if (item < n && L.act) out[item].c[L.k] = q2::to_wire(r);
#endif
}

// The same operations on RAW limbs (uzk_test_fq12_raw_kat, uzk_test_miller_step_raw): components are taken exactly as given -- nothing is
// re-limbed or reduced on the way in, nothing canonicalised on the way out -- so a test can put every component at the edge of El's bound
// and read whether the result is inside it.
struct F12Raw {
    uint32_t c[6][2][9];               // the coefficient of w^k: c0 then c1, nine limbs (op 12 out: eight wire words, the ninth 0)
};
struct F12RawIn {
    F12Raw a, b;
};
struct MillerRawIn {
    uint32_t t[3][2][9];               // T = x, y, z
    uint32_t q[2][2][9];               // Q = qx, qy
    uint32_t base[2][9];               // xP, -yP
};
struct MillerRawOut {
    uint32_t r[6][2][9];               // x, y, z, l0, l1, l3 of lane 0
    uint32_t diff[2][9];               // OR over lanes 1 .. 5 and the six values of (their result XOR lane 0's)
};

#if defined(__HIP_DEVICE_COMPILE__)
namespace q12 {
__device__ __forceinline__ El raw_el(const uint32_t (&c)[2][9]) {
    El r;
#pragma unroll
    for (int i = 0; i < 9; ++i) { r.a.v.l[i] = c[0][i]; r.b.v.l[i] = c[1][i]; }
    return r;
}
__device__ __forceinline__ void raw_put(uint32_t (&c)[2][9], const El& x) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { c[0][i] = x.a.v.l[i]; c[1][i] = x.b.v.l[i]; }
}
__device__ __forceinline__ Base raw_base(const uint32_t (&c)[9]) {
    Base r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v.l[i] = c[i];
    return r;
}
}  // namespace q12
#endif

// uzk_test_fq12_raw_kat: one element per group, lane k holds coefficient k as it lies in the record
__global__ __launch_bounds__(kPairBlock) void pairing_raw_kat_kernel(int op, const F12RawIn* __restrict__ in, F12Raw* __restrict__ out, uint32_t n,
                                                                      const Fq12Consts* __restrict__ cst) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace q12;
    __shared__ Sh sh[kPairsPerBlock];
    const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const uint32_t item = blockIdx.x * kPairsPerBlock + g;
    const uint32_t src = item < n ? item : 0;                      // n >= 1: a group past the end runs element 0 and drops it
    Lane L{&sh[g], lane < 6 ? (int)lane : 0, lane < 6, 0};
    const El x = raw_el(in[src].a.c[L.k]), y = raw_el(in[src].b.c[L.k]);
    El r = x;
    switch (op) {                                                  // the same op in every lane: the barriers inside are uniform
        case 0: r = f12_mul(L, x, y); break;
        case 1: r = f12_sqr(L, x); break;
        case 2: r = f12_sparse(L, x, raw_el(in[src].b.c[0]), raw_el(in[src].b.c[1]), raw_el(in[src].b.c[3])); break;
        case 3: r = f12_conj(L, x); break;
        case 4: r = f12_frob<1>(L, x, cst); break;
        case 5: r = f12_frob<2>(L, x, cst); break;
        case 6: r = f12_frob<3>(L, x, cst); break;
        case 7: r = f12_inv(L, x, cst); break;
        case 8: r = f12_cyc(L, x); break;
        case 9: r = f12_easy(L, x, cst); break;
        case 10: r = f12_hard(L, x, cst); break;
        case 11: r = xi_mul(x); break;
        default: break;
    }
    if (item < n && L.act) {
        if (op == 12) {
            const Fq2w w = q2::to_wire(x);
            uint32_t (&c)[2][9] = out[item].c[L.k];
#pragma unroll
            for (int i = 0; i < 8; ++i) { c[0][i] = w.c0.v[i]; c[1][i] = w.c1.v[i]; }
            c[0][8] = 0; c[1][8] = 0;
        } else {
            raw_put(out[item].c[L.k], r);
        }
    }
#endif
}

// uzk_test_miller_step_raw: one record per group; the group's block of the LDS is filled as miller() fills it, every lane computes the
// same step, lane 0's result is written with what the other five coefficient lanes' results differ from it by
__global__ __launch_bounds__(kPairBlock) void pairing_raw_step_kernel(int op, const MillerRawIn* __restrict__ in, MillerRawOut* __restrict__ out, uint32_t n,
                                                                       const Fq12Consts* __restrict__ cst) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace q12;
    __shared__ Sh sh[kPairsPerBlock];
    const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const uint32_t item = blockIdx.x * kPairsPerBlock + g;
    const uint32_t src = item < n ? item : 0;
    Lane L{&sh[g], lane < 6 ? (int)lane : 0, lane < 6, 0};
    const MillerRawIn& rec = in[src];
    El v[6];
    v[0] = raw_el(rec.t[0]); v[1] = raw_el(rec.t[1]); v[2] = raw_el(rec.t[2]);
    if (L.act && L.k == 0) {
        L.sh->keep[0] = raw_el(rec.q[0]); L.sh->keep[1] = raw_el(rec.q[1]); L.sh->keep[2] = q2::ldr(cst->twist_b3);
        L.sh->base[0] = raw_base(rec.base[0]); L.sh->base[1] = raw_base(rec.base[1]);
    }
    __syncthreads();
    if (op == 0) {
        dbl_step(L.sh, v[0], v[1], v[2], v[3], v[4], v[5]);
    } else {
        const El qx = L.sh->keep[0], qy = L.sh->keep[1];
        add_step(L.sh, v[0], v[1], v[2], qx, qy, v[3], v[4], v[5]);
    }
    // a workgroup is one wave: lane 0 of the group collects the differences by shuffles that every lane of the wave runs
    uint32_t diff[2][9];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            uint32_t d = 0;
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const uint32_t mine = j == 0 ? v[t].a.v.l[i] : v[t].b.v.l[i];
                d |= mine ^ (uint32_t)__shfl((int)mine, (int)(g * kGroup), 64);
            }
            uint32_t acc = 0;
#pragma unroll
            for (int o = 1; o < 6; ++o) acc |= (uint32_t)__shfl((int)d, (int)(g * kGroup + o), 64);
            diff[j][i] = acc;
        }
    if (item < n && lane == 0) {
#pragma unroll
        for (int t = 0; t < 6; ++t) raw_put(out[item].r[t], v[t]);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 9; ++i) out[item].diff[j][i] = diff[j][i];
    }
#endif
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// xi^((p - 1) / 6) by square and multiply over the quotient's bits, then gamma_1,k = g^k, gamma_2,k = gamma_1,k conj(gamma_1,k),
// gamma_3,k = gamma_1,k gamma_2,k (gamma^(p^2) = gamma in Fq2); 3 b' = 9 / xi.
static Fq12Consts make_consts() {
    using namespace h64;
    const F one = from_fp(Fq::one());
    F nine = zero();
    for (int i = 0; i < 9; ++i) nine = add(nine, one);
    const F2 xi{nine, one};
    uint32_t e[8];                                                 // (p - 1) / 6: p = 1 mod 6
    uint64_t rem = 0;
    for (int i = 7; i >= 0; --i) {
        const uint64_t cur = (rem << 32) | (uint64_t)(FqCfg::M[i] - (i == 0 ? 1u : 0u));
        e[i] = (uint32_t)(cur / 6);
        rem = cur % 6;
    }
    F2 g = f2_one();
    for (int i = 255; i >= 0; --i) {
        g = sqr(g);
        if ((e[i >> 5] >> (i & 31)) & 1) g = mul(g, xi);
    }
    Fq12Consts c;
    F2 gk = f2_one();
    for (int k = 0; k < 6; ++k) {
        const F2 cj{gk.a, sub(zero(), gk.b)};
        const F2 g2 = mul(gk, cj);
        c.gamma[0][k] = f2_to(gk);
        c.gamma[1][k] = f2_to(g2);
        c.gamma[2][k] = f2_to(mul(gk, g2));
        gk = mul(gk, g);
    }
    c.twist_b3 = f2_to(mul(F2{nine, zero()}, inv(xi)));
    return c;
}
const Fq12Consts& pairing_consts() {
    static const Fq12Consts c = make_consts();
    return c;
}

struct PairWs {
    Fq12Consts* cst;
    Affine* p;
    G2Affine* q;
    uint8_t* status;
    Fq12w* f[2];
    Fq12w* gt;
};
// the arrays of a product over n pairs, carved from the context's grow-only block; the constants are queued for upload
static int pairing_carve(Ctx& c, uint32_t n, PairWs* w) {
    const size_t nn = n ? n : 1;
    WsCarver cv;
    const auto a_cst = cv.array<Fq12Consts>(1);
    const auto a_p = cv.array<Affine>(nn);
    const auto a_q = cv.array<G2Affine>(nn);
    const auto a_st = cv.array<uint8_t>(nn);
    const auto a_f0 = cv.array<Fq12w>(nn), a_f1 = cv.array<Fq12w>((nn + kProdRadix - 1) / kProdRadix), a_gt = cv.array<Fq12w>(1);
    UZK_TRY(cv.reserve(c.pairing_ws));
    w->cst = cv(a_cst); w->p = cv(a_p); w->q = cv(a_q); w->status = cv(a_st);
    w->f[0] = cv(a_f0); w->f[1] = cv(a_f1); w->gt = cv(a_gt);
    UZK_HIP(hipMemcpyAsync(w->cst, &pairing_consts(), sizeof(Fq12Consts), hipMemcpyHostToDevice, c.stream));
    return UZK_OK;
}

static Fq12w gt_one() {
    Fq12w r;
    std::memset(&r, 0, sizeof r);
    r.c[0].c0 = Fq::one();
    return r;
}

// Miller loops of w.p, w.q (n >= 1; w.status from the check kernel or null), the tree and the final exponentiation, all queued on the
// context's stream; the result is left in w.gt
static int pairing_queue(Ctx& c, const PairWs& w, const uint8_t* d_status, uint32_t n) {
    UZK_LAUNCH(c, "pairing_miller", pairing_miller_kernel, dim3((n + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kPairBlock), 0, c.stream, w.p, w.q, d_status, n, w.cst, w.f[0]);
    uint32_t cnt = n;
    int cur = 0;
    {
        KernelScope ks(c, "pairing_prod");
        while (cnt > 1) {
            const uint32_t outs = (cnt + kProdRadix - 1) / kProdRadix;
            hipLaunchKernelGGL(pairing_prod_kernel, dim3((outs + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kPairBlock), 0, c.stream, w.f[cur], cnt, w.f[cur ^ 1]);
            cnt = outs;
            cur ^= 1;
        }
    }
    UZK_HIP(hipGetLastError());
    UZK_LAUNCH(c, "pairing_finalexp", pairing_finalexp_kernel, dim3(1), dim3(8), 0, c.stream, w.f[cur], w.cst, w.gt);
    return UZK_OK;
}

// The product over n pairs in host memory, or in this device's (on_device: the Groth16 fold's workspace, used where it lies); *bad_out: the first pair
// that failed its check, with its status, or n
int pairing_product_run(Ctx& c, const Affine* p, const G2Affine* q, bool on_device, uint32_t n, Fq12w* gt_out, uint32_t* bad_out, uint8_t* bad_status) {
    *bad_out = n;
    if (n == 0) { *gt_out = gt_one(); return UZK_OK; }
    PairWs w;
    UZK_TRY(pairing_carve(c, n, &w));
    if (on_device) {
        w.p = const_cast<Affine*>(p); w.q = const_cast<G2Affine*>(q);        // read only
    } else {
        UZK_HIP(hipMemcpyAsync(w.p, p, (size_t)n * sizeof(Affine), hipMemcpyHostToDevice, c.stream));
        UZK_HIP(hipMemcpyAsync(w.q, q, (size_t)n * sizeof(G2Affine), hipMemcpyHostToDevice, c.stream));
    }
    UZK_LAUNCH(c, "pairing_check", pairing_check_kernel, dim3((n + kPairBlock - 1) / kPairBlock), dim3(kPairBlock), 0, c.stream, w.p, w.q, w.status, n);
    UZK_TRY(pairing_queue(c, w, w.status, n));
    if (c.pairing_status.size() < n) c.pairing_status.resize(n);          // grow-only, like the device block
    uint8_t* st = c.pairing_status.data();
    UZK_HIP(hipMemcpyAsync(st, w.status, n, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(gt_out, w.gt, sizeof(Fq12w), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    for (uint32_t i = 0; i < n; ++i) {
        if (st[i]) { *bad_out = i; *bad_status = st[i]; break; }
    }
    return UZK_OK;
}

bool gt_is_one(const Fq12w& a) {
    const Fq12w one = gt_one();
    return std::memcmp(&a, &one, sizeof one) == 0;
}

// ---- test hooks -------------------------------------------------------------------------------------------------------------------
int pairing_kat_device(Ctx& c, int op, const Fq12w* a, const Fq12w* b, Fq12w* out, uint32_t n) {
    if (n == 0) return UZK_OK;
    const size_t bytes = (size_t)n * sizeof(Fq12w);
    WsCarver cv;
    const auto a_cst = cv.array<Fq12Consts>(1);
    const auto a_a = cv.array<Fq12w>(n), a_b = cv.array<Fq12w>(n), a_o = cv.array<Fq12w>(n);
    UZK_TRY(cv.reserve(c.pairing_ws));
    Fq12Consts* d_cst = cv(a_cst);
    Fq12w *da = cv(a_a), *db = cv(a_b), *dout = cv(a_o);
    UZK_HIP(hipMemcpyAsync(d_cst, &pairing_consts(), sizeof(Fq12Consts), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(pairing_kat_kernel, dim3((n + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kPairBlock), 0, c.stream, op, da, db, dout, n, d_cst);
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int pairing_miller_device(Ctx& c, const Affine* p, const G2Affine* q, uint32_t n, Fq12w* out) {
    if (n == 0) return UZK_OK;
    PairWs w;
    UZK_TRY(pairing_carve(c, n, &w));
    UZK_HIP(hipMemcpyAsync(w.p, p, (size_t)n * sizeof(Affine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(w.q, q, (size_t)n * sizeof(G2Affine), hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(pairing_miller_kernel, dim3((n + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kPairBlock), 0, c.stream, w.p, w.q, (const uint8_t*)nullptr, n, w.cst, w.f[0]);
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(out, w.f[0], (size_t)n * sizeof(Fq12w), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// n records In -> n records Out, both on the host, through device buffers of the call's own (the constants with them)
template <class In, class Out, class Kernel>
static int pairing_raw_run(Ctx& c, Kernel kernel, int op, const uint32_t* in, uint32_t* out, uint32_t n) {
    if (n == 0) return UZK_OK;
    In* din = nullptr;
    Out* dout = nullptr;
    Fq12Consts* d_cst = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&din), (size_t)n * sizeof(In));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), (size_t)n * sizeof(Out));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_cst), sizeof(Fq12Consts));
    if (e == hipSuccess) e = hipMemcpyAsync(d_cst, &pairing_consts(), sizeof(Fq12Consts), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(din, in, (size_t)n * sizeof(In), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3((n + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kPairBlock), 0, c.stream, op, din, dout, n, d_cst);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * sizeof(Out), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (d_cst) (void)hipFree(d_cst);
    UZK_HIP(e);
    return UZK_OK;
}
int pairing_raw_kat_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, uint32_t n) {
    static_assert(sizeof(F12RawIn) == 216 * sizeof(uint32_t) && sizeof(F12Raw) == 108 * sizeof(uint32_t), "records are packed words");
    return pairing_raw_run<F12RawIn, F12Raw>(c, pairing_raw_kat_kernel, op, in, out, n);
}
int pairing_raw_step_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, uint32_t n) {
    static_assert(sizeof(MillerRawIn) == 108 * sizeof(uint32_t) && sizeof(MillerRawOut) == 126 * sizeof(uint32_t), "records are packed words");
    return pairing_raw_run<MillerRawIn, MillerRawOut>(c, pairing_raw_step_kernel, op, in, out, n);
}

}  // namespace uzk
