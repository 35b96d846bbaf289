// Element-wise known-answer entry points: run the DEVICE field / group primitives on host arrays so
// tests can compare them word-for-word with the oracle (Fq/Fr mont-mul/add/sub KATs, G1
// add / double / mixed-add including P+P, P+(-P) and infinity; SURVEY.md 8c "golden vectors").
#include <type_traits>

#include "ctx.hpp"
#include "ecquad.hpp"
#include "ecquad29.hpp"
#include "ec29l.hpp"
#include "fp29.hpp"
#include "lz29.hpp"

namespace uzk {

template <class F, class F29>
__global__ __launch_bounds__(256) void field_op_kernel(int op, const Fp* __restrict__ a, const Fp* __restrict__ b,
                                                       Fp* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp x = a[i], y = b[i], r;
    switch (op) {
        case 0: r = F::mul(x, y); break;
        case 1: r = F::add(x, y); break;
        case 2: r = F::sub(x, y); break;
        case 3: r = F::mul_portable(x, y); break;
        case 4: r = F::sqr(x); break;
        case 5: r = F::neg(x); break;
        case 6: r = F::from_mont(x); break;
        case 8: r = F::add_portable(x, y); break;
        case 9: r = F::sub_portable(x, y); break;
        // ---- the 9 x 29-bit-limb representation (fp29.hpp), results mapped back to canonical words ----
        case 10: r = F29::to_fp(F29::canon(F29::mul(F29::from_fp(x), F29::to_261(F29::from_fp(y))))); break;   // x*y (2^256-form)
        case 11: r = F29::to_fp(F29::canon(F29::add(F29::from_fp(x), F29::from_fp(y)))); break;
        case 12: r = F29::to_fp(F29::canon(F29::template sub<4>(F29::from_fp(x), F29::from_fp(y)))); break;
        case 13: r = F29::to_fp(F29::canon(F29::template sub<12>(F29::from_fp(x), F29::from_fp(y)))); break;
        case 14: {   // lazy chain at the documented limb bounds: ((x - y + 12M) * (x + y)) with un-normalized operands
            L29 a = F29::from_fp(x), b = F29::from_fp(y);
            L29 d = F29::template sub<12>(a, b);                 // limbs < 2^31
            L29 sum = F29::add(a, b);                            // limbs < 2^30
            L29 p = F29::mul(F29::norm(d), sum);                 // normalized x lazy sum
            L29 q = F29::mul(d, F29::to_261(F29::from_fp(y)));   // lazy difference x normalized
            L29 t = F29::template sub<4>(F29::add(p, p), q);     // 2p - q, lazy
            r = F29::to_fp(F29::canon(F29::to_256(t)));
        } break;
        case 15: r = F29::to_fp(F29::canon(F29::to_256(F29::to_261(F29::from_fp(x))))); break;   // 256 -> 261 -> 256
        case 16: { L29 t = F29::add(F29::from_fp(x), F29::from_fp(y)); r = F29::to_fp(F29::canon(F29::sqr(t))); } break;      // dedicated squaring, lazy operand
        case 17: { L29 t = F29::add(F29::from_fp(x), F29::from_fp(y)); r = F29::to_fp(F29::canon(F29::mul(t, t))); } break;   // ... against the general product
        case 18: {   // x - 3y through the three-subtrahend offset (the -X3 step of ec29.hpp)
            L29 a = F29::from_fp(x), b = F29::from_fp(y), t;
            for (int k = 0; k < 9; ++k) t.l[k] = a.l[k] + F29::Cfg::OFF4T3[k] - 2 * b.l[k] - b.l[k];
            r = F29::to_fp(F29::canon(t));
        } break;
        case 19: r = F29::to_fp(F29::canon(F29::sub_off(F29::from_fp(x), F29::from_fp(y), F29::Cfg::OFF2T1))); break;
        case 20: {   // dual product with one reduction: x*y + (x + y)*x (2^256-form), second pair lazy
            L29 a = F29::from_fp(x), b = F29::from_fp(y);
            r = F29::to_fp(F29::canon(F29::mul2(a, F29::to_261(b), F29::add(a, b), F29::to_261(a))));
        } break;
        // 21..23: the plain C++ products (ops 10, 16, 20 run the generated assembly chains)
        case 21: r = F29::to_fp(F29::canon(F29::mul_cpp(F29::from_fp(x), F29::to_261(F29::from_fp(y))))); break;
        case 22: { L29 t = F29::add(F29::from_fp(x), F29::from_fp(y)); r = F29::to_fp(F29::canon(F29::sqr_cpp(t))); } break;
        case 23: {
            L29 a = F29::from_fp(x), b = F29::from_fp(y);
            r = F29::to_fp(F29::canon(F29::mul2_cpp(a, F29::to_261(b), F29::add(a, b), F29::to_261(a))));
        } break;
        // the constant-operand product (fp29.hpp mulc): y canonical, x any 256-bit value; out = x * y mod M as PLAIN integers
        case 24: { const L29 w = F29::from_fp(y); r = F29::to_fp(F29::canon(F29::mulc(F29::from_fp(x), w, F29::wq_of(w)))); } break;
        // ... with a lazy first operand near the limb bound: 2 (x + 4M) as limb-wise sums (limbs < 2^31.7, value < 19M)
        case 25: {
            const L29 w = F29::from_fp(y);
            L29 t = F29::add(F29::from_fp(x), F29::constant(F29::Cfg::OFF4));
            t = F29::add(t, t);
            r = F29::to_fp(F29::canon(F29::mulc(t, w, F29::wq_of(w))));
        } break;
        // wq_of(y) itself, low 256 bits (floor(y 2^261 / M) mod 2^256)
        case 26: r = F29::to_fp(F29::wq_of(F29::from_fp(y))); break;
        // reduce3 of the lazy sum x + y + 4M (x, y any 256-bit values: limbs < 2^31.4, value < 14.6M for Fr and Fq), RAW: the caller
        // checks the residue and the bound value < 3M
        case 27: r = F29::to_fp(F29::reduce3(F29::add(F29::add(F29::from_fp(x), F29::from_fp(y)), F29::constant(F29::Cfg::OFF4)))); break;
        // ---- the typed lazy arithmetic (lz29.hpp) and its two free conversions; x, y canonical wire elements -----------------
        // 28: re-limb at bit offset -5 (32 x = the 2^261-form), back by exact division by 32: the identity
        case 28: r = F::canon(F29::template to_fp_div<5>(F29::from_fp_x32(x))); break;
        // 29 / 30 / 31: x y, x - y, x y + y y through ld -> typed operation -> to_wire: the wire-form results of ops 0 / 2 and 0 + 4
        case 29: { using Z = LzOps<F29>; r = Z::to_wire(Z::mul(Z::ld(x), Z::ld(y))); } break;
        case 30: { using Z = LzOps<F29>; r = Z::to_wire(Z::norm(Z::sub(Z::ld(x), Z::ld(y)))); } break;
        case 31: { using Z = LzOps<F29>; r = Z::to_wire(Z::mul2(Z::ld(x), Z::ld(y), Z::ld(y), Z::ld(y))); } break;
        // 32: a value in 2^266-form leaves by exact division by 2^10: (x in 2^261-form) * 2^266 / 2^261 = the 2^266-form of x; -> x
        case 32: { const L29 v = F29::mul(F29::from_fp_x32(x), F29::constant(F29::Cfg::R266)); r = F::canon(F29::template to_fp_div<10>(v)); } break;
        // 33: a long lazy chain at the limb bounds: ((x + y) + (x - y)) - ((y - x) - x)  =  3 x - y  ... all typed, one carry step where the types ask
        case 33: {
            using Z = LzOps<F29>;
            const auto a1 = Z::ld(x), b1 = Z::ld(y);
            const auto s1 = Z::add(Z::add(a1, b1), Z::sub(a1, b1));                 // 2 x (+ 33 M), limbs < 6 units
            const auto s2 = Z::norm(Z::sub(Z::norm(Z::sub(b1, a1)), a1));           // y - 2 x (+ offsets)
            r = Z::to_wire(Z::mul(Z::norm(Z::sub(Z::norm(s1), s2)), Z::one()));     // (4 x - y) * 1, through a product: value back below 16 M
        } break;
        default: r = F::to_mont(x); break;
    }
    out[i] = r;
}

__global__ __launch_bounds__(256) void g1_op_kernel(int op, const Affine* __restrict__ a, const Affine* __restrict__ b,
                                                    Jac* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine p = a[i], q = b[i];
    XYZZ acc = xyzz_from_affine(p);
    switch (op) {
        case 0: xyzz_madd(acc, q, false); break;                       // mixed add
        case 1: { XYZZ t = xyzz_from_affine(q); xyzz_add(acc, t); } break;   // full add
        case 2: acc = xyzz_dbl(acc); break;                            // double
        case 3: xyzz_madd(acc, q, true); break;                        // mixed subtract
        default: {                                                      // (p + q) + (p + q) through non-trivial ZZ
            xyzz_madd(acc, q, false);
            XYZZ t = acc;
            xyzz_add(acc, t);
        } break;
    }
    out[i] = xyzz_to_jac(acc);
}

// ops 5..7: the quad addition (ecquad.hpp), four lanes per element
__global__ __launch_bounds__(256) void g1_quad_op_kernel(int op, const Affine* __restrict__ a, const Affine* __restrict__ b,
                                                         Jac* __restrict__ out, size_t n) {
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = gt >> 2;
    const uint32_t q = (uint32_t)(gt & 3);
    if (i >= n) return;
    const Affine p = a[i], r = b[i];
    XYZZ acc = xyzz_from_affine(p);
    if (op == 5) {                                   // p + r, trivial ZZ on both sides
        const XYZZ t = xyzz_from_affine(r);
        xyzz_add_quad(acc, t, q);
    } else if (op == 6) {                            // (p + r) + (p + r): the doubling branch through non-trivial ZZ
        xyzz_madd(acc, r, false);
        const XYZZ t = acc;
        xyzz_add_quad(acc, t, q);
    } else {                                         // (p + r) + (p - r) = 2p: general case, non-trivial ZZ on both sides
        XYZZ t = acc;
        xyzz_madd(acc, r, false);
        xyzz_madd(t, r, true);
        xyzz_add_quad(acc, t, q);
    }
    if (q == 0) out[i] = xyzz_to_jac(acc);
}

// ops 8..13: the same on the 29-bit-limb representation (ecquad29.hpp): 8 a + b, 9 2(a + b) through the addition's
// doubling branch, 10 (a + b) + (a - b), 11 4(a + b) by two quad doublings, 12 2(a + b) by one, 13 4a
__global__ __launch_bounds__(256) void g1_quad29_op_kernel(int op, const Affine* __restrict__ a, const Affine* __restrict__ b,
                                                           Jac* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = gt >> 2;
    const uint32_t q = (uint32_t)(gt & 3);
    if (i >= n) return;
    const Affine p = a[i], r = b[i];
    XYZZ s = xyzz_from_affine(p), t = xyzz_from_affine(r);
    X29 acc;
    if (op == 8) {
        acc = x29_from_xyzz_quad(s, q);
        x29_add_quad(acc, x29_from_xyzz_quad(t, q), q);
    } else if (op == 9) {
        xyzz_madd(s, r, false);
        acc = x29_from_xyzz_quad(s, q);
        const X29 same = acc;
        x29_add_quad(acc, same, q);
    } else if (op == 10) {
        XYZZ u = s;
        xyzz_madd(s, r, false);
        xyzz_madd(u, r, true);
        acc = x29_from_xyzz_quad(s, q);
        x29_add_quad(acc, x29_from_xyzz_quad(u, q), q);
    } else if (op == 11) {
        acc = x29_from_xyzz_quad(s, q);
        x29_add_quad(acc, x29_from_xyzz_quad(t, q), q);
        x29_dbl_quad(acc, q);
        x29_dbl_quad(acc, q);
    } else if (op == 12) {                           // 2(a + b): one doubling of an addition's result
        acc = x29_from_xyzz_quad(s, q);
        x29_add_quad(acc, x29_from_xyzz_quad(t, q), q);
        x29_dbl_quad(acc, q);
    } else {                                         // 4a: doubling of a doubling's result
        acc = x29_from_xyzz_quad(s, q);
        x29_dbl_quad(acc, q);
        x29_dbl_quad(acc, q);
    }
    const Fp mine = x29_coord_to_fp(acc, q);
    XYZZ o;
    o.x = quad_bcast<0>(mine); o.y = quad_bcast<1>(mine); o.zz = quad_bcast<2>(mine); o.zzz = quad_bcast<3>(mine);
    if (q == 0) out[i] = xyzz_to_jac(o);
#endif
}

int field_op_device(Ctx& c, int field, int op, const Fp* a, const Fp* b, Fp* out, size_t n) {
    if (n == 0) return UZK_OK;
    Fp *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t bytes = n * sizeof(Fp);
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&da), bytes));
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&db), bytes));
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&dout), bytes));
    UZK_HIP(hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, c.stream));
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (field == 0) hipLaunchKernelGGL((field_op_kernel<Fq, Fq29>), dim3(grid), dim3(256), 0, c.stream, op, da, db, dout, n);
    else hipLaunchKernelGGL((field_op_kernel<Fr, Fr29>), dim3(grid), dim3(256), 0, c.stream, op, da, db, dout, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

// ---- operands the compiler can see (uzk_test_const_operands) ----------------------------------------------------------------------
// The known-answer kernel above loads every operand from memory.  Production code also multiplies by literals (to_mont, from_mont, a
// zero Horner start, a 16-bit scalar): words the compiler KNOWS, which it may keep in one register with any other word of the same
// value -- the zero-initialised carry word of an assembly statement among them, unless the statement's constraints forbid it.  Each
// case here is one (operation, form of the first operand, form of the second) as template parameters and so a kernel of its own:
// its register allocation is that of the shape alone.  A form fixes some words as literals and loads the rest.
enum { CO_MUL, CO_MUL_RX, CO_SQR, CO_ADD, CO_SUB, CO_ADD_RX, CO_SUB_RX, CO_DBL, CO_L29_MUL, CO_L29_SQR, CO_L29_MUL2, CO_L29_MULC };
// 8 x 32-bit words: all loaded | words 0..3 loaded, 4..7 zero | word 0 loaded, 1..7 zero | R^2 | (1, 0, .., 0) | 0 | one() | M - 1;
// 9 x 29-bit limbs (of the loaded words): limbs 0..4 loaded, 5..8 zero | limb 0 loaded, 1..8 zero | LzOps::one()
enum { CF_RT, CF_LO4, CF_W0, CF_R2, CF_E1, CF_ZERO, CF_ONE, CF_MM1, CF_L5, CF_L1, CF_ONE261 };

#define CO_PRODUCT_CASES(X, OP) \
    X(OP, CF_LO4, CF_R2) X(OP, CF_R2, CF_LO4) X(OP, CF_W0, CF_RT) X(OP, CF_RT, CF_W0) X(OP, CF_RT, CF_E1) X(OP, CF_RT, CF_ZERO) \
    X(OP, CF_RT, CF_ONE) X(OP, CF_R2, CF_ONE) X(OP, CF_MM1, CF_MM1) X(OP, CF_LO4, CF_LO4)
#define CO_SUM_CASES(X, OP) \
    X(OP, CF_RT, CF_ZERO) X(OP, CF_RT, CF_ONE) X(OP, CF_RT, CF_MM1) X(OP, CF_ZERO, CF_RT) X(OP, CF_ONE, CF_RT) X(OP, CF_MM1, CF_RT)
#define CO_CASES(X) \
    CO_PRODUCT_CASES(X, CO_MUL) CO_PRODUCT_CASES(X, CO_MUL_RX) \
    X(CO_SQR, CF_LO4, CF_LO4) X(CO_SQR, CF_W0, CF_W0) X(CO_SQR, CF_R2, CF_R2) X(CO_SQR, CF_MM1, CF_MM1) \
    CO_SUM_CASES(X, CO_ADD) CO_SUM_CASES(X, CO_SUB) CO_SUM_CASES(X, CO_ADD_RX) CO_SUM_CASES(X, CO_SUB_RX) \
    X(CO_DBL, CF_ZERO, CF_ZERO) X(CO_DBL, CF_ONE, CF_ONE) X(CO_DBL, CF_MM1, CF_MM1) X(CO_DBL, CF_LO4, CF_LO4) X(CO_DBL, CF_W0, CF_W0) \
    X(CO_L29_MUL, CF_L5, CF_RT) X(CO_L29_MUL, CF_RT, CF_L5) X(CO_L29_MUL, CF_L1, CF_RT) X(CO_L29_MUL, CF_RT, CF_L1) \
    X(CO_L29_MUL, CF_L5, CF_L5) X(CO_L29_MUL, CF_RT, CF_ONE261) X(CO_L29_MUL, CF_ONE261, CF_RT) X(CO_L29_MUL, CF_L1, CF_ONE261) \
    X(CO_L29_SQR, CF_L5, CF_L5) X(CO_L29_SQR, CF_L1, CF_L1) X(CO_L29_SQR, CF_ONE261, CF_ONE261) \
    X(CO_L29_MUL2, CF_L5, CF_RT) X(CO_L29_MUL2, CF_RT, CF_L5) X(CO_L29_MUL2, CF_L1, CF_RT) X(CO_L29_MUL2, CF_RT, CF_L1) \
    X(CO_L29_MUL2, CF_RT, CF_ONE261) \
    X(CO_L29_MULC, CF_L5, CF_RT) X(CO_L29_MULC, CF_L1, CF_RT) X(CO_L29_MULC, CF_RT, CF_L5) X(CO_L29_MULC, CF_RT, CF_L1) \
    X(CO_L29_MULC, CF_RT, CF_ONE261)

#if defined(__HIP_DEVICE_COMPILE__)
template <class F> struct CoCfgOf;
template <class C> struct CoCfgOf<Field<C>> { using type = C; };
template <class F, int FORM>
__device__ __forceinline__ Fp co_words(const Fp& x) {
    using C = typename CoCfgOf<F>::type;
    Fp r;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if constexpr (FORM == CF_RT) r.v[k] = x.v[k];
        else if constexpr (FORM == CF_LO4) r.v[k] = k < 4 ? x.v[k] : 0u;
        else if constexpr (FORM == CF_W0) r.v[k] = k < 1 ? x.v[k] : 0u;
        else if constexpr (FORM == CF_R2) r.v[k] = C::R2[k];
        else if constexpr (FORM == CF_E1) r.v[k] = k == 0 ? 1u : 0u;
        else if constexpr (FORM == CF_ZERO) r.v[k] = 0u;
        else if constexpr (FORM == CF_ONE) r.v[k] = C::R1[k];
        else r.v[k] = C::M[k] - (k == 0 ? 1u : 0u);                  // M is odd: no borrow
    }
    return r;
}
template <class F29, int FORM>
__device__ __forceinline__ L29 co_limbs(const Fp& x) {
    if constexpr (FORM == CF_ONE261) return F29::constant(F29::Cfg::ONE261);
    L29 r = F29::from_fp(x);
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if ((FORM == CF_L5 && k >= 5) || (FORM == CF_L1 && k >= 1)) r.l[k] = 0u;
    return r;
}
#endif

template <class F, class F29, int OP, int FA, int FB, bool PORTABLE>
__global__ __launch_bounds__(256) void const_operand_kernel(const Fp* __restrict__ a, const Fp* __restrict__ b, Fp* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    // a grid-stride loop although the launch gives every lane one element: the literals are then set up outside the loop, as in the
    // production kernels that loop after their product, and that is where the compiler was seen to merge them with the carry word
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Fp r;
    if constexpr (OP >= CO_L29_MUL) {
        const L29 x = co_limbs<F29, FA>(a[i]), y = co_limbs<F29, FB>(b[i]);
        L29 t;
        if constexpr (OP == CO_L29_MUL) t = PORTABLE ? F29::mul_cpp(x, y) : F29::mul(x, y);
        else if constexpr (OP == CO_L29_SQR) t = PORTABLE ? F29::sqr_cpp(x) : F29::sqr(x);
        else if constexpr (OP == CO_L29_MUL2) t = PORTABLE ? F29::mul2_cpp(x, y, x, x) : F29::mul2(x, y, x, x);                // x y + x x
        // the constant-operand product has no C++ form: x y as (x y 2^-261) 2^522 2^-261 by two C++ products
        else t = PORTABLE ? F29::mul_cpp(F29::mul_cpp(x, y), F29::constant(F29::Cfg::R522)) : F29::mulc(x, y, F29::wq_of(y));
        r = F29::to_fp(F29::canon(t));
    } else {
        const Fp x = co_words<F, FA>(a[i]), y = co_words<F, FB>(b[i]);
        if constexpr (OP == CO_MUL) r = PORTABLE ? F::mul_portable(x, y) : F::mul(x, y);
        else if constexpr (OP == CO_MUL_RX) r = PORTABLE ? F::mul_portable(x, y) : F::canon(F::mul_rx(x, y));
        else if constexpr (OP == CO_SQR) r = PORTABLE ? F::mul_portable(x, x) : F::sqr(x);
        else if constexpr (OP == CO_ADD) r = PORTABLE ? F::add_portable(x, y) : F::add(x, y);
        else if constexpr (OP == CO_SUB) r = PORTABLE ? F::sub_portable(x, y) : F::sub(x, y);
        else if constexpr (OP == CO_ADD_RX) r = PORTABLE ? F::add_portable(x, y) : F::canon(F::add_rx(x, y));
        else if constexpr (OP == CO_SUB_RX) r = PORTABLE ? F::sub_portable(x, y) : F::canon(F::sub_rx(x, y));
        else r = PORTABLE ? F::add_portable(x, x) : F::dbl(x);
    }
    out[i] = r;
    }
#endif
}

template <int OP, int FA, int FB>
static void const_operand_launch(Ctx& c, int field, bool portable, const Fp* da, const Fp* db, Fp* dout, size_t n) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (field == 0 && !portable) hipLaunchKernelGGL((const_operand_kernel<Fq, Fq29, OP, FA, FB, false>), grid, block, 0, c.stream, da, db, dout, n);
    else if (field == 0) hipLaunchKernelGGL((const_operand_kernel<Fq, Fq29, OP, FA, FB, true>), grid, block, 0, c.stream, da, db, dout, n);
    else if (!portable) hipLaunchKernelGGL((const_operand_kernel<Fr, Fr29, OP, FA, FB, false>), grid, block, 0, c.stream, da, db, dout, n);
    else hipLaunchKernelGGL((const_operand_kernel<Fr, Fr29, OP, FA, FB, true>), grid, block, 0, c.stream, da, db, dout, n);
}

bool const_operand_case_known(int op, int form_a, int form_b) {
#define CO_KNOWN(o, fa, fb) if (op == o && form_a == fa && form_b == fb) return true;
    CO_CASES(CO_KNOWN)
#undef CO_KNOWN
    return false;
}

int const_operand_device(Ctx& c, int field, int op, int form_a, int form_b, bool portable, const Fp* a, const Fp* b, Fp* out, size_t n) {
    if (n == 0) return UZK_OK;
    Fp *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t bytes = n * sizeof(Fp);
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&da), bytes));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&db), bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
#define CO_RUN(o, fa, fb) if (op == o && form_a == fa && form_b == fb) const_operand_launch<o, fa, fb>(c, field, portable, da, db, dout, n);
        CO_CASES(CO_RUN)
#undef CO_RUN
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

// ops 14..21: the additions of ec29l.hpp (lazy 29-bit limbs, operands re-limbed from the wire form, bounds in the types).
// one lane per element: 14 a + b, 15 2(a + b) through the addition's doubling branch, 16 (a + b) + (a - b) (non-trivial ZZ on both
// sides), 17 (a + b) - (a + b) = infinity (cancellation) ... then + a; four lanes per element: 18..21 the same four by quads.
__global__ __launch_bounds__(256) void g1_p29_op_kernel(int op, const Affine* __restrict__ a, const Affine* __restrict__ b,
                                                        Jac* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const bool quad = op >= 18;
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = quad ? gt >> 2 : gt;
    const uint32_t q = (uint32_t)(gt & 3);
    const bool live = i < n;                             // no early return: the quad path below has a barrier
    const int f = quad ? op - 18 : op - 14;
    auto add = [&](P29& x, const P29& y) { if (quad) p29_add_quad(x, y, q); else p29_add(x, y); };
    P29 acc = p29_inf();
    if (live) {
        const Affine p = a[i], r = b[i];
        XYZZ s = xyzz_from_affine(p), t = xyzz_from_affine(r);
        if (f == 0) {
            acc = p29_load(s);
            add(acc, p29_load(t));
        } else if (f == 1) {
            xyzz_madd(s, r, false);
            acc = p29_load(s);
            const P29 same = acc;
            add(acc, same);
        } else if (f == 2) {
            XYZZ u = s;
            xyzz_madd(s, r, false);
            xyzz_madd(u, r, true);
            acc = p29_load(s);
            add(acc, p29_load(u));
        } else {
            XYZZ u = s;
            xyzz_madd(u, r, false);                          // a + b
            XYZZ v = u;
            v.y = Fq::neg(v.y);                              // -(a + b), same ZZ / ZZZ
            acc = p29_load(u);
            add(acc, p29_load(v));                           // infinity
            add(acc, p29_load(s));                           // + a
            P29 w = p29_load(t);
            add(w, p29_inf());                               // b + infinity
            add(acc, w);                                     // a + b
        }
    }
    if (quad) {
        const Fp c = !live || p29_is_inf(acc) ? Fq::zero() : p29_coord_to_fp(acc, q);
        __shared__ Fp sh[64][4];
        sh[threadIdx.x >> 2][q] = c;
        __syncthreads();
        if (live && q == 0) {
            XYZZ o;
            o.x = sh[threadIdx.x >> 2][0]; o.y = sh[threadIdx.x >> 2][1]; o.zz = sh[threadIdx.x >> 2][2]; o.zzz = sh[threadIdx.x >> 2][3];
            out[i] = xyzz_to_jac(o);
        }
    } else if (live) {
        out[i] = xyzz_to_jac(p29_store(acc));
    }
#endif
}

// ---- raw 9-limb known-answer entry points (uzk_test_l29_kat, uzk_test_p29_kat) -------------------------------------------------
// The primitives of fp29.hpp and the typed operations of lz29.hpp applied to limbs EXACTLY as given (no re-limbing, no canon on the
// way out), so that tests can drive every operation to the edges of its stated contract and check the raw result against it.
// Record i of `in` holds four operands a, b, c, d of 9 limbs each; out[i] is the raw result (8-word results in l[0..7], l[8] = 0).
#define LZ29_FIELD_FQ 0
#define LZ29_FIELD_FR 1
#define LZ29_TYPE_FQ Fq29
#define LZ29_TYPE_FR Fr29
enum { LZ29_KIND_add, LZ29_KIND_sub, LZ29_KIND_mul, LZ29_KIND_sqr, LZ29_KIND_mul2, LZ29_KIND_norm, LZ29_KIND_assume, LZ29_KIND_canon,
       LZ29_KIND_to_wire };
struct Lz29SigInfo { int field, kind; };
static const Lz29SigInfo kLz29Sigs[] = {
#define LZ29_SIG(idx, fld, op, ar, ka, va, kb, vb, kc, vc, kd, vd, kr, vr) {LZ29_FIELD_##fld, LZ29_KIND_##op},
#include "lz29_sigs.inc"
#undef LZ29_SIG
};
// the typed operations whose code depends on the type parameters: sub (its Off29 constant), to_wire (its branch), canon
bool l29_sig_runnable(int field, uint32_t idx) {
    if (idx >= sizeof(kLz29Sigs) / sizeof(kLz29Sigs[0])) return false;
    const Lz29SigInfo& s = kLz29Sigs[idx];
    return s.field == field && (s.kind == LZ29_KIND_sub || s.kind == LZ29_KIND_to_wire || s.kind == LZ29_KIND_canon);
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ L29 l29_words(const Fp& w) {
    L29 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.l[k] = w.v[k];
    r.l[8] = 0;
    return r;
}
template <class F, int Ka, int Va, int Kb, int Vb> __device__ __forceinline__ L29 sig_sub(const L29& a, const L29& b) {
    Lz<F, Ka, Va> x; Lz<F, Kb, Vb> y; x.v = a; y.v = b;
    return LzOps<F>::sub(x, y).v;
}
template <class F, int K, int V> __device__ __forceinline__ L29 sig_to_wire(const L29& a) { Lz<F, K, V> x; x.v = a; return l29_words(LzOps<F>::to_wire(x)); }
template <class F, int K, int V> __device__ __forceinline__ L29 sig_canon(const L29& a) { Lz<F, K, V> x; x.v = a; return l29_words(LzOps<F>::canon(x)); }
#endif

template <class F>
__global__ __launch_bounds__(256) void l29_op_kernel(int op, uint32_t param, const L29* __restrict__ in, L29* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const L29 a = in[4 * i], b = in[4 * i + 1], c = in[4 * i + 2], d = in[4 * i + 3];
    L29 r = F::zero();
    switch (op) {
        case 0: r = F::mul(a, b); break;
        case 1: r = F::sqr(a); break;
        case 2: r = F::mul2(a, b, c, d); break;
        case 3: r = F::mul_cpp(a, b); break;
        case 4: r = F::sqr_cpp(a); break;
        case 5: r = F::mul2_cpp(a, b, c, d); break;
        case 6: r = F::mulc(a, b, F::wq_of(b)); break;                               // b: canonical plain w
        case 7: {                                                                     // one wave-uniform w: record 0's b
            const L29 w = F::uniform(in[1]);
            r = F::mulcs(a, w, F::uniform(F::wq_of(w)));
        } break;
        case 8: r = F::add(a, b); break;
        case 9: r = F::norm(a); break;
        case 10: r = F::norm1(a); break;
        case 11: r = F::reduce(a); break;
        case 12: r = F::reduce3(a); break;
        case 13: r = F::canon(a); break;
        case 14: r = l29_words(F::to_fp(a)); break;
        case 15: r = l29_words(F::template to_fp_div<5>(a)); break;
        case 16: r = l29_words(F::template to_fp_div<10>(a)); break;
        case 17: r = F::template sub<4>(a, b); break;
        case 18: r = F::template sub<8>(a, b); break;
        case 19: r = F::template sub<12>(a, b); break;
        case 20: {                                                                    // sub_off with the named offset `param`
            using C = typename F::Cfg;
            switch (param) {
                case 0: r = F::sub_off(a, b, C::OFF4); break;
                case 1: r = F::sub_off(a, b, C::OFF8); break;
                case 2: r = F::sub_off(a, b, C::OFF12); break;
                case 3: r = F::sub_off(a, b, C::OFF4T3); break;
                case 4: r = F::sub_off(a, b, C::OFF2T1); break;
                default: r = F::sub_off(a, b, C::OFF8T1); break;
            }
        } break;
        case 21: {                                                                    // the inventoried typed signature `param`
            switch (param) {
#define LZ29_RUN(fld, body) if constexpr (std::is_same<F, LZ29_TYPE_##fld>::value) { r = body; }
#define LZ29_RUN_sub(idx, fld, ka, va, kb, vb) case idx: LZ29_RUN(fld, (sig_sub<F, ka, va, kb, vb>(a, b))) break;
#define LZ29_RUN_to_wire(idx, fld, ka, va, kb, vb) case idx: LZ29_RUN(fld, (sig_to_wire<F, ka, va>(a))) break;
#define LZ29_RUN_canon(idx, fld, ka, va, kb, vb) case idx: LZ29_RUN(fld, (sig_canon<F, ka, va>(a))) break;
#define LZ29_RUN_add(...)
#define LZ29_RUN_mul(...)
#define LZ29_RUN_sqr(...)
#define LZ29_RUN_mul2(...)
#define LZ29_RUN_norm(...)
#define LZ29_RUN_assume(...)
#define LZ29_SIG(idx, fld, op, ar, ka, va, kb, vb, kc, vc, kd, vd, kr, vr) LZ29_RUN_##op(idx, fld, ka, va, kb, vb)
#include "lz29_sigs.inc"
#undef LZ29_SIG
                default: break;
            }
        } break;
        case 22: r = F::reduce(F::from_fp_x32(*reinterpret_cast<const Fp*>(&a))); break;   // acc29_set's step: a.l[0..7] are wire words
        default: break;
    }
    out[i] = r;
#endif
}

int l29_op_device(Ctx& c, int field, int op, uint32_t param, const uint32_t* in, uint32_t* out, size_t n) {
    if (n == 0) return UZK_OK;
    L29 *din = nullptr, *dout = nullptr;
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&din), 4 * n * sizeof(L29)));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dout), n * sizeof(L29));
    if (e == hipSuccess) e = hipMemcpyAsync(din, in, 4 * n * sizeof(L29), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)((n + 255) / 256);
        if (field == 0) hipLaunchKernelGGL(l29_op_kernel<Fq29>, dim3(grid), dim3(256), 0, c.stream, op, param, din, dout, n);
        else hipLaunchKernelGGL(l29_op_kernel<Fr29>, dim3(grid), dim3(256), 0, c.stream, op, param, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(L29), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

// ec29l.hpp's additions on raw coordinate limbs: record i of `in` is two P29 (a, then b: x, y, zz, zzz), out[i] the raw P29 result.
// op 0 a + b (p29_add), 1 2a (p29_dbl), 2 / 3 the same by the four lanes of a quad (lane 0's result).
__global__ __launch_bounds__(256) void p29_op_kernel(int op, const P29* __restrict__ in, P29* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const bool quad = op >= 2;
    const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = quad ? gt >> 2 : gt;
    const uint32_t q = (uint32_t)(gt & 3);
    if (i >= n) return;                              // whole quads leave together (4 n threads, blocks of 256); no barrier below
    P29 acc = in[2 * i];
    const P29 p = in[2 * i + 1];
    if (op == 0) p29_add(acc, p);
    else if (op == 1) p29_dbl(acc);
    else if (op == 2) p29_add_quad(acc, p, q);
    else p29_dbl_quad(acc, q);
    if (!quad || q == 0) out[i] = acc;
#endif
}

int p29_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (n == 0) return UZK_OK;
    P29 *din = nullptr, *dout = nullptr;
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&din), 2 * n * sizeof(P29)));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dout), n * sizeof(P29));
    if (e == hipSuccess) e = hipMemcpyAsync(din, in, 2 * n * sizeof(P29), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
        const size_t threads = op >= 2 ? 4 * n : n;
        hipLaunchKernelGGL(p29_op_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c.stream, op, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(P29), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

int g1_op_device(Ctx& c, int op, const Affine* a, const Affine* b, Jac* out, size_t n) {
    if (n == 0) return UZK_OK;
    Affine *da = nullptr, *db = nullptr;
    Jac* dout = nullptr;
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&da), n * sizeof(Affine)));
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&db), n * sizeof(Affine)));
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&dout), n * sizeof(Jac)));
    UZK_HIP(hipMemcpyAsync(da, a, n * sizeof(Affine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(db, b, n * sizeof(Affine), hipMemcpyHostToDevice, c.stream));
    if (op >= 18) hipLaunchKernelGGL(g1_p29_op_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, c.stream, op, da, db, dout, n);
    else if (op >= 14) hipLaunchKernelGGL(g1_p29_op_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, op, da, db, dout, n);
    else if (op >= 8) hipLaunchKernelGGL(g1_quad29_op_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, c.stream, op, da, db, dout, n);
    else if (op >= 5) hipLaunchKernelGGL(g1_quad_op_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, c.stream, op, da, db, dout, n);
    else hipLaunchKernelGGL(g1_op_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, op, da, db, dout, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(Jac), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

}  // namespace uzk
