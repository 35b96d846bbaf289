// NTT over G1: the elements are curve points, the twiddles scalars of Fr (arkworks' EvaluationDomain::{fft, ifft} over
// Vec<G1Projective>).  inverse(monomial SRS) = Lagrange SRS: the bases of every commit of the round API, derived on the device
// for any n = 2^k instead of being read from one of the reference's three files.
//
//   g1ntt_load     affine wire points -> P29 (ec29l.hpp) at the bit-reversed index of a working array (144 B per point)
//   g1ntt_stage    one radix-2 decimation-in-time stage in place: (A, B) -> (A + w B, A - w B), one launch per stage
//   g1ntt_scale    inverse only: every point times 1 / n
//   g1ntt_affine   P29 -> affine wire points, one inversion per run of kAffineRun points (Montgomery's trick)
//
// A butterfly is one scalar multiplication by a 254-bit twiddle and two complete additions; it moves 432 B and costs about 10^5
// vector instructions, so the stages are bound by instruction issue and nothing is tiled through the LDS.  What the LDS holds is
// the table of the scalar multiplication: fixed 4-bit windows with signed digits (-8 .. 8), so that every lane of a wave adds at
// the same 64 places whatever its twiddle is -- with plain or NAF double-and-add the lanes of a wave have different twiddles and
// the wave pays an addition at (almost) every bit.  252 doublings + 64 additions + 7 group operations for the table {B .. 8 B}.
// The digits of the twiddles are constants of the domain: computed once per n on the host, cached in the context (one table
// serves both directions: w^-j = -w^(n/2 - j)).
//
// Every group operation is done by the four lanes of a quad (p29_add_quad / p29_dbl_quad): a stage of n = 2^14 is 8 192
// butterflies -- 128 waves for 1 024 SIMDs with one lane per butterfly, 512 with a quad -- and a quad shares ONE table, 1 152 B,
// where four lanes with a butterfly each would need four (a wave's tables: 74 KB of the CU's 160 KB).  See DESIGN.md.
//
// Complete: inputs and outputs may be infinity, w * infinity = infinity, an accumulator that is still infinity takes the table
// entry, equal and opposite operands of an addition double and cancel (p29_add_quad).
#include <cstdio>
#include <cstring>

#include "ctx.hpp"
#include "ec29l.hpp"
#include "host_math.hpp"
#include "lane_tools.hpp"

namespace uzk {

constexpr int kG1Windows = 64;        // 4-bit windows of a 254-bit scalar (the top one holds two bits and a carry: <= 4)
constexpr int kG1Block = 64;          // threads of a stage workgroup: 16 quads
constexpr int kG1Quads = kG1Block / 4;
constexpr int kG1EntryWords = 36;     // a table entry: x, y, zz, zzz
constexpr int kAffineRun = 16;
static_assert(8 * kG1EntryWords * kG1Quads * 4 <= 64 * 1024, "the quads' tables fit a workgroup's LDS");

// digits d[i] in [-8, 8] with s = sum d[i] 16^i, for a canonical s < 2^254
static void signed_digits(const Fp& s, int8_t* d) {
    int carry = 0;
    for (int i = 0; i < kG1Windows; ++i) {
        int v = (int)((s.v[i >> 3] >> ((i & 7) * 4)) & 15) + carry;
        carry = v > 8;
        d[i] = (int8_t)(carry ? v - 16 : v);
    }
}

struct G1NttPlan {
    uint32_t* d_digits = nullptr;     // (n / 2 + 1) rows of 16 words: the digits of w^j, j < n / 2; the last row: (r - 1) / n
    bool scale_negate = true;         // 1 / n = -((r - 1) / n): a scalar that is log2 n bits shorter
};

__device__ __forceinline__ uint32_t bitrev(uint32_t i, uint32_t logn) { return logn ? __brev(i) >> (32 - logn) : 0; }

__global__ __launch_bounds__(256) void g1ntt_load_kernel(const Affine* __restrict__ in, P29* __restrict__ work, uint32_t n, uint32_t logn) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    work[bitrev(i, logn)] = p29_load(xyzz_from_affine(in[i]));
}

#if defined(__HIP_DEVICE_COMPILE__)
namespace g1n {
using namespace p29;
// A coordinate brought under 2 M by two products by 1 (x 2^261 stays x 2^261), and its negative as a limb-wise subtraction and one
// carry step (below 6 M: a P29 coordinate again).  Both products, the subtraction and the carry step are signatures the MSM's
// additions already instantiate (lz29_sigs.inc): the transform adds none to the inventory.
using Ty = Lz<Fq29, 1, 2>;
__device__ __forceinline__ Ty tight(const L29& y) {
    const auto t = Z::mul(co(y), Z::template relax<1, 32>(Z::one()));                     // < 8 M
    return Z::mul(t, Z::template relax<1, 2>(Z::one()));
}
__device__ __forceinline__ Co neg_tight(const Ty& y) {
    return Z::template relax<1, 32>(Z::norm(Z::template relax<4, 6>(Z::sub(Z::zero(), y))));
}
__device__ __forceinline__ L29 neg_coord(const L29& y) { return neg_tight(tight(y)).v; }
// the quad's table in the LDS: word w of entry e at ((e * 36 + w) * 16 + quad): the 16 quads of a workgroup hit 16 banks whatever
// entries they read, the four lanes of a quad read one address.  Every lane writes every word it later reads (the four lanes hold
// the same values), so no lane depends on another's store.
__device__ __forceinline__ void put(uint32_t* tab, uint32_t e, uint32_t c, const L29& v) {
#pragma unroll
    for (int k = 0; k < 9; ++k) tab[((e * kG1EntryWords + c * 9 + k) * kG1Quads)] = v.l[k];
}
__device__ __forceinline__ L29 get(const uint32_t* tab, uint32_t e, uint32_t c) {
    L29 r;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.l[k] = tab[((e * kG1EntryWords + c * 9 + k) * kG1Quads)];
    return r;
}
// An entry's y is stored tight (value < 2 M), so that -y costs no product at the place of use.
__device__ __forceinline__ void put_point(uint32_t* tab, uint32_t e, const P29& p) {
    put(tab, e, 0, p.x); put(tab, e, 1, tight(p.y).v); put(tab, e, 2, p.zz); put(tab, e, 3, p.zzz);
}
__device__ __forceinline__ P29 get_point(const uint32_t* tab, uint32_t e, bool negate) {
    P29 r;
    Ty y;
    y.v = get(tab, e, 1);
    const Co ny = neg_tight(y);
    r.x = get(tab, e, 0); r.zz = get(tab, e, 2); r.zzz = get(tab, e, 3);
#pragma unroll
    for (int k = 0; k < 9; ++k) r.y.l[k] = negate ? ny.v.l[k] : y.v.l[k];
    return r;
}

// s * b by the quad; digits: the 16 words of s's signed digits; negate: -s * b.  b is not infinity.
__device__ __forceinline__ P29 scalar_mul_quad(const P29& b, const uint32_t* __restrict__ digits, bool negate, uint32_t* tab, uint32_t q) {
    put_point(tab, 0, b);
#pragma unroll 1
    for (uint32_t e = 2; e <= 8; ++e) {                            // entry e - 1 = e b: 2 b, 2 b + b, 2 (2 b), 4 b + b, 2 (3 b), 6 b + b, 2 (4 b)
        P29 p = get_point(tab, (e & 1) ? e - 2 : e / 2 - 1, false);
        if (e & 1) p29_add_quad(p, b, q);
        else p29_dbl_quad(p, q);
        put_point(tab, e - 1, p);
    }
    P29 acc = p29_inf();
    uint32_t word = digits[15];
#pragma unroll 1
    for (int wi = 15; wi >= 0; --wi) {
        const uint32_t next = digits[wi > 0 ? wi - 1 : 0];         // asked for a window group ahead
#pragma unroll 1
        for (int k = 3; k >= 0; --k) {
            if (!p29_is_inf(acc)) {
#pragma unroll 1
                for (int t = 0; t < 4; ++t) p29_dbl_quad(acc, q);
            }
            const int d = (int)(int8_t)(word >> (8 * k));
            if (d != 0) {
                const P29 p = get_point(tab, (uint32_t)(d < 0 ? -d : d) - 1, (d < 0) != negate);
                p29_add_quad(acc, p, q);
            }
        }
        word = next;
    }
    return acc;
}
__device__ __forceinline__ void store_coord(P29* dst, const P29& p, uint32_t q) {      // lane q of the quad writes coordinate q
    const L29 v = qsel(q, co(p.x), co(p.y), co(p.zz), co(p.zzz)).v;
    L29* o = q == 0 ? &dst->x : q == 1 ? &dst->y : q == 2 ? &dst->zz : &dst->zzz;
    *o = v;
}
}  // namespace g1n
#endif

// Stage with blocks of 2 m points, m = 2^mlog: butterfly (j, t), t < m, on work[2 m j + t] and work[2 m j + t + m] with the twiddle
// w^(t n / 2m) (inverse: its inverse).  t = 0 (and so the whole first stage) multiplies by 1.
__global__ __launch_bounds__(kG1Block) void g1ntt_stage_kernel(P29* __restrict__ work, const uint32_t* __restrict__ digits, uint32_t n, uint32_t logn,
                                                               uint32_t mlog, int inverse) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t tab_all[8 * kG1EntryWords * kG1Quads];
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = gt >> 2, q = gt & 3;
    if (b >= n / 2) return;                                          // whole quads leave together; no barrier below
    uint32_t* tab = tab_all + (threadIdx.x >> 2);
    const uint32_t t = b & ((1u << mlog) - 1), j = b >> mlog;
    P29* pa = work + ((size_t)j << (mlog + 1)) + t;
    P29* pb = pa + ((size_t)1 << mlog);
    P29 B = *pb;
    if (t != 0 && !p29_is_inf(B)) {
        const uint32_t step = t << (logn - 1 - mlog);                // w^step, step < n / 2
        const uint32_t row = inverse ? n / 2 - step : step;          // w^-step = -w^(n / 2 - step)
        B = g1n::scalar_mul_quad(B, digits + (size_t)row * 16, inverse != 0, tab, q);
    }
    P29 A = *pa, S = A;
    p29_add_quad(S, B, q);
    B.y = g1n::neg_coord(B.y);
    p29_add_quad(A, B, q);
    g1n::store_coord(pa, S, q);
    g1n::store_coord(pb, A, q);
#endif
}

// work[i] = (negate ? -s : s) * work[i], the digits of s in `digits`
__global__ __launch_bounds__(kG1Block) void g1ntt_scale_kernel(P29* __restrict__ work, const uint32_t* __restrict__ digits, uint32_t n, int negate) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t tab_all[8 * kG1EntryWords * kG1Quads];
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = gt >> 2, q = gt & 3;
    if (i >= n) return;
    P29 p = work[i];
    if (p29_is_inf(p)) return;
    p = g1n::scalar_mul_quad(p, digits, negate != 0, tab_all + (threadIdx.x >> 2), q);
    g1n::store_coord(work + i, p, q);
#endif
}

// x = X / ZZ, y = Y / ZZZ with 1 / ZZ = (ZZ / ZZZ)^2 (ZZ^3 = ZZZ^2): one inversion of the product of the run's ZZZ, in the wire's
// arithmetic (lane_tools.hpp; one per run of kAffineRun points).
// prefix[i]: the product of the ZZZ of the run's points before i (infinity contributes 1).
__global__ __launch_bounds__(64) void g1ntt_affine_kernel(const P29* __restrict__ work, Fp* __restrict__ prefix, Affine* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = (uint64_t)t * kAffineRun;
    if (lo >= n) return;
    const uint32_t hi = (uint32_t)(lo + kAffineRun < n ? lo + kAffineRun : n);
    Fp prod = Fq::one();
    for (uint32_t i = (uint32_t)lo; i < hi; ++i) {
        prefix[i] = prod;
        const P29 p = work[i];
        if (!p29_is_inf(p)) prod = Fq::mul(prod, p29_store(p).zzz);
    }
    Fp inv = fq_inv_lane(prod);
    for (uint32_t i = hi; i-- > (uint32_t)lo;) {
        const P29 p = work[i];
        Affine a;
        if (p29_is_inf(p)) { a.x = Fq::zero(); a.y = Fq::zero(); out[i] = a; continue; }
        const XYZZ w = p29_store(p);
        const Fp zi = Fq::mul(inv, prefix[i]);                       // 1 / ZZZ_i
        inv = Fq::mul(inv, w.zzz);
        const Fp zz_inv = Fq::sqr(Fq::mul(zi, w.zz));
        a.x = Fq::mul(w.x, zz_inv);
        a.y = Fq::mul(w.y, zi);
        out[i] = a;
    }
}

static int g1ntt_plan(Ctx& c, uint64_t n, G1NttPlan** out) {
    auto it = c.g1ntt_plans.find(n);
    if (it != c.g1ntt_plans.end()) { *out = static_cast<G1NttPlan*>(it->second); return UZK_OK; }
    const size_t rows = (size_t)(n / 2) + 1;
    std::vector<uint32_t> h(rows * 16);
    const Fp w = fr_root_of_unity(n);
    Fp cur = Fr::one();
    for (size_t j = 0; j < n / 2; ++j) {
        signed_digits(Fr::from_mont(cur), reinterpret_cast<int8_t*>(&h[j * 16]));
        cur = Fr::mul(cur, w);
    }
    {   // (r - 1) / n = -(1 / n) mod r
        const Fp ninv = fr_inv(fr_from_u64(n));
        signed_digits(Fr::from_mont(Fr::neg(ninv)), reinterpret_cast<int8_t*>(&h[(n / 2) * 16]));
    }
    G1NttPlan* p = new G1NttPlan;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_digits), h.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_digits, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);      // h leaves scope
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (p->d_digits) (void)hipFree(p->d_digits);
        delete p;
        set_error("g1 ntt: twiddle digits of n = %llu: %s", (unsigned long long)n, hipGetErrorString(e));
        return UZK_ERR_DEVICE;
    }
    c.g1ntt_plans[n] = p;
    *out = p;
    return UZK_OK;
}

void g1ntt_free(Ctx& c) {
    for (auto& kv : c.g1ntt_plans) {
        G1NttPlan* p = static_cast<G1NttPlan*>(kv.second);
        if (p->d_digits) (void)hipFree(p->d_digits);
        delete p;
    }
    c.g1ntt_plans.clear();
    c.g1ntt_work.release();
    c.g1ntt_prefix.release();
    c.g1ntt_io.release();
}

// group operations of one transform as the kernels run them (doublings, additions): tools/g1_ntt_shape.py
void g1ntt_op_count(uint64_t n, bool inverse, uint64_t* dbl_out, uint64_t* add_out) {
    uint32_t logn = 0;
    while ((1ull << logn) < n) ++logn;
    uint64_t muls = 0;
    for (uint32_t s = 0; s < logn; ++s) muls += n / 2 - (n >> (s + 1));      // t != 0
    if (inverse && n > 1) muls += n;
    *dbl_out = muls * (252 + 4);
    *add_out = muls * (64 + 3) + (uint64_t)logn * n;
}

// d_in -> d_out (may alias), natural order both; n = 2^k checked by the caller
int g1ntt_run(Ctx& c, const Affine* d_in, Affine* d_out, uint64_t n, bool inverse) {
    if (n == 1) {
        if (d_in != d_out) UZK_HIP(hipMemcpyAsync(d_out, d_in, sizeof(Affine), hipMemcpyDeviceToDevice, c.stream));
        return UZK_OK;
    }
    uint32_t logn = 0;
    while ((1ull << logn) < n) ++logn;
    G1NttPlan* plan = nullptr;
    UZK_TRY(g1ntt_plan(c, n, &plan));
    UZK_TRY(c.g1ntt_work.reserve(n * sizeof(P29)));
    UZK_TRY(c.g1ntt_prefix.reserve(n * sizeof(Fp)));
    P29* work = c.g1ntt_work.as<P29>();
    const uint32_t n32 = (uint32_t)n;
    {
        KernelScope ks(c, "g1ntt_load");
        hipLaunchKernelGGL(g1ntt_load_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, d_in, work, n32, logn);
    }
    UZK_HIP(hipGetLastError());
    const unsigned stage_blocks = (unsigned)((n / 2 * 4 + kG1Block - 1) / kG1Block);
    for (uint32_t s = 0; s < logn; ++s) {
        char name[32];
        snprintf(name, sizeof name, "g1ntt_stage_%02u", s);
        KernelScope ks(c, name);
        hipLaunchKernelGGL(g1ntt_stage_kernel, dim3(stage_blocks), dim3(kG1Block), 0, c.stream, work, plan->d_digits, n32, logn, s, inverse ? 1 : 0);
        UZK_HIP(hipGetLastError());
    }
    if (inverse) {
        KernelScope ks(c, "g1ntt_scale");
        hipLaunchKernelGGL(g1ntt_scale_kernel, dim3((unsigned)((n * 4 + kG1Block - 1) / kG1Block)), dim3(kG1Block), 0, c.stream, work,
                           plan->d_digits + (size_t)(n / 2) * 16, n32, plan->scale_negate ? 1 : 0);
        UZK_HIP(hipGetLastError());
    }
    {
        KernelScope ks(c, "g1ntt_affine");
        const uint64_t threads = (n + kAffineRun - 1) / kAffineRun;
        hipLaunchKernelGGL(g1ntt_affine_kernel, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, c.stream, work, c.g1ntt_prefix.as<Fp>(), d_out, n32);
    }
    UZK_HIP(hipGetLastError());
    return UZK_OK;
}

}  // namespace uzk
