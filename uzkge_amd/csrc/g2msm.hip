// Multi-scalar multiplication over BN254 G2 (the b_g2_query term of a Groth16 proof's B): kernels, pipeline, base registry and the
// known-answer kernels of uzk_test_g2_kat and uzk_test_g2_raw_kat.  Design: DESIGN.md, "G2 MSM".
//
// One pass (n <= 2^15 points, `batch` scalar vectors over the same bases, vectors and windows on grid axes):
//   g2_digits      scalar (Montgomery) -> canonical -> + 0x80..80: byte w of the sum, minus 128, is the signed digit of window w
//                  (c = 8, 32 windows, digits in [-128, 127], no carry chain: sum (byte_w - 128) 256^w = s)
//   g2_sort        one workgroup per (vector, window): counting sort of the point indices by |digit| in LDS, the runs of the 128
//                  buckets cut into tasks of at most 32 points (a fat bucket -- boolean scalars -- becomes many tasks)
//   g2_accumulate  one lane per task: mixed additions over its slice of a run (g2_29.hpp), partial sum to HBM
//   g2_segments    one lane per (vector, window, 8 buckets): bucket sums from their tasks' partials, running sums, times the
//                  segment's base index by double-and-add
//   g2_windows     one lane per (vector, window): the 16 segment sums
// and on the host the Horner combination of the 32 window sums per vector (host_g2.hpp).  Longer inputs run as point chunks of
// 2^15 whose window sums are added on the host before the one Horner chain.
//
// uzk_msm_g2_batch_finish ends on the device instead (the same pass, then):
//   g2_chunk_sum   n > 2^15 only, one lane per window: a vector's window sums += those of the chunk just run
//   g2_horner      one lane per vector: total = sum_w 256^w S_w from the top window down, 31 x 8 doublings and 32 general additions
//                  (a window sum can equal or negate the running total: the addition falls through to the doubling, or to infinity)
//   g2_affine      one lane per vector: (X / ZZ, Y / ZZZ) by one inversion in Fq2, conj / norm over one Fq inversion chain
#include <algorithm>
#include <cstring>

#include "ctx.hpp"
#include "lane_tools.hpp"
#include "g2_29.hpp"
#include "handles.hpp"
#include "host_g2.hpp"

namespace uzk {

namespace {
constexpr uint32_t kW = 32;            // windows of 8 bits
constexpr uint32_t kBuckets = 128;     // |digit| in 1 .. 128
constexpr uint32_t kTaskLen = 32;      // points per task at most
constexpr uint32_t kSegs = 16;         // segments of a window's bucket reduction
[[maybe_unused]] constexpr uint32_t kSegLen = kBuckets / kSegs;
constexpr uint32_t kChunkLog = 15;     // points of one pass (a sorted entry is 15 index bits + the sign)
constexpr uint32_t kGroup = 128;       // scalar vectors of one launch sequence (bounds the workspace)

constexpr uint32_t task_cap(uint32_t n) { return kBuckets + n / kTaskLen + 1; }

struct G2Work {
    DevBuf digits, sorted, tstart, tasks, tpart, segs, wsum;
    DevBuf csum, total, aff;           // the device finish: a group's chunk-summed window sums, its Horner totals, its affine results
};

struct G2Entry {
    G2Affine* d_points = nullptr;
    size_t n = 0;
    int device = 0;
};
HandleTable<G2Entry> g_reg(1ull << 59);

// frees the set's device memory; the calling thread's current device is left as it was
void g2_entry_free(const G2Entry& e) {
    if (!e.d_points) return;
    DeviceGuard on(e.device);
    (void)hipFree(e.d_points);
}
}  // namespace

// ---- kernels ----------------------------------------------------------------------------------------------------------------

// digits[(b * 32 + w) * n + i] = byte w of (s_i + 0x8080..80), s_i the canonical scalar i of vector b
__global__ __launch_bounds__(256) void g2_digits_kernel(const Fp* __restrict__ scalars, uint8_t* __restrict__ digits, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    const Fp s = Fr::from_mont(scalars[(uint64_t)b * n + i]);
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c += (uint64_t)s.v[k] + 0x80808080u;            // s < 2^254: the sum stays below 2^256
        const uint32_t t = (uint32_t)c;
        c >>= 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) digits[((uint64_t)b * kW + 4 * k + j) * n + i] = (uint8_t)(t >> (8 * j));
    }
}

// One workgroup per (window, vector).  sorted[slot * n ..]: point index | sign << 15, grouped by |digit| (0 first: never read);
// tstart[slot * 130 + k]: first task of bucket k (k = 1 .. 128), [129] the task count; tasks[slot * cap + t] = start | len << 16.
__global__ __launch_bounds__(256) void g2_sort_kernel(const uint8_t* __restrict__ digits, uint16_t* __restrict__ sorted, uint32_t* __restrict__ tstart,
                                                      uint32_t* __restrict__ tasks, uint32_t n, uint32_t cap) {
    __shared__ uint32_t cnt[kBuckets + 1], start[kBuckets + 2], cur[kBuckets + 1], ts[kBuckets + 2];
    const uint32_t slot = blockIdx.y * kW + blockIdx.x, tid = threadIdx.x;
    const uint8_t* dg = digits + (uint64_t)slot * n;
    if (tid <= kBuckets) cnt[tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 256) {
        const int d = (int)dg[i] - 128;
        atomicAdd(&cnt[d < 0 ? -d : d], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0, t = 0;
        for (uint32_t k = 0; k <= kBuckets; ++k) {
            start[k] = s; cur[k] = s; s += cnt[k];
            ts[k] = t;
            if (k > 0) t += (cnt[k] + kTaskLen - 1) / kTaskLen;
        }
        start[kBuckets + 1] = s;
        ts[kBuckets + 1] = t;
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 256) {
        const int d = (int)dg[i] - 128;
        const uint32_t k = d < 0 ? -d : d;
        const uint32_t pos = atomicAdd(&cur[k], 1u);
        sorted[(uint64_t)slot * n + pos] = (uint16_t)(i | (d < 0 ? 0x8000u : 0u));
    }
    if (tid <= kBuckets + 1) tstart[(uint64_t)slot * (kBuckets + 2) + tid] = ts[tid];
    if (tid >= 1 && tid <= kBuckets) {
        const uint32_t L = cnt[tid], m = (L + kTaskLen - 1) / kTaskLen;       // m tasks of L / m points, the remainder spread
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t lo = L * j / m, hi = L * (j + 1) / m;
            tasks[(uint64_t)slot * cap + ts[tid] + j] = (start[tid] + lo) | ((hi - lo) << 16);
        }
    }
}

// One lane per task: the sum of its points (negated where the digit is), as wire XYZZ.
__global__ __launch_bounds__(64) void g2_accumulate_kernel(const G2Affine* __restrict__ points, const uint16_t* __restrict__ sorted,
                                                           const uint32_t* __restrict__ tstart, const uint32_t* __restrict__ tasks,
                                                           G2XYZZ* __restrict__ tpart, uint32_t n, uint32_t cap) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t slot = blockIdx.z * kW + blockIdx.y, t = blockIdx.x * 64 + threadIdx.x;
    if (t >= tstart[(uint64_t)slot * (kBuckets + 2) + kBuckets + 1]) return;
    const uint32_t task = tasks[(uint64_t)slot * cap + t];
    const uint16_t* run = sorted + (uint64_t)slot * n + (task & 0xffffu);
    const uint32_t len = task >> 16;
    G2Acc acc = g2acc_inf();
    for (uint32_t j = 0; j < len; ++j) {
        const uint32_t e = run[j];
        g2acc_madd(acc, points[e & 0x7fffu], (e >> 15) != 0);
    }
    tpart[(uint64_t)slot * cap + t] = g2acc_store(acc);
#endif
}

// One lane per (vector, window, segment of 8 buckets lo .. lo + 7): sum_k k B_k = sum_k (k - lo + 1) B_k + (lo - 1) sum_k B_k,
// the first by running sums, the second by double-and-add (lo - 1 = 8 seg).
__global__ __launch_bounds__(64) void g2_segments_kernel(const uint32_t* __restrict__ tstart, const G2XYZZ* __restrict__ tpart, G2XYZZ* __restrict__ segs,
                                                         uint32_t slots, uint32_t cap) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t gt = blockIdx.x * 64 + threadIdx.x;
    if (gt >= slots * kSegs) return;
    const uint32_t slot = gt / kSegs, seg = gt % kSegs;
    const uint32_t* ts = tstart + (uint64_t)slot * (kBuckets + 2);
    const G2XYZZ* tp = tpart + (uint64_t)slot * cap;
    G2P run = g2p_inf(), acc = g2p_inf();
    for (uint32_t k = seg * kSegLen + kSegLen; k > seg * kSegLen; --k) {
        for (uint32_t t = ts[k]; t < ts[k + 1]; ++t) g2p_add(run, g2p_load(tp[t]));
        g2p_add(acc, run);
    }
    if (seg != 0 && !run.inf) {
        for (int d = 0; d < 3; ++d) g2p_dbl(run);                    // 8 run
        G2P m = g2p_inf();
        for (int bit = 3; bit >= 0; --bit) {
            g2p_dbl(m);
            if ((seg >> bit) & 1) g2p_add(m, run);
        }
        g2p_add(acc, m);
    }
    segs[gt] = g2p_store(acc);
#endif
}

__global__ __launch_bounds__(64) void g2_windows_kernel(const G2XYZZ* __restrict__ segs, G2XYZZ* __restrict__ wsum, uint32_t slots) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= slots) return;
    G2P acc = g2p_inf();
    for (uint32_t s = 0; s < kSegs; ++s) g2p_add(acc, g2p_load(segs[(uint64_t)slot * kSegs + s]));
    wsum[slot] = g2p_store(acc);
#endif
}

// ---- the finish on the device (uzk_msm_g2_batch_finish) ----------------------------------------------------------------------

// csum[w] (+)= wsum[w] for the 32 windows of one vector: `first` starts the sum.  No barrier.
__global__ __launch_bounds__(64) void g2_chunk_sum_kernel(const G2XYZZ* __restrict__ wsum, G2XYZZ* __restrict__ csum, uint32_t first) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t w = threadIdx.x;
    if (w >= kW) return;
    G2P acc = first ? g2p_inf() : g2p_load(csum[w]);
    g2p_add(acc, g2p_load(wsum[w]));
    csum[w] = g2p_store(acc);
#endif
}

// One lane per vector: total[b] = sum_w 256^w sums[b * 32 + w].  The additions are the general ones: after eight doublings the running
// total can be the next window's sum (doubling) or its negative (infinity), and it is infinite until the first nonzero window.
__global__ __launch_bounds__(64) void g2_horner_kernel(const G2XYZZ* __restrict__ sums, G2XYZZ* __restrict__ total, uint32_t nb) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;                                            // no barrier and no cross-lane move below
    G2P acc = g2p_inf();
#pragma unroll 1
    for (int w = (int)kW - 1; w >= 0; --w) {
        if (w != (int)kW - 1) {
#pragma unroll 1
            for (int d = 0; d < 8; ++d) g2p_dbl(acc);
        }
        g2p_add(acc, g2p_load(sums[(uint64_t)b * kW + w]));
    }
    total[b] = g2p_store(acc);
#endif
}

// Fq2 on the wire words (canonical Montgomery, Fq's own product): the affine map runs once per vector, behind a chain of 280 group
// operations, so it takes the plain field
__device__ inline Fq2w g2w_mul(const Fq2w& a, const Fq2w& b) {
    Fq2w r;
    r.c0 = Fq::sub(Fq::mul(a.c0, b.c0), Fq::mul(a.c1, b.c1));
    r.c1 = Fq::add(Fq::mul(a.c0, b.c1), Fq::mul(a.c1, b.c0));
    return r;
}
// 1 / (a + b u) = (a - b u) / (a^2 + b^2); a + b u != 0 (-1 is no square in Fq: the norm of a nonzero element is nonzero)
__device__ inline Fq2w g2w_inv(const Fq2w& a) {
    const Fp ni = fq_inv_lane(Fq::add(Fq::sqr(a.c0), Fq::sqr(a.c1)));
    Fq2w r;
    r.c0 = Fq::mul(a.c0, ni);
    r.c1 = Fq::neg(Fq::mul(a.c1, ni));
    return r;
}

// One lane per point: wire XYZZ -> canonical affine (X / ZZ, Y / ZZZ) by one inversion of ZZ ZZZ; infinity (zz = 0) -> all zeros
__global__ __launch_bounds__(64) void g2_affine_kernel(const G2XYZZ* __restrict__ in, G2Affine* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const G2XYZZ p = in[i];
    G2Affine r;
    r.x.c0 = Fq::zero(); r.x.c1 = r.x.c0; r.y = r.x;
    if (!(Fq::is_zero(p.zz.c0) && Fq::is_zero(p.zz.c1))) {
        const Fq2w inv = g2w_inv(g2w_mul(p.zz, p.zzz));
        r.x = g2w_mul(p.x, g2w_mul(inv, p.zzz));
        r.y = g2w_mul(p.y, g2w_mul(inv, p.zz));
    }
    out[i] = r;
}

// The primitives element-wise (uzk_test_g2_kat).  Fq2 ops: a, b, out are Fq2w; group ops: a, b affine, out XYZZ.
__global__ __launch_bounds__(64) void g2_kat_kernel(int op, const void* __restrict__ av, const void* __restrict__ bv, void* __restrict__ outv, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (op < 10) {
        using namespace q2;
        const Fq2w a = static_cast<const Fq2w*>(av)[i], b = static_cast<const Fq2w*>(bv)[i];
        Fq2w r = fq2w_zero();
        switch (op) {
            case 0: r = to_wire(mul(ld(a), ld(b))); break;
            case 1: r = to_wire(sqr(ld(a))); break;
            case 2: r = to_wire(add(ld(a), ld(b))); break;
            case 3: r = to_wire(sub(ld(a), ld(b))); break;
            case 4: r = to_wire(neg(ld(a))); break;
            case 5: r = to_wire(mul_kara(ld(a), ld(b))); break;
            default: break;
        }
        static_cast<Fq2w*>(outv)[i] = r;
        return;
    }
    const G2Affine a = static_cast<const G2Affine*>(av)[i], b = static_cast<const G2Affine*>(bv)[i];
    G2XYZZ r;
    if (op == 10 || op == 13) {                       // the accumulator's mixed addition: a + b, a - b
        G2Acc acc = g2acc_inf();
        g2acc_madd(acc, a, false);
        g2acc_madd(acc, b, op == 13);
        r = g2acc_store(acc);
    } else {
        G2P p = g2p_from_affine(a);
        if (op == 11 || op == 14) g2p_add(p, g2p_from_affine(b));
        if (op == 12 || op == 14) g2p_dbl(p);
        r = g2p_store(p);
    }
    static_cast<G2XYZZ*>(outv)[i] = r;
#endif
}

// The group law on RAW limbs (uzk_test_g2_raw_kat): coordinates are taken exactly as given -- nothing is re-limbed or reduced on the way
// in, nothing canonicalised on the way out -- so a test can put every coordinate at the edge of the bound g2_29.hpp carries for it.
struct G2RawPt {
    uint32_t c[4][2][9];               // x, y, zz, zzz; each c0 then c1, nine limbs (op 3 out, op 2 in.b: eight wire words, the ninth 0)
    uint32_t inf;
};
struct G2RawIn {
    G2RawPt a, b;
    uint32_t flag;
};

#if defined(__HIP_DEVICE_COMPILE__)
template <int V>
__device__ __forceinline__ q2::E2<1, V> g2raw_e2(const uint32_t (&c)[2][9]) {
    q2::E2<1, V> r;
#pragma unroll
    for (int i = 0; i < 9; ++i) { r.a.v.l[i] = c[0][i]; r.b.v.l[i] = c[1][i]; }
    return r;
}
template <int V>
__device__ __forceinline__ void g2raw_put(uint32_t (&c)[2][9], const q2::E2<1, V>& x) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { c[0][i] = x.a.v.l[i]; c[1][i] = x.b.v.l[i]; }
}
__device__ __forceinline__ Fq2w g2raw_wire(const uint32_t (&c)[2][9]) {
    Fq2w w;
#pragma unroll
    for (int i = 0; i < 8; ++i) { w.c0.v[i] = c[0][i]; w.c1.v[i] = c[1][i]; }
    return w;
}
__device__ __forceinline__ void g2raw_put_wire(uint32_t (&c)[2][9], const Fq2w& w) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { c[0][i] = w.c0.v[i]; c[1][i] = w.c1.v[i]; }
    c[0][8] = 0; c[1][8] = 0;
}
__device__ __forceinline__ G2P g2raw_point(const G2RawPt& r) {
    G2P p;
    p.x = g2raw_e2<16>(r.c[0]); p.y = g2raw_e2<16>(r.c[1]); p.zz = g2raw_e2<16>(r.c[2]); p.zzz = g2raw_e2<16>(r.c[3]);
    p.inf = r.inf != 0;
    return p;
}
__device__ __forceinline__ G2Acc g2raw_acc(const G2RawPt& r) {
    G2Acc a;
    a.x = g2raw_e2<16>(r.c[0]); a.y = g2raw_e2<16>(r.c[1]); a.zz = g2raw_e2<2>(r.c[2]); a.zzz = g2raw_e2<2>(r.c[3]);
    a.inf = r.inf != 0;
    return a;
}
#endif

// op 0 g2p_add(a, b), 1 g2p_dbl(a), 2 g2acc_madd(a as accumulator, b.x / b.y as wire words, flag = negate), 3 g2p_store(a) (flag 0) or
// g2acc_store(a) (flag 1) as wire words, 4 q2::is_zero of a's x as E2<1, 32> (the answer in out.inf)
__global__ __launch_bounds__(64) void g2_raw_kat_kernel(int op, const G2RawIn* __restrict__ in, G2RawPt* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const G2RawIn rec = in[i];
    G2RawPt r;
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 2; ++j)
            for (int l = 0; l < 9; ++l) r.c[k][j][l] = 0;
    r.inf = 0;
    if (op == 0 || op == 1) {
        G2P p = g2raw_point(rec.a);
        if (op == 0) g2p_add(p, g2raw_point(rec.b));
        else g2p_dbl(p);
        g2raw_put(r.c[0], p.x); g2raw_put(r.c[1], p.y); g2raw_put(r.c[2], p.zz); g2raw_put(r.c[3], p.zzz);
        r.inf = p.inf;
    } else if (op == 2) {
        G2Acc a = g2raw_acc(rec.a);
        G2Affine q;
        q.x = g2raw_wire(rec.b.c[0]); q.y = g2raw_wire(rec.b.c[1]);
        g2acc_madd(a, q, rec.flag != 0);
        g2raw_put(r.c[0], a.x); g2raw_put(r.c[1], a.y); g2raw_put(r.c[2], a.zz); g2raw_put(r.c[3], a.zzz);
        r.inf = a.inf;
    } else if (op == 3) {
        const G2XYZZ w = rec.flag != 0 ? g2acc_store(g2raw_acc(rec.a)) : g2p_store(g2raw_point(rec.a));
        g2raw_put_wire(r.c[0], w.x); g2raw_put_wire(r.c[1], w.y); g2raw_put_wire(r.c[2], w.zz); g2raw_put_wire(r.c[3], w.zzz);
        r.inf = rec.a.inf != 0;
    } else {
        r.inf = q2::is_zero(g2raw_e2<32>(rec.a.c[0]));
    }
    out[i] = r;
#endif
}

// ---- host -------------------------------------------------------------------------------------------------------------------

static G2Work& work(Ctx& c) {
    if (!c.g2) c.g2 = new G2Work();
    return *static_cast<G2Work*>(c.g2);
}
void g2_free(Ctx& c) {
    if (!c.g2) return;
    G2Work* w = static_cast<G2Work*>(c.g2);
    w->digits.release(); w->sorted.release(); w->tstart.release(); w->tasks.release(); w->tpart.release(); w->segs.release(); w->wsum.release(); w->csum.release(); w->total.release(); w->aff.release();
    delete w;
    c.g2 = nullptr;
}

int g2_register(Ctx& c, const G2Affine* points, size_t n, uint64_t* handle_out) {
    G2Entry e;
    e.n = n;
    e.device = c.device;
    if (n > 0) {
        UZK_HIP(hipMalloc(reinterpret_cast<void**>(&e.d_points), n * sizeof(G2Affine)));
        hipError_t err = hipMemcpyAsync(e.d_points, points, n * sizeof(G2Affine), hipMemcpyHostToDevice, c.stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c.stream);
        if (err != hipSuccess) { (void)hipFree(e.d_points); UZK_HIP(err); }
    }
    *handle_out = g_reg.insert(e);
    return UZK_OK;
}
int g2_register_owned(G2Affine* d_points, size_t n, int device, uint64_t* handle_out) {
    G2Entry e;
    e.d_points = d_points;
    e.n = n;
    e.device = device;
    *handle_out = g_reg.insert(e);
    return UZK_OK;
}
bool g2_lookup(uint64_t handle, const G2Affine** d_points, size_t* n, int* device) {
    G2Entry e;
    if (!g_reg.get(handle, &e)) return false;
    if (d_points) *d_points = e.d_points;
    if (n) *n = e.n;
    if (device) *device = e.device;
    return true;
}
bool g2_release(uint64_t handle) {
    G2Entry e;
    if (!g_reg.take(handle, &e)) return false;
    g2_entry_free(e);
    return true;
}
void g2_release_all() { g_reg.drain(g2_entry_free); }

// window sums of `batch` vectors over n <= 2^15 points, left in the workspace: wsum[b * 32 + w], wire XYZZ; nothing is waited for
static int g2_pass_launch(Ctx& c, const G2Affine* d_points, const Fp* d_scalars, uint32_t n, uint32_t batch) {
    G2Work& w = work(c);
    const uint32_t slots = batch * kW, cap = task_cap(n);
    UZK_TRY(w.digits.reserve((size_t)slots * n));
    UZK_TRY(w.sorted.reserve((size_t)slots * n * sizeof(uint16_t)));
    UZK_TRY(w.tstart.reserve((size_t)slots * (kBuckets + 2) * sizeof(uint32_t)));
    UZK_TRY(w.tasks.reserve((size_t)slots * cap * sizeof(uint32_t)));
    UZK_TRY(w.tpart.reserve((size_t)slots * cap * sizeof(G2XYZZ)));
    UZK_TRY(w.segs.reserve((size_t)slots * kSegs * sizeof(G2XYZZ)));
    UZK_TRY(w.wsum.reserve((size_t)slots * sizeof(G2XYZZ)));
    c.cur_stream = c.stream;
    UZK_LAUNCH(c, "g2_digits", g2_digits_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, c.stream, d_scalars, w.digits.as<uint8_t>(), n);
    UZK_LAUNCH(c, "g2_sort", g2_sort_kernel, dim3(kW, batch), dim3(256), 0, c.stream, w.digits.as<uint8_t>(), w.sorted.as<uint16_t>(), w.tstart.as<uint32_t>(),
               w.tasks.as<uint32_t>(), n, cap);
    UZK_LAUNCH(c, "g2_accumulate", g2_accumulate_kernel, dim3((cap + 63) / 64, kW, batch), dim3(64), 0, c.stream, d_points, w.sorted.as<uint16_t>(),
               w.tstart.as<uint32_t>(), w.tasks.as<uint32_t>(), w.tpart.as<G2XYZZ>(), n, cap);
    UZK_LAUNCH(c, "g2_segments", g2_segments_kernel, dim3((slots * kSegs + 63) / 64), dim3(64), 0, c.stream, w.tstart.as<uint32_t>(), w.tpart.as<G2XYZZ>(),
               w.segs.as<G2XYZZ>(), slots, cap);
    UZK_LAUNCH(c, "g2_windows", g2_windows_kernel, dim3((slots + 63) / 64), dim3(64), 0, c.stream, w.segs.as<G2XYZZ>(), w.wsum.as<G2XYZZ>(), slots);
    return UZK_OK;
}

// the same, copied to the host: out[b * 32 + w]
static int g2_pass(Ctx& c, const G2Affine* d_points, const Fp* d_scalars, uint32_t n, uint32_t batch, G2XYZZ* out) {
    UZK_TRY(g2_pass_launch(c, d_points, d_scalars, n, batch));
    UZK_HIP(hipMemcpyAsync(out, work(c).wsum.p, (size_t)batch * kW * sizeof(G2XYZZ), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// out[b] = sum_i scalars[b * n + i] * points[i]; d_scalars on the device (Montgomery form), out on the host
int g2_msm_run(Ctx& c, const G2Affine* d_points, const Fp* d_scalars, size_t n, uint32_t batch, G2Jac* out) {
    for (uint32_t b = 0; b < batch; ++b) out[b] = h64::j2_to(h64::j2_inf());
    if (n == 0 || batch == 0) return UZK_OK;
    const size_t chunk = (size_t)1 << kChunkLog;
    std::vector<G2XYZZ> ws((size_t)std::min(batch, kGroup) * kW);
    std::vector<h64::J2> sums;
    for (uint32_t b0 = 0; b0 < batch; b0 += kGroup) {
        const uint32_t nb = std::min(kGroup, batch - b0);
        sums.assign((size_t)nb * kW, h64::j2_inf());
        if (n <= chunk) {
            UZK_TRY(g2_pass(c, d_points, d_scalars + (size_t)b0 * n, (uint32_t)n, nb, ws.data()));
            HostScope hs(c, "host_g2_horner");
            for (size_t k = 0; k < sums.size(); ++k) sums[k] = h64::j2_from_xyzz(ws[k]);
        } else {
            // point chunks: a vector's scalars are n apart, so each vector runs its chunks on its own
            for (uint32_t b = 0; b < nb; ++b)
                for (size_t lo = 0; lo < n; lo += chunk) {
                    const size_t len = std::min(chunk, n - lo);
                    UZK_TRY(g2_pass(c, d_points + lo, d_scalars + (size_t)(b0 + b) * n + lo, (uint32_t)len, 1, ws.data()));
                    HostScope hs(c, "host_g2_horner");
                    for (uint32_t w = 0; w < kW; ++w) sums[(size_t)b * kW + w] = h64::j2_add(sums[(size_t)b * kW + w], h64::j2_from_xyzz(ws[w]));
                }
        }
        HostScope hs(c, "host_g2_horner");
        for (uint32_t b = 0; b < nb; ++b) {
            h64::J2 total = h64::j2_inf();
            for (int w = (int)kW - 1; w >= 0; --w) {
                if (w != (int)kW - 1) for (int d = 0; d < 8; ++d) total = h64::j2_dbl(total);
                total = h64::j2_add(total, sums[(size_t)b * kW + w]);
            }
            out[b0 + b] = h64::j2_to(total);
        }
    }
    return UZK_OK;
}

// The same sums as canonical affine points (infinity all zeros), finished on the device: to `out` (host), to `d_out` (device), or to
// both; at least one of them.  The window sums never leave the device.  With d_out alone nothing is waited for.
int g2_msm_finish_run(Ctx& c, const G2Affine* d_points, const Fp* d_scalars, size_t n, uint32_t batch, G2Affine* out, G2Affine* d_out) {
    if (batch == 0) return UZK_OK;
    if (n == 0) {
        if (out) std::memset(out, 0, (size_t)batch * sizeof(G2Affine));
        if (d_out) UZK_HIP(hipMemsetAsync(d_out, 0, (size_t)batch * sizeof(G2Affine), c.stream));
        return UZK_OK;
    }
    G2Work& w = work(c);
    const size_t chunk = (size_t)1 << kChunkLog;
    for (uint32_t b0 = 0; b0 < batch; b0 += kGroup) {
        const uint32_t nb = std::min(kGroup, batch - b0);
        UZK_TRY(w.total.reserve((size_t)nb * sizeof(G2XYZZ)));
        const G2XYZZ* sums = nullptr;
        if (n <= chunk) {
            UZK_TRY(g2_pass_launch(c, d_points, d_scalars + (size_t)b0 * n, (uint32_t)n, nb));
            sums = w.wsum.as<G2XYZZ>();
        } else {
            // point chunks, each vector on its own (as g2_msm_run): its window sums gather in csum
            UZK_TRY(w.csum.reserve((size_t)nb * kW * sizeof(G2XYZZ)));
            for (uint32_t b = 0; b < nb; ++b)
                for (size_t lo = 0; lo < n; lo += chunk) {
                    const size_t len = std::min(chunk, n - lo);
                    UZK_TRY(g2_pass_launch(c, d_points + lo, d_scalars + (size_t)(b0 + b) * n + lo, (uint32_t)len, 1));
                    UZK_LAUNCH(c, "g2_chunk_sum", g2_chunk_sum_kernel, dim3(1), dim3(64), 0, c.stream, w.wsum.as<G2XYZZ>(), w.csum.as<G2XYZZ>() + (size_t)b * kW,
                               lo == 0 ? 1u : 0u);
                }
            sums = w.csum.as<G2XYZZ>();
        }
        G2Affine* dst = d_out ? d_out + b0 : nullptr;
        if (!dst) {
            UZK_TRY(w.aff.reserve((size_t)nb * sizeof(G2Affine)));
            dst = w.aff.as<G2Affine>();
        }
        UZK_LAUNCH(c, "g2_horner", g2_horner_kernel, dim3((nb + 63) / 64), dim3(64), 0, c.stream, sums, w.total.as<G2XYZZ>(), nb);
        UZK_LAUNCH(c, "g2_affine", g2_affine_kernel, dim3((nb + 63) / 64), dim3(64), 0, c.stream, w.total.as<G2XYZZ>(), dst, nb);
        if (out) UZK_HIP(hipMemcpyAsync(out + b0, dst, (size_t)nb * sizeof(G2Affine), hipMemcpyDeviceToHost, c.stream));
    }
    if (out) UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

void g2_fold_host(const G2Jac* partials, size_t count, G2Jac* out) {
    h64::J2 acc = h64::j2_inf();
    for (size_t i = 0; i < count; ++i) acc = h64::j2_add(acc, h64::j2_from(partials[i]));
    *out = h64::j2_to(acc);
}
void g2_to_affine_host(const G2Jac* p, G2Affine* out) { *out = h64::j2_to_affine(h64::j2_from(*p)); }

// op 0..5: a, b, out are n Fq2 elements (8 words); op 10..14: a, b n affine points (16 words), out n Jacobian points (24 words)
int g2_op_device(Ctx& c, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    if (n == 0) return UZK_OK;
    const bool group = op >= 10;
    const size_t in_bytes = n * (group ? sizeof(G2Affine) : sizeof(Fq2w)), out_bytes = n * (group ? sizeof(G2XYZZ) : sizeof(Fq2w));
    void *da = nullptr, *db = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&da, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&db, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, out_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(da, a, in_bytes, hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, in_bytes, hipMemcpyHostToDevice, c.stream);
    std::vector<G2XYZZ> xy(group ? n : 0);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(g2_kat_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream, op, da, db, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(group ? static_cast<void*>(xy.data()) : static_cast<void*>(out), dout, out_bytes, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (da) (void)hipFree(da);
    if (db) (void)hipFree(db);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    if (group) {
        G2Jac* jo = reinterpret_cast<G2Jac*>(out);
        for (size_t i = 0; i < n; ++i) jo[i] = h64::j2_to(h64::j2_from_xyzz(xy[i]));
    }
    return UZK_OK;
}

// n records of G2RawIn (147 words) -> n records of G2RawPt (73 words), both on the host
int g2_raw_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (n == 0) return UZK_OK;
    static_assert(sizeof(G2RawIn) == 147 * sizeof(uint32_t) && sizeof(G2RawPt) == 73 * sizeof(uint32_t), "records are packed words");
    G2RawIn* din = nullptr;
    G2RawPt* dout = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&din), n * sizeof(G2RawIn));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), n * sizeof(G2RawPt));
    if (e == hipSuccess) e = hipMemcpyAsync(din, in, n * sizeof(G2RawIn), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(g2_raw_kat_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream, op, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(G2RawPt), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

}  // namespace uzk
