// Validation of an SRS on the device: are the bases curve points, and are they the powers of one tau?
//
//   srs_curve_kernel    one point per lane, grid-stride: both coordinates below p, y^2 = x^3 + 3 on the 8 x 32-bit Montgomery words
//                       (three products against 64 bytes read -- the lazy 29-bit limbs would not pay here).  A wave ballots its three
//                       classes and its first bad lane, a workgroup folds its waves in the LDS and writes ONE record; the host folds
//                       the records after one copy.  No atomics.
//   srs_weights_kernel  one lane per Keccak block: digest j = Keccak-256(seed || "uzksrsv1" || le64(j)) is the two 128-bit weights
//                       rho_2j, rho_2j+1, written as Montgomery Fr.  The same code runs on the host (uzk_srs_fold_weights).
//
// The fold itself is two MSMs over the same weights (api.cpp): L = sum rho_i P_i, R = sum rho_i P_i+1; the run is a power sequence
// of tau iff e(R, H) = e(L, [tau] H), up to a 2^-128 chance over the seed.
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "keccak.hpp"
#include "lane_tools.hpp"

namespace uzk {

constexpr uint32_t kSrsBlock = 256;
constexpr uint32_t kSrsWaves = kSrsBlock / 64;
constexpr uint64_t kSrsNone = ~0ull;

// what one workgroup found; first_bad relative to the array the kernel was given
struct SrsCurveRecord { uint64_t first_bad, infinity, non_canonical, off_curve; };

enum { SRS_GOOD = 0, SRS_INF = 1, SRS_NON_CANONICAL = 2, SRS_OFF_CURVE = 3 };
UZK_HD int srs_classify(const Affine& p) {
    if (affine_is_inf(p)) return SRS_INF;
    if (!below_modulus<FqCfg>(p.x) || !below_modulus<FqCfg>(p.y)) return SRS_NON_CANONICAL;
    const Fp one = Fq::one();
    const Fp three = Fq::add_portable(Fq::add_portable(one, one), one);   // g1_b() in plain C++: folded at compile time, which this
    const Fp rhs = g1_rhs(p.x, three);                                     // kernel's 64 registers (occupancy 8) depend on
    return Fq::eq(Fq::sqr(p.y), rhs) ? SRS_GOOD : SRS_OFF_CURVE;
}

// Every thread runs every round and reaches the barrier: a lane past the end classifies nothing and votes "good".
__global__ __launch_bounds__(kSrsBlock) void srs_curve_kernel(const Affine* __restrict__ pts, uint64_t count, SrsCurveRecord* __restrict__ records) {
    __shared__ SrsCurveRecord part[kSrsWaves];
    const uint32_t t = threadIdx.x, wave = t / 64, lane = t % 64;
    const uint64_t stride = (uint64_t)gridDim.x * kSrsBlock;
    const uint64_t rounds = (count + stride - 1) / stride;
    uint64_t first = kSrsNone, n_inf = 0, n_nc = 0, n_off = 0;           // the same in every lane of a wave
#pragma unroll 1
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t wave_base = r * stride + (uint64_t)blockIdx.x * kSrsBlock + wave * 64;
        const uint64_t i = wave_base + lane;
        int cls = SRS_GOOD;
        if (i < count) cls = srs_classify(pts[i]);
        const uint64_t m_inf = __ballot(cls == SRS_INF), m_nc = __ballot(cls == SRS_NON_CANONICAL), m_off = __ballot(cls == SRS_OFF_CURVE);
        n_inf += (uint64_t)__popcll(m_inf);
        n_nc += (uint64_t)__popcll(m_nc);
        n_off += (uint64_t)__popcll(m_off);
        const uint64_t bad = m_nc | m_off;
        // a wave's indices grow from round to round: its first hit is its smallest
        if (bad != 0 && first == kSrsNone) first = wave_base + (uint64_t)(__ffsll((unsigned long long)bad) - 1);
    }
    if (lane == 0) {
        SrsCurveRecord rec;
        rec.first_bad = first; rec.infinity = n_inf; rec.non_canonical = n_nc; rec.off_curve = n_off;
        part[wave] = rec;
    }
    __syncthreads();
    if (t == 0) {
        SrsCurveRecord rec = part[0];
        for (uint32_t w = 1; w < kSrsWaves; ++w) {
            rec.first_bad = part[w].first_bad < rec.first_bad ? part[w].first_bad : rec.first_bad;
            rec.infinity += part[w].infinity; rec.non_canonical += part[w].non_canonical; rec.off_curve += part[w].off_curve;
        }
        records[blockIdx.x] = rec;
    }
}

// ---- weights ------------------------------------------------------------------------------------------------------------------
struct SrsSeed { uint64_t w[4]; };                     // the 32 seed bytes as four little-endian lanes
constexpr uint64_t kSrsDomain = 0x31767372736b7a75ull; // "uzksrsv1" read as a little-endian lane

// Block j: the 48-byte message seed || "uzksrsv1" || le64(j) is six lanes of one rate block; byte 48 is the padding byte 0x01, the
// block's last byte carries the closing bit.  Digest bytes 0..15 and 16..31 are the two weights (little endian, < 2^128).
UZK_HD void srs_weight_pair(const SrsSeed& seed, uint64_t j, Fp& even, Fp& odd) {
    uint64_t s[25];
#pragma unroll
    for (int l = 0; l < 25; ++l) s[l] = 0;
    s[0] = seed.w[0]; s[1] = seed.w[1]; s[2] = seed.w[2]; s[3] = seed.w[3];
    s[4] = kSrsDomain;
    s[5] = j;
    s[6] = 0x01ull;
    s[16] = 0x8000000000000000ull;
    vf_keccak_f(s);
    Fp a = Fr::zero(), b = Fr::zero();
    a.v[0] = (uint32_t)s[0]; a.v[1] = (uint32_t)(s[0] >> 32); a.v[2] = (uint32_t)s[1]; a.v[3] = (uint32_t)(s[1] >> 32);
    b.v[0] = (uint32_t)s[2]; b.v[1] = (uint32_t)(s[2] >> 32); b.v[2] = (uint32_t)s[3]; b.v[3] = (uint32_t)(s[3] >> 32);
    even = Fr::to_mont(a);
    odd = Fr::to_mont(b);
}

// out[k] = rho_(first + k), k < count: lane b of the grid takes block first / 2 + b
__global__ __launch_bounds__(kSrsBlock) void srs_weights_kernel(SrsSeed seed, uint64_t first, uint64_t count, uint64_t blocks, Fp* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * kSrsBlock + threadIdx.x;
    if (b < blocks) {
        const uint64_t j = first / 2 + b;
        Fp even, odd;
        srs_weight_pair(seed, j, even, odd);
        // weight 2 j lies below `first` only for the first block of an odd start; 2 j - first < count then cannot wrap
        const uint64_t at = 2 * j - first;
        if (2 * j >= first && at < count) out[at] = even;
        if (at + 1 < count) out[at + 1] = odd;
    }
}

static SrsSeed srs_seed_of(const uint8_t seed[32]) {
    SrsSeed s;
    std::memcpy(s.w, seed, 32);
    return s;
}
// Keccak blocks that hold weights first .. first + count - 1 (count >= 1, first + count does not wrap)
static uint64_t srs_weight_blocks(uint64_t first, uint64_t count) { return (first + count - 1) / 2 - first / 2 + 1; }

void srs_weights_host(const uint8_t seed[32], uint64_t first, uint64_t count, Fp* out) {
    if (count == 0) return;
    const SrsSeed s = srs_seed_of(seed);
    const uint64_t blocks = srs_weight_blocks(first, count);
    for (uint64_t b = 0; b < blocks; ++b) {
        const uint64_t j = first / 2 + b;
        Fp even, odd;
        srs_weight_pair(s, j, even, odd);
        const uint64_t at = 2 * j - first;                 // wraps to 2^64 - 1 for the even half below an odd start
        if (2 * j >= first && at < count) out[at] = even;
        if (at + 1 < count) out[at + 1] = odd;
    }
}

int srs_weights_run(Ctx& c, const uint8_t seed[32], uint64_t first, uint64_t count, Fp* d_out) {
    if (count == 0) return UZK_OK;
    const uint64_t blocks = srs_weight_blocks(first, count);
    const uint64_t grid = (blocks + kSrsBlock - 1) / kSrsBlock;
    if (grid > 0x7fffffffull) { set_error("srs weights: %llu weights in one launch", (unsigned long long)count); return UZK_ERR_PARAMETER; }
    UZK_LAUNCH(c, "srs_weights", srs_weights_kernel, dim3((unsigned)grid), dim3(kSrsBlock), 0, c.stream, srs_seed_of(seed), first, count, blocks, d_out);
    return UZK_OK;
}

// The report of d_points[0 .. count): first_bad relative to d_points (the caller adds its offset).
int srs_curve_run(Ctx& c, const Affine* d_points, uint64_t count, uzk_srs_curve_report* out) {
    out->checked = count; out->infinity = 0; out->non_canonical = 0; out->off_curve = 0; out->first_bad = kSrsNone;
    if (count == 0) return UZK_OK;
    // eight workgroups of four waves per compute unit fill every SIMD's wave slots; beyond that a lane strides
    const uint64_t want = (count + kSrsBlock - 1) / kSrsBlock, cap = (uint64_t)c.num_cus * 8;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    UZK_TRY(c.srs_records.reserve((size_t)grid * sizeof(SrsCurveRecord)));
    SrsCurveRecord* d_rec = c.srs_records.as<SrsCurveRecord>();
    UZK_LAUNCH(c, "srs_curve", srs_curve_kernel, dim3(grid), dim3(kSrsBlock), 0, c.stream, d_points, count, d_rec);
    std::vector<SrsCurveRecord> rec(grid);
    UZK_HIP(hipMemcpyAsync(rec.data(), d_rec, (size_t)grid * sizeof(SrsCurveRecord), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    for (const SrsCurveRecord& r : rec) {
        out->infinity += r.infinity; out->non_canonical += r.non_canonical; out->off_curve += r.off_curve;
        if (r.first_bad < out->first_bad) out->first_bad = r.first_bad;
    }
    return UZK_OK;
}

void srscheck_free(Ctx& c) {
    c.srs_records.release();
    c.srs_weights.release();
    c.srs_points.release();
}

}  // namespace uzk
