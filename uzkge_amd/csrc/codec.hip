// The point codec: ark-serialize's compressed G1, G2 and Baby Jubjub points (include/uzkge_gpu.h, "the point codec"), one lane per point.
//
//   codec_g1_dec    x little-endian, flags in the top two bits; y = sqrt(x^3 + 3) in one chain of Fq (sqrt29.hpp), the root chosen by the
//                   sign flag against its negation in canonical, non-Montgomery words
//   codec_g2_dec    x.c0, x.c1; y = sqrt(x^3 + 3 / (9 + u)) in Fq2 by the norm method: three chain lengths, two of them side by side
//   codec_g2_sub    [r] Q = O for the decoded points with status 0: the double-and-add over G2P (g2_in_subgroup of lane_tools.hpp)
//   codec_ed_dec    y; x = sqrt((1 - y^2) / (1 - d y^2)) in Fr with the division inside the root (fr_sqrt_ratio)
//   codec_ed_sub    ed::classify on the decoded points with status 0
//   codec_*_enc     the cheap direction: leave Montgomery form, compare the coordinate with its negation, write the bytes
//   codec_sqrt_kat  the three roots alone (include/uzkge_gpu_test.h uzk_test_sqrt_kat)
// Every lane of a decoding batch walks the same constant exponent; lanes that stop early (an infinity, a word that is not canonical)
// only sit out.  A point whose status is not 0 is written as zeros.  tests/codec_ref.py is the restatement on Python integers.
#include "ctx.hpp"
#include "ed29.hpp"
#include "g2_29.hpp"
#include "handles.hpp"
#include "lane_tools.hpp"
#include "sqrt29.hpp"

namespace uzk {

constexpr uint32_t kCdBlock = 64;
enum { CD_OK = 0, CD_NOT_CANONICAL = 1, CD_NO_POINT = 2, CD_NOT_IN_SUBGROUP = 3 };
enum { CD_G1 = 0, CD_G2 = 1, CD_ED = 2 };
static_assert(sizeof(Affine) == 64 && sizeof(G2Affine) == 128 && sizeof(EdAffine) == 64, "wire points");

// 32 little-endian bytes as an integer (encodings are 4-byte aligned: 32 or 64 bytes apart in a 256-byte aligned array)
__device__ __forceinline__ Fp cd_load(const uint8_t* p) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p);
    Fp v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.v[j] = src[j];
    return v;
}
__device__ __forceinline__ void cd_store(uint8_t* p, const Fp& v, uint32_t flags) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 7; ++j) dst[j] = v.v[j];
    dst[7] = v.v[7] | flags;
}
// c > M - c for a canonical c (0 is not larger than its negation, which is 0)
template <class C>
__device__ __forceinline__ bool cd_larger(const Fp& c) {
    if (Field<C>::is_zero(c)) return false;
    const Fp n = u256_sub(Field<C>::modulus(), c);
    return !u256_geq(n, c);
}

__global__ __launch_bounds__(kCdBlock) void codec_g1_dec_kernel(const uint8_t* __restrict__ in, Affine* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;                                            // no barrier and no cross-lane move below
    using Z = LzOps<Fq29>;
    Fp x = cd_load(in + (size_t)i * 32);
    const uint32_t flags = x.v[7] >> 30;                           // bit 0: infinity, bit 1: the larger y
    x.v[7] &= 0x3fffffffu;
    Affine p;
    p.x = Fq::zero(); p.y = p.x;
    uint32_t st = CD_OK;
    if (flags & 1) {
        if ((flags & 2) || !Fq::is_zero(x)) st = CD_NOT_CANONICAL;
    } else if (!below_modulus<FqCfg>(x)) {
        st = CD_NOT_CANONICAL;
    } else {
        const Fp xm = Fq::to_mont(x);
        const sq::Cq X = sq::red(Z::ld(xm));
        const Fp one = Fq::one();
        const sq::Cq rhs = sq::red(Z::add(Z::mul(Z::sqr(X), X), Z::ld(Fq::add(Fq::add(one, one), one))));
        sq::Cq Y;
        if (!sq::fq_sqrt(rhs, &Y)) st = CD_NO_POINT;
        else {
            Fp ym = Z::to_wire(Y);
            const Fp yc = Fq::from_mont(ym);
            if (Fq::is_zero(yc) && (flags & 2)) st = CD_NOT_CANONICAL;
            else {
                if (cd_larger<FqCfg>(yc) != ((flags & 2) != 0)) ym = Fq::neg(ym);
                p.x = xm; p.y = ym;
            }
        }
    }
    out[i] = p;
    status[i] = (uint8_t)st;
#endif
}

__global__ __launch_bounds__(kCdBlock) void codec_g2_dec_kernel(const uint8_t* __restrict__ in, G2Affine* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    Fp x0 = cd_load(in + (size_t)i * 64), x1 = cd_load(in + (size_t)i * 64 + 32);
    const uint32_t flags = x1.v[7] >> 30;
    x1.v[7] &= 0x3fffffffu;
    G2Affine p;
    p.x = fq2w_zero(); p.y = p.x;
    uint32_t st = CD_OK;
    if (flags & 1) {
        if ((flags & 2) || !Fq::is_zero(x0) || !Fq::is_zero(x1)) st = CD_NOT_CANONICAL;
    } else if (!below_modulus<FqCfg>(x0) || !below_modulus<FqCfg>(x1)) {
        st = CD_NOT_CANONICAL;
    } else {
        Fq2w xw;
        xw.c0 = Fq::to_mont(x0); xw.c1 = Fq::to_mont(x1);
        const auto X = q2::ldr(xw);
        const auto rhs = q2::red(q2::add(q2::mul(q2::sqr(X), X), q2::ldr(g2_twist_b())));
        q2::E2<1, 2> Y;
        if (!sq::fq2_sqrt(rhs, &Y)) st = CD_NO_POINT;
        else {
            Fq2w yw = q2::to_wire(Y);
            const Fp c0 = Fq::from_mont(yw.c0), c1 = Fq::from_mont(yw.c1);
            const bool zero = Fq::is_zero(c0) && Fq::is_zero(c1);
            if (zero && (flags & 2)) st = CD_NOT_CANONICAL;
            else {
                const bool larger = Fq::is_zero(c1) ? cd_larger<FqCfg>(c0) : cd_larger<FqCfg>(c1);     // c1 first, then c0
                if (larger != ((flags & 2) != 0)) yw = fq2w_neg(yw);
                p.x = xw; p.y = yw;
            }
        }
    }
    out[i] = p;
    status[i] = (uint8_t)st;
#endif
}

// [r] Q = O over G2P (g2_in_subgroup of lane_tools.hpp): the bits of r are the same for every lane
__global__ __launch_bounds__(kCdBlock) void codec_g2_sub_kernel(G2Affine* __restrict__ pts, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    if (status[i] != CD_OK) return;
    if (!g2_in_subgroup(g2p_from_affine(pts[i]))) {
        G2Affine z;
        z.x = fq2w_zero(); z.y = z.x;
        pts[i] = z;
        status[i] = (uint8_t)CD_NOT_IN_SUBGROUP;
    }
#endif
}

__global__ __launch_bounds__(kCdBlock) void codec_ed_dec_kernel(const uint8_t* __restrict__ in, EdAffine* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    using Z = LzOps<Fr29>;
    Fp y = cd_load(in + (size_t)i * 32);
    const bool sign = (y.v[7] >> 31) != 0;
    y.v[7] &= 0x7fffffffu;                                         // bit 6 of the last byte belongs to y: set, y is not below q
    EdAffine p;
    p.x = Fr::zero(); p.y = p.x;
    uint32_t st = CD_OK;
    if (!ed_coord_canonical(y)) st = CD_NOT_CANONICAL;
    else {
        const Fp ym = Fr::to_mont(y);
        const sq::Cr Y = ed::ld(ym);
        const auto yy = Z::sqr(Y);
        const sq::Cr u = sq::red(Z::sub(Z::one(), yy));
        const sq::Cr v = sq::red(Z::sub(Z::one(), Z::mul(yy, Z::ld(ed_d_wire()))));       // d is not a square: never 0
        sq::Cr X;
        if (!sq::fr_sqrt_ratio(u, v, &X)) st = CD_NO_POINT;
        else {
            Fp xm = Z::to_wire(X);
            const Fp xc = Fr::from_mont(xm);
            if (Fr::is_zero(xc) && sign) st = CD_NOT_CANONICAL;
            else {
                if (cd_larger<FrCfg>(xc) != sign) xm = Fr::neg(xm);
                p.x = xm; p.y = ym;
            }
        }
    }
    out[i] = p;
    status[i] = (uint8_t)st;
#endif
}

__global__ __launch_bounds__(kCdBlock) void codec_ed_sub_kernel(EdAffine* __restrict__ pts, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    if (status[i] != CD_OK) return;
    const uint32_t st = ed::classify(pts[i]);
    if (st != CD_OK) {
        EdAffine z;
        z.x = Fr::zero(); z.y = z.x;
        pts[i] = z;
        status[i] = (uint8_t)st;
    }
#endif
}

// ---- encoding -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCdBlock) void codec_g1_enc_kernel(const Affine* __restrict__ pts, uint8_t* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    const Affine p = pts[i];
    Fp x = Fq::zero();
    uint32_t flags = 0, st = CD_OK;
    if (!below_modulus<FqCfg>(p.x) || !below_modulus<FqCfg>(p.y)) st = CD_NOT_CANONICAL;
    else if (affine_is_inf(p)) flags = 1u << 30;
    else {
        x = Fq::from_mont(p.x);
        flags = cd_larger<FqCfg>(Fq::from_mont(p.y)) ? 1u << 31 : 0;
    }
    cd_store(out + (size_t)i * 32, x, flags);
    status[i] = (uint8_t)st;
#endif
}

__global__ __launch_bounds__(kCdBlock) void codec_g2_enc_kernel(const G2Affine* __restrict__ pts, uint8_t* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    const G2Affine p = pts[i];
    Fp x0 = Fq::zero(), x1 = x0;
    uint32_t flags = 0, st = CD_OK;
    if (!below_modulus<FqCfg>(p.x.c0) || !below_modulus<FqCfg>(p.x.c1) || !below_modulus<FqCfg>(p.y.c0) || !below_modulus<FqCfg>(p.y.c1))
        st = CD_NOT_CANONICAL;
    else if (fq2w_is_zero(p.x) && fq2w_is_zero(p.y)) flags = 1u << 30;
    else {
        x0 = Fq::from_mont(p.x.c0); x1 = Fq::from_mont(p.x.c1);
        const Fp c0 = Fq::from_mont(p.y.c0), c1 = Fq::from_mont(p.y.c1);
        flags = (Fq::is_zero(c1) ? cd_larger<FqCfg>(c0) : cd_larger<FqCfg>(c1)) ? 1u << 31 : 0;
    }
    cd_store(out + (size_t)i * 64, x0, 0);
    cd_store(out + (size_t)i * 64 + 32, x1, flags);
    status[i] = (uint8_t)st;
#endif
}

__global__ __launch_bounds__(kCdBlock) void codec_ed_enc_kernel(const EdAffine* __restrict__ pts, uint8_t* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    const EdAffine p = pts[i];
    Fp y = Fr::zero();
    uint32_t flags = 0, st = CD_OK;
    if (!ed_coord_canonical(p.x) || !ed_coord_canonical(p.y)) st = CD_NOT_CANONICAL;
    else {
        y = Fr::from_mont(p.y);
        flags = cd_larger<FrCfg>(Fr::from_mont(p.x)) ? 1u << 31 : 0;
    }
    cd_store(out + (size_t)i * 32, y, flags);
    status[i] = (uint8_t)st;
#endif
}

// ---- the roots alone ------------------------------------------------------------------------------------------------------------------
// field 0 Fq, 1 Fq2 (two elements per item), 2 Fr; a: canonical Montgomery words
__global__ __launch_bounds__(kCdBlock) void codec_sqrt_kat_kernel(int field, const Fp* __restrict__ a, Fp* __restrict__ root, uint8_t* __restrict__ is_square, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCdBlock + threadIdx.x;
    if (i >= n) return;
    bool ok;
    if (field == 0) {
        sq::Cq r;
        ok = sq::fq_sqrt(sq::red(LzOps<Fq29>::ld(a[i])), &r);
        root[i] = LzOps<Fq29>::to_wire(r);
    } else if (field == 1) {
        Fq2w w;
        w.c0 = a[2 * (size_t)i]; w.c1 = a[2 * (size_t)i + 1];
        q2::E2<1, 2> r;
        ok = sq::fq2_sqrt(q2::ldr(w), &r);
        const Fq2w rw = q2::to_wire(r);
        root[2 * (size_t)i] = rw.c0; root[2 * (size_t)i + 1] = rw.c1;
    } else {
        sq::Cr r;
        ok = sq::fr_sqrt_ratio(sq::red(LzOps<Fr29>::ld(a[i])), LzOps<Fr29>::relax<1, 2>(LzOps<Fr29>::one()), &r);
        root[i] = LzOps<Fr29>::to_wire(r);
    }
    is_square[i] = ok ? 1 : 0;
#endif
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
static uint32_t cd_grid(size_t n) { return (uint32_t)((n + kCdBlock - 1) / kCdBlock); }
static size_t cd_enc_bytes(int group) { return group == CD_G2 ? 64 : 32; }
static size_t cd_point_bytes(int group) { return group == CD_G2 ? sizeof(G2Affine) : 64; }

int codec_decompress_run(Ctx& c, int group, const uint8_t* in, size_t n, bool check_subgroup, void* out, void* d_out, uint8_t* status_out) {
    WsCarver cv;
    const auto a_in = cv.array<uint8_t>(n * cd_enc_bytes(group));
    const auto a_pts = cv.array<uint8_t>(d_out ? 0 : n * cd_point_bytes(group));
    const auto a_st = cv.array<uint8_t>(n);
    UZK_TRY(cv.reserve(c.codec_ws));
    uint8_t* d_in = cv(a_in);
    uint8_t* d_st = cv(a_st);
    void* d_pts = d_out ? d_out : static_cast<void*>(cv(a_pts));
    const uint32_t m = (uint32_t)n;
    UZK_HIP(hipMemcpyAsync(d_in, in, n * cd_enc_bytes(group), hipMemcpyHostToDevice, c.stream));
    if (group == CD_G1) {
        UZK_LAUNCH(c, "codec_g1_dec", codec_g1_dec_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, d_in, static_cast<Affine*>(d_pts), d_st, m);
    } else if (group == CD_G2) {
        UZK_LAUNCH(c, "codec_g2_dec", codec_g2_dec_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, d_in, static_cast<G2Affine*>(d_pts), d_st, m);
        if (check_subgroup) UZK_LAUNCH(c, "codec_g2_sub", codec_g2_sub_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, static_cast<G2Affine*>(d_pts), d_st, m);
    } else {
        UZK_LAUNCH(c, "codec_ed_dec", codec_ed_dec_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, d_in, static_cast<EdAffine*>(d_pts), d_st, m);
        if (check_subgroup) UZK_LAUNCH(c, "codec_ed_sub", codec_ed_sub_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, static_cast<EdAffine*>(d_pts), d_st, m);
    }
    if (!d_out) UZK_HIP(hipMemcpyAsync(out, d_pts, n * cd_point_bytes(group), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int codec_compress_run(Ctx& c, int group, const void* points, size_t n, uint8_t* out, uint8_t* status_out) {
    WsCarver cv;
    const auto a_pts = cv.array<uint8_t>(n * cd_point_bytes(group));
    const auto a_out = cv.array<uint8_t>(n * cd_enc_bytes(group));
    const auto a_st = cv.array<uint8_t>(n);
    UZK_TRY(cv.reserve(c.codec_ws));
    uint8_t *d_pts = cv(a_pts), *d_enc = cv(a_out), *d_st = cv(a_st);
    const uint32_t m = (uint32_t)n;
    UZK_HIP(hipMemcpyAsync(d_pts, points, n * cd_point_bytes(group), hipMemcpyHostToDevice, c.stream));
    if (group == CD_G1) {
        UZK_LAUNCH(c, "codec_g1_enc", codec_g1_enc_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, reinterpret_cast<const Affine*>(d_pts), d_enc, d_st, m);
    } else if (group == CD_G2) {
        UZK_LAUNCH(c, "codec_g2_enc", codec_g2_enc_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, reinterpret_cast<const G2Affine*>(d_pts), d_enc, d_st, m);
    } else {
        UZK_LAUNCH(c, "codec_ed_enc", codec_ed_enc_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, reinterpret_cast<const EdAffine*>(d_pts), d_enc, d_st, m);
    }
    UZK_HIP(hipMemcpyAsync(out, d_enc, n * cd_enc_bytes(group), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int codec_sqrt_kat_run(Ctx& c, int field, const Fp* a, size_t n, Fp* root_out, uint8_t* is_square_out) {
    const size_t per = field == 1 ? 2 : 1;
    WsCarver cv;
    const auto a_in = cv.array<Fp>(n * per);
    const auto a_out = cv.array<Fp>(n * per);
    const auto a_st = cv.array<uint8_t>(n);
    UZK_TRY(cv.reserve(c.codec_ws));
    Fp *d_in = cv(a_in), *d_out = cv(a_out);
    uint8_t* d_st = cv(a_st);
    UZK_HIP(hipMemcpyAsync(d_in, a, n * per * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, "codec_sqrt_kat", codec_sqrt_kat_kernel, dim3(cd_grid(n)), dim3(kCdBlock), 0, c.stream, field, d_in, d_out, d_st, (uint32_t)n);
    UZK_HIP(hipMemcpyAsync(root_out, d_out, n * per * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(is_square_out, d_st, n, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

}  // namespace uzk
