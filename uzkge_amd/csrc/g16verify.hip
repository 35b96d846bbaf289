// Batch Groth16 verification up to the pairing: M proofs under one verifying key are folded, under the caller's weights rho_i, into
// the G1 arguments of ONE product of M + 3 Miller loops
//     prod_i e(rho_i A_i, B_i) . e(-(sum rho) alpha, beta) . e(-sum rho_i X_i, gamma) . e(-sum rho_i C_i, delta) = 1,
//     sum rho_i X_i = (sum rho) IC_0 + sum_j (sum_i rho_i x_ij) IC_j
// (Groth16Verifier.sol verifyProof, one proof at a time, is the reference; tests/g16_verify_ref.py is the restatement on Python
// integers).  Everything per proof runs on the device; the library computes no pairing.
//
//   g16v_decode     one lane per proof: eight big-endian words (EVM order a.x a.y b.x.c1 b.x.c0 b.y.c1 b.y.c0 c.x c.y) compared with p,
//                   into Montgomery form; the curve equation of A and C in Fq, of B in Fq2 on the lazy limbs (fq2_29.hpp)
//   g16v_subgroup   one lane per proof: [r] B by double-and-add over g2_29.hpp's G2P (the bits of r are the same for every lane, so
//                   a wave runs one control flow); then the masked weight of the proof (0 unless its status is 0)
//   g16v_reduce     one workgroup per public input: t_0 = sum rho_i, t_j = sum_i rho_i x_ij over the batch in Fr (no atomics)
//   g16v_amul       one lane per item: rho_i A_i for the M proofs and t_0 alpha as item M, double-and-add over the full 254 bits of the
//                   scalar, then the affine map with the inversion in the same lane
//   two MSMs        X over the key's l resident points, C over the M fresh points, through msm_run (what the PlonK fold uses)
//
// The two chains are one lane per item.  A G2P addition keeps four Fq2 coordinates of both operands and a dozen products alive: spread
// over a quad (ecquad29.hpp's arrangement) it would need that header's cross-lane selects rewritten for pairs of limbs vectors, and
// the chain would still be 254 doublings long -- the latency of a fold is the chain length, not the lane count (52 proofs are one
// wave either way).  The shorter chain is an endomorphism criterion for B (a 127-bit multiplication); see DESIGN.md.
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "fq12_29.hpp"
#include "g2_29.hpp"
#include "handles.hpp"
#include "host_math.hpp"
#include "lane_tools.hpp"

namespace uzk {

constexpr uint32_t kGvBlock = 64;
constexpr uint32_t kGvWords = 8;
static_assert(kGvWords * 32 == UZK_G16_PROOF_BYTES, "a blob is eight 32-byte words");
enum { GV_OK = 0, GV_NOT_CANONICAL = 1, GV_OFF_CURVE = 2, GV_NOT_IN_SUBGROUP = 3 };

// ---- decode and check -----------------------------------------------------------------------------------------------------------
// A proof with a nonzero status leaves infinities in the three point arrays.  The twist has r (2 p - r) points, an odd number, so no
// point of it has order two: y = 0 with x != 0 fails the curve equation, and G2P's affine form (y = 0 <=> infinity) loses nothing.
__global__ __launch_bounds__(kGvBlock) void g16v_decode_kernel(const uint8_t* __restrict__ proofs, Affine* __restrict__ pa, G2Affine* __restrict__ pb,
                                                                Affine* __restrict__ pc, uint8_t* __restrict__ status, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kGvBlock + threadIdx.x;
    if (i >= m) return;
    const uint8_t* blob = proofs + (size_t)i * UZK_G16_PROOF_BYTES;
    Fp w[kGvWords];
    bool canonical = true;
#pragma unroll
    for (uint32_t t = 0; t < kGvWords; ++t) {                     // unrolled: w stays in registers
        const Fp v = load_be32(blob + 32 * t);
        canonical = canonical && below_modulus<FqCfg>(v);
        w[t] = Fq::to_mont(v);
    }
    Affine a, c;
    G2Affine b;
    a.x = w[0]; a.y = w[1];
    b.x.c1 = w[2]; b.x.c0 = w[3]; b.y.c1 = w[4]; b.y.c0 = w[5];
    c.x = w[6]; c.y = w[7];
    uint32_t st = GV_OK;
    if (!canonical) st = GV_NOT_CANONICAL;
    else {
        const bool b_inf = fq2w_is_zero(b.x) && fq2w_is_zero(b.y);
        if (!affine_is_inf(a) && !g1_on_curve(a)) st = GV_OFF_CURVE;
        else if (!affine_is_inf(c) && !g1_on_curve(c)) st = GV_OFF_CURVE;
        else if (!b_inf && !g2_on_twist(b)) st = GV_OFF_CURVE;
    }
    if (st != GV_OK) {
        a.x = Fq::zero(); a.y = a.x; c = a;
        b.x = fq2w_zero(); b.y = b.x;
    }
    pa[i] = a; pb[i] = b; pc[i] = c;
    status[i] = (uint8_t)st;
#endif
}

// ---- [r] B = O, and the masked weights --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGvBlock) void g16v_subgroup_kernel(Affine* __restrict__ pa, G2Affine* __restrict__ pb, Affine* __restrict__ pc,
                                                                  const Fp* __restrict__ rho, uint8_t* __restrict__ status, Fp* __restrict__ wm, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kGvBlock + threadIdx.x;
    if (i >= m) return;                                            // no barrier and no cross-lane move below
    uint32_t st = status[i];
    if (st == GV_OK && !g2_in_subgroup(g2p_from_affine(pb[i]))) {
        st = GV_NOT_IN_SUBGROUP;
        Affine z;
        z.x = Fq::zero(); z.y = z.x;
        G2Affine z2;
        z2.x = fq2w_zero(); z2.y = z2.x;
        pa[i] = z; pc[i] = z; pb[i] = z2;
        status[i] = (uint8_t)st;
    }
    wm[i] = st == GV_OK ? rho[i] : Fr::zero();
#endif
}

// t[0] = sum_i wm_i, t[j] = sum_i wm_i x_i(j-1): one workgroup per j
__global__ __launch_bounds__(256) void g16v_reduce_kernel(const Fp* __restrict__ wm, const Fp* __restrict__ pub, uint32_t m, uint32_t n_pub,
                                                           Fp* __restrict__ t) {
    __shared__ Fp part[256];
    const uint32_t j = blockIdx.x, th = threadIdx.x;
    Fp acc = Fr::zero();
    for (uint32_t i = th; i < m; i += 256) acc = Fr::add(acc, j == 0 ? wm[i] : Fr::mul(wm[i], pub[(size_t)i * n_pub + j - 1]));
    part[th] = acc;
    __syncthreads();
    for (uint32_t step = 128; step > 0; step >>= 1) {
        if (th < step) part[th] = Fr::add(part[th], part[th + step]);
        __syncthreads();
    }
    if (th == 0) t[j] = part[0];
}

// ---- rho_i A_i and t_0 alpha as canonical affine points ------------------------------------------------------------------------------
__global__ __launch_bounds__(kGvBlock) void g16v_amul_kernel(const Affine* __restrict__ pa, const Fp* __restrict__ wm, const Fp* __restrict__ t, Affine alpha,
                                                              Affine* __restrict__ out, uint32_t m) {
    const uint32_t i = blockIdx.x * kGvBlock + threadIdx.x;
    if (i > m) return;
    const Affine p = i < m ? pa[i] : alpha;
    const Fp s = Fr::from_mont(i < m ? wm[i] : t[0]);              // canonical: below r < 2^254
    out[i] = xyzz_to_affine_lane(g1_mul_lane(p, s));
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------
struct GvEntry {
    int device = 0;
    uint32_t n_inputs = 0;
    Affine alpha;
    Affine* d_ic = nullptr;        // gamma_abc_g1: n_inputs points
};
static HandleTable<GvEntry> g_gv(6ull << 59);

// frees the key's device memory; the calling thread's current device is left as it was
static void g16v_key_free(const GvEntry& e) {
    DeviceGuard on(e.device);
    if (e.d_ic) (void)hipFree(e.d_ic);
}

int g16v_key_check(const uzk_g16_vk_desc* d) {
    if (d->n_inputs < 1 || d->n_inputs > UZK_G16_VERIFY_MAX_INPUTS) {
        set_error("uzk_g16_vk_create: %u inputs (the constant one included: 1 .. %d)", d->n_inputs, UZK_G16_VERIFY_MAX_INPUTS);
        return UZK_ERR_PARAMETER;
    }
    if (!d->gamma_abc_g1) { set_error("uzk_g16_vk_create: gamma_abc_g1 is null"); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

int g16v_key_create(Ctx& c, const uzk_g16_vk_desc* d, uint64_t* out) {
    GvEntry e;
    e.device = c.device; e.n_inputs = d->n_inputs;
    std::memcpy(&e.alpha, &d->alpha_g1, sizeof e.alpha);
    const size_t bytes = (size_t)d->n_inputs * sizeof(Affine);
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&e.d_ic), bytes);
    if (err == hipSuccess) err = hipMemcpyAsync(e.d_ic, d->gamma_abc_g1, bytes, hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c.stream);  // the caller's array may go away
    if (err != hipSuccess) {
        (void)hipGetLastError();
        g16v_key_free(e);
        set_error("uzk_g16_vk_create: %s", hipGetErrorString(err));
        return UZK_ERR_DEVICE;
    }
    *out = g_gv.insert(e);
    return UZK_OK;
}

bool g16v_key_known(uint64_t h, uint32_t* n_inputs, int* device) {
    GvEntry e;
    if (!g_gv.get(h, &e)) return false;
    if (n_inputs) *n_inputs = e.n_inputs;
    if (device) *device = e.device;
    return true;
}

// The caller makes sure no fold over this key is still running.
int g16v_key_release(uint64_t h) {
    GvEntry e;
    if (!g_gv.take(h, &e)) { set_error("uzk_g16_vk_release: unknown verifying key %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    g16v_key_free(e);
    return UZK_OK;
}

void g16v_release_all() { g_gv.drain(g16v_key_free); }

// ---- the fold -----------------------------------------------------------------------------------------------------------------
// The G1 arguments of the last three pairs: -(t_0 alpha) from the scalar multiplications' array, -X and -C from the MSMs' Jacobian sums
// (X / Z^2, Y / Z^3), brought to affine with the inversion in the lane.  Three lanes; no barrier.
// out may be alpha_w: lane 0 reads its point before it writes it, the other lanes write behind it
__global__ __launch_bounds__(kGvBlock) void g16v_tail_kernel(const Affine* alpha_w, const Jac* __restrict__ xc, Affine* out) {
    const uint32_t t = threadIdx.x;
    if (t >= 3) return;
    Affine r;
    r.x = Fq::zero(); r.y = r.x;
    if (t == 0) {
        if (!affine_is_inf(*alpha_w)) { r.x = alpha_w->x; r.y = Fq::neg(alpha_w->y); }
    } else {
        r = jac_to_affine_lane(xc[t - 1]);
        r.y = Fq::neg(r.y);                                        // 0 stays 0
    }
    out[t] = r;
}

struct GvKeep {            // where a fold left rho_i A_i (then t_0 alpha) and B_i, each with room for the product's three further pairs
    const char* who = "uzk_g16_verify_batch";
    Affine* d_ra = nullptr;
    G2Affine* d_b = nullptr;
    Jac* d_xc = nullptr;
};
static int g16v_fold_impl(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pub, uint32_t m, const Fp* weights, Affine* a_out, G2Affine* b_out,
                          Jac* alpha_out, Jac* x_out, Jac* c_out, uint8_t* status_out, GvKeep* keep);

// m >= 1.  a_out, b_out: m points each; alpha_out, x_out, c_out: one Jacobian point each.
int g16v_fold_run(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pub, uint32_t m, const Fp* weights, Affine* a_out, G2Affine* b_out,
                  Jac* alpha_out, Jac* x_out, Jac* c_out, uint8_t* status_out) {
    return g16v_fold_impl(c, h, proofs, pub, m, weights, a_out, b_out, alpha_out, x_out, c_out, status_out, nullptr);
}

// The fold's kernels, then prod_i e(rho_i A_i, B_i) e(-t_0 alpha, beta) e(-X, gamma) e(-C, delta): rho_i A_i and B_i go from the
// fold's workspace to the Miller loops without leaving the device; the two MSM sums come back from msm_run as Jacobian points and
// are brought to affine and negated on the device.  *bad_g2_out < 3: that point of g2 failed the product's check.
int g16v_verify_run(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pub, uint32_t m, const Fp* weights, const G2Affine* g2, uint8_t* status_out,
                    Fq12w* gt_out, uint32_t* bad_g2_out) {
    GvKeep k;
    Jac xc[2], al;
    UZK_TRY(g16v_fold_impl(c, h, proofs, pub, m, weights, nullptr, nullptr, &al, &xc[0], &xc[1], status_out, &k));
    UZK_HIP(hipMemcpyAsync(k.d_xc, xc, sizeof xc, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(k.d_b + m, g2, 3 * sizeof(G2Affine), hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, "g16v_tail", g16v_tail_kernel, dim3(1), dim3(kGvBlock), 0, c.stream, k.d_ra + m, k.d_xc, k.d_ra + m);                            // t_0 alpha is replaced by its negative where it lies; -X and -C follow it
    uint32_t bad = m + 3;
    uint8_t bad_status = 0;
    UZK_TRY(pairing_product_run(c, k.d_ra, k.d_b, true, m + 3, gt_out, &bad, &bad_status));   // synchronises: xc and g2 were read
    // the fold's own points passed the same checks in g16v_decode; only the caller's three can fail here
    *bad_g2_out = bad >= m && bad < m + 3 ? bad - m : 3;
    if (bad < m) { set_error("uzk_g16_verify_batch: pair %u of the fold failed the product's check", bad); return UZK_ERR_DEVICE; }
    return UZK_OK;
}

static int g16v_fold_impl(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pub, uint32_t m, const Fp* weights, Affine* a_out, G2Affine* b_out,
                          Jac* alpha_out, Jac* x_out, Jac* c_out, uint8_t* status_out, GvKeep* keep) {
    GvEntry e;
    const char* who = keep ? keep->who : "uzk_g16_verify_fold";
    if (!g_gv.get(h, &e)) { set_error("%s: unknown verifying key %llu", who, (unsigned long long)h); return UZK_ERR_PARAMETER; }
    if (e.device != c.device) { set_error("%s: the key lives on device %d, the calling context on device %d", who, e.device, c.device); return UZK_ERR_PARAMETER; }
    const uint32_t n_pub = e.n_inputs - 1;
    WsCarver cv;
    const auto a_proofs = cv.array<uint8_t>((size_t)m * UZK_G16_PROOF_BYTES);
    const auto a_pub = cv.array<Fp>((size_t)m * n_pub), a_rho = cv.array<Fp>(m), a_wm = cv.array<Fp>(m);
    const auto a_status = cv.array<uint8_t>(m);
    const auto a_a = cv.array<Affine>(m);
    const auto a_b = cv.array<G2Affine>((size_t)m + 3);
    const auto a_c = cv.array<Affine>(m);
    const auto a_t = cv.array<Fp>(e.n_inputs);
    const auto a_ra = cv.array<Affine>((size_t)m + 3);             // m + 1 of them for a fold; the product's pairs lie behind
    const auto a_xc = cv.array<Jac>(2);
    UZK_TRY(cv.reserve(c.g16v_ws));
    uint8_t *d_proofs = cv(a_proofs), *d_status = cv(a_status);
    Fp *d_pub = cv(a_pub), *d_rho = cv(a_rho), *d_wm = cv(a_wm), *d_t = cv(a_t);
    Affine *d_a = cv(a_a), *d_c = cv(a_c), *d_ra = cv(a_ra);
    G2Affine* d_b = cv(a_b);
    if (keep) {
        keep->d_ra = d_ra; keep->d_b = d_b; keep->d_xc = cv(a_xc);
    }
    const Fp one = Fr::one();
    UZK_HIP(hipMemcpyAsync(d_proofs, proofs, (size_t)m * UZK_G16_PROOF_BYTES, hipMemcpyHostToDevice, c.stream));
    if (n_pub) UZK_HIP(hipMemcpyAsync(d_pub, pub, (size_t)m * n_pub * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_rho, weights ? weights : &one, (size_t)m * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    const unsigned grid = (m + kGvBlock - 1) / kGvBlock;
    UZK_LAUNCH(c, "g16v_decode", g16v_decode_kernel, dim3(grid), dim3(kGvBlock), 0, c.stream, d_proofs, d_a, d_b, d_c, d_status, m);
    UZK_LAUNCH(c, "g16v_subgroup", g16v_subgroup_kernel, dim3(grid), dim3(kGvBlock), 0, c.stream, d_a, d_b, d_c, d_rho, d_status, d_wm, m);
    UZK_LAUNCH(c, "g16v_reduce", g16v_reduce_kernel, dim3(e.n_inputs), dim3(256), 0, c.stream, d_wm, d_pub, m, n_pub, d_t);
    UZK_LAUNCH(c, "g16v_amul", g16v_amul_kernel, dim3((m + 1 + kGvBlock - 1) / kGvBlock), dim3(kGvBlock), 0, c.stream, d_a, d_wm, d_t, e.alpha, d_ra, m);
    Affine alpha_w;                                                // t_0 alpha, read after the last synchronisation
    UZK_HIP(hipMemcpyAsync(status_out, d_status, m, hipMemcpyDeviceToHost, c.stream));
    if (a_out) UZK_HIP(hipMemcpyAsync(a_out, d_ra, (size_t)m * sizeof(Affine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(&alpha_w, d_ra + m, sizeof(Affine), hipMemcpyDeviceToHost, c.stream));
    if (b_out) UZK_HIP(hipMemcpyAsync(b_out, d_b, (size_t)m * sizeof(G2Affine), hipMemcpyDeviceToHost, c.stream));
    if (c.prof_on) UZK_HIP(hipStreamSynchronize(c.stream));        // so that the two host sections below time the MSMs alone
    int rc;
    {
        HostScope hs(c, "host_g16v_msm_x");
        rc = msm_run(c, e.d_ic, ScalarView::dense(d_t, e.n_inputs), e.n_inputs, 1, x_out, 0, 0, 0);
    }
    if (rc == UZK_OK) {
        HostScope hs(c, "host_g16v_msm_c");
        rc = msm_run(c, d_c, ScalarView::dense(d_wm, m), m, 1, c_out, 0, 0, 0);
    }
    // also on failure: the copies into the caller's arrays are queued on this stream and must not outlive the call
    const hipError_t se = hipStreamSynchronize(c.stream);
    UZK_TRY(rc);
    UZK_HIP(se);
    if (affine_is_inf(alpha_w)) *alpha_out = jac_inf();
    else { alpha_out->x = alpha_w.x; alpha_out->y = alpha_w.y; alpha_out->z = Fq::one(); }
    return UZK_OK;
}

}  // namespace uzk
