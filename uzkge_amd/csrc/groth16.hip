// Groth16 prover on a resident proving key (uzk_g16_*): key registry, the witness map (sparse products, transforms, the pointwise
// quotient), the scalar rows of the four MSMs and the host finish.  Design: DESIGN.md, "Groth16 prover".
//
// One group of up to UZK_G16_GROUP proofs (`nb` assignments z of m elements each, on the device):
//   g16_transpose     zT[i * nb + w] = z[w * m + i]: the gathers below read nb consecutive elements per column
//   g16_spmv_slices   one lane per (slice, witness): the rows of A, B, C (one matrix of 3 n_constraints rows) are cut into slices of at
//                     most kSlice entries on the host when the key is made -- a bit-decomposition row of 254 entries becomes 8 slices,
//                     so no lane walks a fat row while its wave waits; partial sums to HBM
//   g16_spmv_rows     one lane per (matrix, domain point, witness): the sum of the row's partials, the input-consistency rows of a
//                     (a[n_constraints + j] = z[j]) and the zero padding, written straight into the transform buffers
//   ntt_run           3 nb inverse transforms, 3 nb forward transforms over the coset 5 H
//   g16_pointwise     t = (a o b - c) / (5^n - 1)
//   ntt_run           nb inverse coset transforms: h
//   g16_scalar_rows   the scalar vectors of the MSMs: the tail (1, r) of A, z || 1 || s for B in G1 and G2,
//                     z[l ..] || h[0 .. n - 1) || -r s for K
//   msm_dispatch_view (A, B1, K) and g2_msm_run (B), then on the host C = s A + r B1 + K and the affine maps.
// uzk_g16_prove_batch_finish shares all of it up to the MSMs, lets the G2 MSM end on the device (g2_msm_finish_run), uploads the three
// G1 sums and finishes there: g16_chains (s A, r B1), g16_combine (C and the affine maps), g16_encode (the verifier's blob).
#include <algorithm>
#include <cstring>

#include "ctx.hpp"
#include "g2_29.hpp"
#include "handles.hpp"
#include "host_ec64.hpp"
#include "host_g2.hpp"
#include "host_math.hpp"
#include "lane_tools.hpp"

namespace uzk {

namespace {
constexpr uint32_t kSlice = 32;                 // entries of a row one lane multiplies
constexpr uint32_t kGroup = UZK_G16_GROUP;      // the G2 MSM's group: proofs of one launch sequence
constexpr uint32_t kFinBlock = 64;               // lanes of a workgroup of the finish kernels
constexpr uint64_t kGroupElems = 1ull << 21;    // elements of one group's longest row at most (g16_group; transform buffers: 3 x 64 MiB)

struct Slice {
    uint32_t start, len;                        // entries [start, start + len) of the concatenated col / val arrays
};

struct G16Key {
    uint32_t m = 0, l = 0, nc = 0, n_slices = 0;
    uint64_t n = 0, nnz = 0;
    int device = 0;
    Affine *ga = nullptr, *gb1 = nullptr, *gk = nullptr;
    G2Affine* gb2 = nullptr;
    uint32_t *col = nullptr, *row_slice = nullptr;      // row_slice[3 nc + 1]: first slice of a row
    Fp* val = nullptr;
    Slice* slices = nullptr;
    Fp shift, shift_inv, zh_inv;                        // 5, 1 / 5, 1 / (5^n - 1)
};

struct G16Work {
    DevBuf z_in, zT, part, abc, tail_a, row_b, row_k, rs;
    DevBuf fin_sums, fin_terms, fin_a, fin_b, fin_c, fin_proofs, fin_blobs, fin_test;     // the device finish
};

HandleTable<G16Key> g_reg(1ull << 58);
static_assert(sizeof(uzk_g16_key_desc) == 592 && sizeof(uzk_g16_proof) == 256, "the layouts the Python and Rust bindings mirror");

// frees the key's device memory; the calling thread's current device is left as it was
void key_free(const G16Key& k) {
    DeviceGuard on(k.device);
    void* ptrs[] = {k.ga, k.gb1, k.gk, k.gb2, k.col, k.row_slice, k.val, k.slices};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
}
}  // namespace

// ---- kernels ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void g16_transpose_kernel(const Fp* __restrict__ z, Fp* __restrict__ zT, uint32_t m, uint32_t nb) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * nb) return;
    const uint32_t w = (uint32_t)(t % nb), i = (uint32_t)(t / nb);
    zT[t] = z[(uint64_t)w * m + i];
}

// part[s * nb + w] = sum over slice s of val[k] * z_w[col[k]]
__global__ __launch_bounds__(256) void g16_spmv_slices_kernel(const Slice* __restrict__ slices, const uint32_t* __restrict__ col, const Fp* __restrict__ val,
                                                              const Fp* __restrict__ zT, Fp* __restrict__ part, uint32_t n_slices, uint32_t nb) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_slices * nb) return;
    const uint32_t w = (uint32_t)(t % nb);
    const Slice s = slices[t / nb];
    Fp acc = Fr::zero();
    for (uint32_t k = s.start; k < s.start + s.len; ++k) acc = Fr::add(acc, Fr::mul(val[k], zT[(uint64_t)col[k] * nb + w]));
    part[t] = acc;
}

// abc[(mat * nb + w) * n + i]: row i of matrix `mat` times z_w for i < nc; z_w[i - nc] for the l input-consistency rows of a; zero beyond
__global__ __launch_bounds__(256) void g16_spmv_rows_kernel(const uint32_t* __restrict__ row_slice, const Fp* __restrict__ part, const Fp* __restrict__ zT,
                                                            Fp* __restrict__ abc, uint32_t nc, uint32_t l, uint64_t n, uint32_t nb) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * n * nb) return;
    const uint32_t w = (uint32_t)(t % nb);
    const uint64_t r = t / nb, i = r % n;
    const uint32_t mat = (uint32_t)(r / n);
    Fp acc = Fr::zero();
    if (i < nc) {
        const uint32_t row = mat * nc + (uint32_t)i;
        for (uint32_t s = row_slice[row]; s < row_slice[row + 1]; ++s) acc = Fr::add(acc, part[(uint64_t)s * nb + w]);
    } else if (mat == 0 && i < (uint64_t)nc + l) {
        acc = zT[(i - nc) * nb + w];
    }
    abc[((uint64_t)mat * nb + w) * n + i] = acc;
}

// a[i] = (a[i] b[i] - c[i]) zh_inv over the `count` points of a group; b and c follow a at distance `count`
__global__ __launch_bounds__(256) void g16_pointwise_kernel(Fp* __restrict__ abc, uint64_t count, Fp zh_inv) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    abc[i] = Fr::mul(Fr::sub(Fr::mul(abc[i], abc[count + i]), abc[2 * count + i]), zh_inv);
}

// proof b = blockIdx.y:  tail_a = (1, r);  row_b = z || 1 || s;  row_k = z[l ..] || h[0 .. n - 1) || -r s
__global__ __launch_bounds__(256) void g16_scalar_rows_kernel(const Fp* __restrict__ z, const Fp* __restrict__ h, const Fp* __restrict__ rs, Fp* __restrict__ tail_a,
                                                              Fp* __restrict__ row_b, Fp* __restrict__ row_k, uint32_t m, uint32_t l, uint64_t n, uint32_t nb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t b = blockIdx.y;
    const uint64_t len_b = (uint64_t)m + 2, len_k = (uint64_t)(m - l) + n;
    const Fp r = rs[b], s = rs[nb + b];
    if (i < m) row_b[b * len_b + i] = z[(uint64_t)b * m + i];
    else if (i == m) { row_b[b * len_b + i] = Fr::one(); tail_a[2 * b] = Fr::one(); }
    else if (i == (uint64_t)m + 1) { row_b[b * len_b + i] = s; tail_a[2 * b + 1] = r; }
    if (i < m - l) row_k[b * len_k + i] = z[(uint64_t)b * m + l + i];
    else if (i < len_k - 1) row_k[b * len_k + i] = h[(uint64_t)b * n + (i - (m - l))];
    else if (i == len_k - 1) row_k[b * len_k + i] = Fr::neg(Fr::mul(r, s));
}

// ---- the finish on the device: C = s A + r B1 + K, the affine maps, the blob ---------------------------------------------------------
// One lane per (term, proof): lane t < nb is s_t A_t, lane nb + t is r_t B1_t, by double-and-add over the 254 bits of the canonical
// scalar (g1_mul_lane of lane_tools.hpp; the base is a Jacobian sum with Z != 1, so the addition is the full one).  No barrier.
__global__ __launch_bounds__(kFinBlock) void g16_chains_kernel(const Jac* __restrict__ sums, const Fp* __restrict__ rs, XYZZ* __restrict__ terms, uint32_t nb) {
    const uint32_t t = blockIdx.x * kFinBlock + threadIdx.x;
    if (t >= 2 * nb) return;
    const XYZZ p = xyzz_from_jac(sums[t]);                         // A then B1
    const Fp s = Fr::from_mont(t < nb ? rs[nb + t] : rs[t - nb]);  // s for A, r for B1; canonical: below r < 2^254
    terms[t] = g1_mul_lane(p, s);
}

// One lane per (point, proof): lane t < nb writes the affine A_t; lane nb + t adds s A + r B1 + K by general additions (the two terms
// can be equal or opposite, any operand and the sum itself can be infinite) and writes the affine C_t.  The inversion is in the lane.
__global__ __launch_bounds__(kFinBlock) void g16_combine_kernel(const Jac* __restrict__ sums, const XYZZ* __restrict__ terms, Affine* __restrict__ a_out,
                                                                 Affine* __restrict__ c_out, uint32_t nb) {
    const uint32_t t = blockIdx.x * kFinBlock + threadIdx.x;
    if (t >= 2 * nb) return;
    if (t < nb) { a_out[t] = xyzz_to_affine_lane(xyzz_from_jac(sums[t])); return; }
    const uint32_t b = t - nb;
    XYZZ acc = terms[b];
    xyzz_add(acc, terms[nb + b]);
    xyzz_add(acc, xyzz_from_jac(sums[2 * (size_t)nb + b]));
    c_out[b] = xyzz_to_affine_lane(acc);
}

// One lane per (proof, word): word t of the blob (a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0, c.x, c.y) as the canonical integer in 32
// big-endian bytes, and the same element, in Montgomery form, at its place in the struct (where c0 comes before c1).
__global__ __launch_bounds__(kFinBlock) void g16_encode_kernel(const Affine* __restrict__ pa, const G2Affine* __restrict__ pb, const Affine* __restrict__ pc,
                                                                Fp* __restrict__ proofs, uint8_t* __restrict__ blobs, uint32_t nb) {
    const uint32_t i = blockIdx.x * kFinBlock + threadIdx.x;
    if (i >= 8 * nb) return;
    const uint32_t b = i / 8, t = i % 8;
    const uint32_t slot = (t >= 2 && t < 6) ? (t ^ 1u) : t;        // the struct's word: c0 first
    const Fp v = slot < 2 ? reinterpret_cast<const Fp*>(pa)[(size_t)b * 2 + slot]
               : slot < 6 ? reinterpret_cast<const Fp*>(pb)[(size_t)b * 4 + slot - 2]
                          : reinterpret_cast<const Fp*>(pc)[(size_t)b * 2 + slot - 6];
    proofs[(size_t)b * 8 + slot] = v;
    store_be32(blobs + (size_t)b * UZK_G16_PROOF_BYTES + 32 * t, Fq::from_mont(v));
}

// ---- keys -------------------------------------------------------------------------------------------------------------------

// What a key's three sizes must satisfy, before any of its arrays is looked at; *domain_out = n.
static int g16_shape_check(uint64_t m, uint64_t l, uint64_t nc, uint64_t* domain_out) {
    if (l < 1 || l > m) { set_error("uzk_g16_key_create: n_inputs %llu must be in 1 .. n_vars %llu", (unsigned long long)l, (unsigned long long)m); return UZK_ERR_PARAMETER; }
    if (nc < 1) { set_error("uzk_g16_key_create: no constraints"); return UZK_ERR_PARAMETER; }
    uint64_t n = 1;
    while (n < nc + l) n <<= 1;
    if (!domain_supported(n)) { set_error("uzk_g16_key_create: no evaluation domain of size %llu", (unsigned long long)n); return UZK_ERR_DEGREE; }
    if (m + 2 > (1ull << UZK_MSM_G2_MAX_LOG2)) { set_error("uzk_g16_key_create: n_vars %llu exceeds the G2 MSM's 2^%d points", (unsigned long long)m, UZK_MSM_G2_MAX_LOG2); return UZK_ERR_DEGREE; }
    *domain_out = n;
    return UZK_OK;
}

// Everything that can be said about a descriptor without a device; *domain_out = n.
int g16_key_check(const uzk_g16_key_desc* d, uint64_t* domain_out) {
    if (!d) { set_error("uzk_g16_key_create: null descriptor"); return UZK_ERR_PARAMETER; }
    const uint64_t m = d->n_vars, l = d->n_inputs, nc = d->n_constraints;
    uint64_t n = 0;
    UZK_TRY(g16_shape_check(m, l, nc, &n));
    if (d->l_query_len != m - l) { set_error("uzk_g16_key_create: l_query has %llu entries, n_vars - n_inputs = %llu", (unsigned long long)d->l_query_len, (unsigned long long)(m - l)); return UZK_ERR_PARAMETER; }
    if (d->h_query_len != n - 1) { set_error("uzk_g16_key_create: h_query has %llu entries, the domain has %llu points", (unsigned long long)d->h_query_len, (unsigned long long)n); return UZK_ERR_PARAMETER; }
    if (!d->a_query || !d->b_g1_query || !d->b_g2_query || (m > l && !d->l_query) || (n > 1 && !d->h_query)) { set_error("uzk_g16_key_create: null query column"); return UZK_ERR_PARAMETER; }
    uint64_t total = 0;
    for (int k = 0; k < 3; ++k) {
        const uint64_t* rp = d->row_ptr[k];
        if (!rp) { set_error("uzk_g16_key_create: null row pointers of matrix %d", k); return UZK_ERR_PARAMETER; }
        if (rp[0] != 0) { set_error("uzk_g16_key_create: row_ptr[%d][0] is not 0", k); return UZK_ERR_PARAMETER; }
        for (uint64_t i = 0; i < nc; ++i)
            if (rp[i + 1] < rp[i]) { set_error("uzk_g16_key_create: row pointers of matrix %d decrease at row %llu", k, (unsigned long long)i); return UZK_ERR_PARAMETER; }
        const uint64_t nnz = rp[nc];
        if (nnz > 0 && (!d->col[k] || !d->val[k])) { set_error("uzk_g16_key_create: null entries of matrix %d", k); return UZK_ERR_PARAMETER; }
        total += nnz;
        if (total >= (1ull << 32)) { set_error("uzk_g16_key_create: more than 2^32 - 1 matrix entries"); return UZK_ERR_PARAMETER; }
        for (uint64_t e = 0; e < nnz; ++e)
            if (d->col[k][e] >= m) { set_error("uzk_g16_key_create: matrix %d, entry %llu: column %u >= n_vars %llu", k, (unsigned long long)e, d->col[k][e], (unsigned long long)m); return UZK_ERR_PARAMETER; }
    }
    *domain_out = n;
    return UZK_OK;
}

template <class T>
static int upload(Ctx& c, T** d_out, const std::vector<T>& v) {
    *d_out = nullptr;
    if (v.empty()) return UZK_OK;
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(d_out), v.size() * sizeof(T)));
    UZK_HIP(hipMemcpyAsync(*d_out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c.stream));
    return UZK_OK;
}

static int key_upload(Ctx& c, const uzk_g16_key_desc* d, G16Key& k) {
    const uint32_t m = k.m, l = k.l, nc = k.nc;
    const Affine *aq = reinterpret_cast<const Affine*>(d->a_query), *bq = reinterpret_cast<const Affine*>(d->b_g1_query),
                 *lq = reinterpret_cast<const Affine*>(d->l_query), *hq = reinterpret_cast<const Affine*>(d->h_query);
    Affine alpha, beta, delta;
    std::memcpy(&alpha, &d->alpha_g1, sizeof alpha); std::memcpy(&beta, &d->beta_g1, sizeof beta); std::memcpy(&delta, &d->delta_g1, sizeof delta);
    std::vector<Affine> ga(aq, aq + m), gb1(bq, bq + m), gk;
    ga.push_back(alpha); ga.push_back(delta);
    gb1.push_back(beta); gb1.push_back(delta);
    gk.reserve((size_t)(m - l) + k.n);
    if (m > l) gk.insert(gk.end(), lq, lq + (m - l));
    if (k.n > 1) gk.insert(gk.end(), hq, hq + (k.n - 1));
    gk.push_back(delta);
    const G2Affine* b2 = reinterpret_cast<const G2Affine*>(d->b_g2_query);
    std::vector<G2Affine> gb2(b2, b2 + m);
    G2Affine beta2, delta2;
    std::memcpy(&beta2, &d->beta_g2, sizeof beta2); std::memcpy(&delta2, &d->delta_g2, sizeof delta2);
    gb2.push_back(beta2); gb2.push_back(delta2);
    // the three matrices as one of 3 nc rows; every row cut into slices of at most kSlice entries
    std::vector<uint32_t> col, row_slice((size_t)3 * nc + 1);
    std::vector<Fp> val;
    std::vector<Slice> slices;
    col.reserve(k.nnz); val.reserve(k.nnz);
    for (int mat = 0; mat < 3; ++mat) {
        const uint64_t* rp = d->row_ptr[mat];
        const uint32_t base = (uint32_t)col.size();
        if (rp[nc] > 0) {
            col.insert(col.end(), d->col[mat], d->col[mat] + rp[nc]);
            const Fp* v = reinterpret_cast<const Fp*>(d->val[mat]);
            val.insert(val.end(), v, v + rp[nc]);
        }
        for (uint32_t i = 0; i < nc; ++i) {
            row_slice[(size_t)mat * nc + i] = (uint32_t)slices.size();
            for (uint64_t lo = rp[i]; lo < rp[i + 1]; lo += kSlice)
                slices.push_back(Slice{base + (uint32_t)lo, (uint32_t)std::min<uint64_t>(kSlice, rp[i + 1] - lo)});
        }
    }
    row_slice[(size_t)3 * nc] = (uint32_t)slices.size();
    k.n_slices = (uint32_t)slices.size();
    UZK_TRY(upload(c, &k.ga, ga));
    UZK_TRY(upload(c, &k.gb1, gb1));
    UZK_TRY(upload(c, &k.gk, gk));
    UZK_TRY(upload(c, &k.gb2, gb2));
    UZK_TRY(upload(c, &k.col, col));
    UZK_TRY(upload(c, &k.val, val));
    UZK_TRY(upload(c, &k.slices, slices));
    UZK_TRY(upload(c, &k.row_slice, row_slice));
    UZK_HIP(hipStreamSynchronize(c.stream));          // the host vectors go out of scope
    return UZK_OK;
}

int g16_key_create(Ctx& c, const uzk_g16_key_desc* d, uint64_t* out) {
    G16Key k;
    UZK_TRY(g16_key_check(d, &k.n));
    k.m = d->n_vars; k.l = d->n_inputs; k.nc = d->n_constraints;
    k.nnz = d->row_ptr[0][k.nc] + d->row_ptr[1][k.nc] + d->row_ptr[2][k.nc];
    k.device = c.device;
    k.shift = fr_from_u64(5);
    k.shift_inv = fr_inv(k.shift);
    k.zh_inv = fr_inv(Fr::sub(f_pow_u64<Fr>(k.shift, k.n), Fr::one()));
    const int rc = key_upload(c, d, k);
    if (rc != UZK_OK) { (void)hipStreamSynchronize(c.stream); key_free(k); return rc; }
    *out = g_reg.insert(k);
    return UZK_OK;
}

static bool key_lookup(uint64_t h, G16Key* out) { return g_reg.get(h, out); }
bool g16_key_known(uint64_t h, uint32_t* n_vars, uint32_t* n_inputs, uint32_t* n_constraints, uint64_t* domain, int* device) {
    G16Key k;
    if (!key_lookup(h, &k)) return false;
    if (n_vars) *n_vars = k.m;
    if (n_inputs) *n_inputs = k.l;
    if (n_constraints) *n_constraints = k.nc;
    if (domain) *domain = k.n;
    if (device) *device = k.device;
    return true;
}
bool g16_key_release(uint64_t h) {
    G16Key k;
    if (!g_reg.take(h, &k)) return false;
    key_free(k);
    return true;
}
void g16_release_all() { g_reg.drain(key_free); }

// ---- the prover -------------------------------------------------------------------------------------------------------------

static G16Work& work(Ctx& c) {
    if (!c.g16) c.g16 = new G16Work();
    return *static_cast<G16Work*>(c.g16);
}
void g16_free(Ctx& c) {
    if (!c.g16) return;
    G16Work* w = static_cast<G16Work*>(c.g16);
    w->z_in.release(); w->zT.release(); w->part.release(); w->abc.release(); w->tail_a.release(); w->row_b.release(); w->row_k.release(); w->rs.release();
    w->fin_sums.release(); w->fin_terms.release(); w->fin_a.release(); w->fin_b.release(); w->fin_c.release(); w->fin_proofs.release(); w->fin_blobs.release();
    w->fin_test.release();
    delete w;
    c.g16 = nullptr;
}

// Proofs of one launch sequence for a key of domain n with m variables, l of them inputs: at most kGroup, and as many as keep the
// longest per-proof row within kGroupElems elements in all -- the domain (the transform buffers), the row of B (m + 2: z_in, zT,
// row_b) and the row of K ((m - l) + n: row_k, the longest MSM).  Every G1 MSM of such a group is one msm.hip admits
// (uzk_test_g16_plan; tests/test_gpu_g16_large.py sweeps the accepted shapes).
static uint32_t g16_group(uint64_t n, uint64_t m, uint64_t l) {
    const uint64_t longest = std::max<uint64_t>(m + 2, (m - l) + n);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kGroup, kGroupElems / longest));
}
static uint32_t group_of(const G16Key& k) { return g16_group(k.n, k.m, k.l); }

// uzk_test_g16_plan: the shape rules of a key and the plan of its groups, with no key; the lengths of the MSMs A, B1, K and whether
// msm.hip takes each at batch = group under this context's tuning.  Launches nothing, reserves nothing.
int g16_plan_test(Ctx& c, uint32_t m, uint32_t l, uint32_t nc, uint32_t* group_out, uint64_t lens_out[3], int admitted_out[3]) {
    uint64_t n = 0;
    UZK_TRY(g16_shape_check(m, l, nc, &n));
    const uint32_t group = g16_group(n, m, l);
    const uint64_t lens[3] = {(uint64_t)m + 2, (uint64_t)m + 2, (uint64_t)(m - l) + n};
    *group_out = group;
    for (int i = 0; i < 3; ++i) {
        lens_out[i] = lens[i];
        admitted_out[i] = msm_admit(c, (size_t)lens[i], group, 0) == UZK_OK ? 1 : 0;
    }
    return UZK_OK;
}
static unsigned blocks(uint64_t threads) { return (unsigned)((threads + 255) / 256); }

// h of nb <= group_of(k) assignments: left in the first nb * n elements of the work buffer `abc`
static int h_group(Ctx& c, const G16Key& k, const Fp* d_z, uint32_t nb) {
    G16Work& w = work(c);
    const uint64_t n = k.n;
    UZK_TRY(w.zT.reserve((size_t)k.m * nb * sizeof(Fp)));
    UZK_TRY(w.part.reserve(std::max<size_t>(1, (size_t)k.n_slices * nb) * sizeof(Fp)));
    UZK_TRY(w.abc.reserve((size_t)3 * n * nb * sizeof(Fp)));
    Fp* abc = w.abc.as<Fp>();
    c.cur_stream = c.stream;
    UZK_LAUNCH(c, "g16_transpose", g16_transpose_kernel, dim3(blocks((uint64_t)k.m * nb)), dim3(256), 0, c.stream, d_z, w.zT.as<Fp>(), k.m, nb);
    if (k.n_slices > 0)
        UZK_LAUNCH(c, "g16_spmv_slices", g16_spmv_slices_kernel, dim3(blocks((uint64_t)k.n_slices * nb)), dim3(256), 0, c.stream, k.slices, k.col, k.val,
                   w.zT.as<Fp>(), w.part.as<Fp>(), k.n_slices, nb);
    UZK_LAUNCH(c, "g16_spmv_rows", g16_spmv_rows_kernel, dim3(blocks(3 * n * nb)), dim3(256), 0, c.stream, k.row_slice, w.part.as<Fp>(), w.zT.as<Fp>(), abc, k.nc, k.l, n, nb);
    UZK_TRY(ntt_run(c, abc, abc, n, true, nullptr, 3 * nb));
    UZK_TRY(ntt_run(c, abc, abc, n, false, &k.shift, 3 * nb));
    UZK_LAUNCH(c, "g16_pointwise", g16_pointwise_kernel, dim3(blocks(n * nb)), dim3(256), 0, c.stream, abc, n * nb, k.zh_inv);
    UZK_TRY(ntt_run(c, abc, abc, n, true, &k.shift_inv, nb));
    return UZK_OK;
}

int g16_h_run(Ctx& c, uint64_t h, const Fp* d_z, uint32_t batch, Fp* d_h) {
    G16Key k;
    if (!key_lookup(h, &k)) { set_error("uzk_g16_h_device: unknown key handle %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    const uint32_t group = group_of(k);
    for (uint32_t b0 = 0; b0 < batch; b0 += group) {
        const uint32_t nb = std::min(group, batch - b0);
        UZK_TRY(h_group(c, k, d_z + (size_t)b0 * k.m, nb));
        UZK_HIP(hipMemcpyAsync(d_h + (size_t)b0 * k.n, work(c).abc.p, (size_t)nb * k.n * sizeof(Fp), hipMemcpyDeviceToDevice, c.stream));
    }
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// k P by double-and-add over the 254 bits of the canonical scalar
static h64::J j_scalar_mul(const h64::J& p, const Fp& k_mont) {
    const Fp k = Fr::from_mont(k_mont);
    h64::J acc = h64::j_inf();
    for (int bit = 253; bit >= 0; --bit) {
        acc = h64::j_dbl(acc);
        if ((k.v[bit >> 5] >> (bit & 31)) & 1) acc = h64::j_add(acc, p);
    }
    return acc;
}

// Everything of a group up to and including the four MSMs, shared by the two finishes: proofs b0 .. b0 + nb of the call.  The G1 sums
// come back to the host (msm.hip's own final fold); B goes to jb2 on the host (the window sums combined there) or, when jb2 is null,
// to d_b2 on the device as canonical affine points (g2_msm_finish_run: nothing of B leaves the device).  w.rs holds r, then s.
static int msm_group(Ctx& c, const G16Key& k, const Fp* z, bool z_on_device, const Fp* r_host, const Fp* s_host, uint32_t b0, uint32_t nb, Jac* ja, Jac* jb1,
                     Jac* jk, G2Jac* jb2, G2Affine* d_b2) {
    G16Work& w = work(c);
    const uint32_t m = k.m;
    const uint64_t n = k.n, len_b = (uint64_t)m + 2, len_k = (uint64_t)(m - k.l) + n;
    Ctx::Srs ga, gb1, gk;
    ga.d_points = k.ga; ga.n = len_b; ga.device = k.device;
    gb1.d_points = k.gb1; gb1.n = len_b; gb1.device = k.device;
    gk.d_points = k.gk; gk.n = len_k; gk.device = k.device;
    const Fp* d_z = z + (size_t)b0 * m;
    if (!z_on_device) {
        UZK_TRY(w.z_in.reserve((size_t)nb * m * sizeof(Fp)));
        UZK_HIP(hipMemcpyAsync(w.z_in.p, z + (size_t)b0 * m, (size_t)nb * m * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
        d_z = w.z_in.as<Fp>();
    }
    UZK_TRY(w.rs.reserve((size_t)2 * group_of(k) * sizeof(Fp)));
    UZK_HIP(hipMemcpyAsync(w.rs.p, r_host + b0, (size_t)nb * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(w.rs.as<Fp>() + nb, s_host + b0, (size_t)nb * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    {
        HostScope hs(c, "host_g16_h");
        UZK_TRY(h_group(c, k, d_z, nb));
        UZK_TRY(w.tail_a.reserve((size_t)2 * nb * sizeof(Fp)));
        UZK_TRY(w.row_b.reserve((size_t)len_b * nb * sizeof(Fp)));
        UZK_TRY(w.row_k.reserve((size_t)len_k * nb * sizeof(Fp)));
        UZK_LAUNCH(c, "g16_scalar_rows", g16_scalar_rows_kernel, dim3(blocks(std::max(len_b, len_k)), nb), dim3(256), 0, c.stream, d_z, w.abc.as<Fp>(), w.rs.as<Fp>(),
                   w.tail_a.as<Fp>(), w.row_b.as<Fp>(), w.row_k.as<Fp>(), m, k.l, n, nb);
        if (c.prof_on) UZK_HIP(hipStreamSynchronize(c.stream));     // so that the stage timers below hold one stage each
    }
    {
        HostScope hs(c, "host_g16_msm_a");
        ScalarView sv;                                              // z where it lies, the tail (1, r) behind it
        sv.main = d_z; sv.stride = m; sv.n_main = m;
        sv.tail = w.tail_a.as<Fp>(); sv.tail_n = 2;
        UZK_TRY(msm_dispatch_view(ga, 0, sv, len_b, nb, ja));
    }
    {
        HostScope hs(c, "host_g16_msm_b1");
        UZK_TRY(msm_dispatch_view(gb1, 0, ScalarView::dense(w.row_b.as<Fp>(), len_b), len_b, nb, jb1));
    }
    {
        HostScope hs(c, "host_g16_msm_k");
        UZK_TRY(msm_dispatch_view(gk, 0, ScalarView::dense(w.row_k.as<Fp>(), len_k), len_k, nb, jk));
    }
    {
        HostScope hs(c, "host_g16_msm_g2");
        if (jb2) UZK_TRY(g2_msm_run(c, k.gb2, w.row_b.as<Fp>(), len_b, nb, jb2));
        else {
            UZK_TRY(g2_msm_finish_run(c, k.gb2, w.row_b.as<Fp>(), len_b, nb, nullptr, d_b2));
            if (c.prof_on) UZK_HIP(hipStreamSynchronize(c.stream)); // the stage ends with its kernels
        }
    }
    return UZK_OK;
}

int g16_prove_run(Ctx& c, uint64_t h, const Fp* z, bool z_on_device, const Fp* r_host, const Fp* s_host, uint32_t batch, uzk_g16_proof* out) {
    G16Key k;
    if (!key_lookup(h, &k)) { set_error("uzk_g16_prove_batch: unknown key handle %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    const uint32_t group = group_of(k);
    std::vector<Jac> ja(group), jb1(group), jk(group);
    std::vector<G2Jac> jb2(group);
    for (uint32_t b0 = 0; b0 < batch; b0 += group) {
        const uint32_t nb = std::min(group, batch - b0);
        UZK_TRY(msm_group(c, k, z, z_on_device, r_host, s_host, b0, nb, ja.data(), jb1.data(), jk.data(), jb2.data(), nullptr));
        HostScope hs(c, "host_g16_finish");
        for (uint32_t b = 0; b < nb; ++b) {
            const h64::J A = h64::j_from(ja[b]), B1 = h64::j_from(jb1[b]);
            const h64::J C = h64::j_add(h64::j_add(j_scalar_mul(A, s_host[b0 + b]), j_scalar_mul(B1, r_host[b0 + b])), h64::j_from(jk[b]));
            const Affine a = jac_to_affine_host(ja[b]), cc = jac_to_affine_host(h64::j_to(C));
            const G2Affine bb = h64::j2_to_affine(h64::j2_from(jb2[b]));
            uzk_g16_proof& p = out[b0 + b];
            std::memcpy(&p.a, &a, sizeof a);
            std::memcpy(&p.b, &bb, sizeof bb);
            std::memcpy(&p.c, &cc, sizeof cc);
        }
    }
    return UZK_OK;
}

// ---- the finish on the device ---------------------------------------------------------------------------------------------------
// The three G1 sums of nb proofs lie in d_sums as A[nb], B1[nb], K[nb] (Jacobian, as msm.hip returns them), r then s in d_rs:
//   g16_chains   2 nb lanes -> terms[0 .. nb) = s A, terms[nb .. 2 nb) = r B1
//   g16_combine  2 nb lanes -> d_a[b] = affine A, d_c[b] = affine (s A + r B1 + K)
static int finish_launch(Ctx& c, const Jac* d_sums, const Fp* d_rs, XYZZ* d_terms, uint32_t nb, Affine* d_a, Affine* d_c) {
    const unsigned grid = (2 * nb + kFinBlock - 1) / kFinBlock;
    UZK_LAUNCH(c, "g16_chains", g16_chains_kernel, dim3(grid), dim3(kFinBlock), 0, c.stream, d_sums, d_rs, d_terms, nb);
    UZK_LAUNCH(c, "g16_combine", g16_combine_kernel, dim3(grid), dim3(kFinBlock), 0, c.stream, d_sums, d_terms, d_a, d_c, nb);
    return UZK_OK;
}

// proofs_out (host, the struct layout), blobs_out (host) and d_blobs_out (device): UZK_G16_PROOF_BYTES per proof; at least one of them
int g16_prove_finish_run(Ctx& c, uint64_t h, const Fp* z, bool z_on_device, const Fp* r_host, const Fp* s_host, uint32_t batch, uzk_g16_proof* proofs_out,
                         uint8_t* blobs_out, uint8_t* d_blobs_out) {
    G16Key k;
    if (!key_lookup(h, &k)) { set_error("uzk_g16_prove_batch_finish: unknown key handle %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    G16Work& w = work(c);
    const uint32_t group = group_of(k);
    std::vector<Jac> sums((size_t)3 * group);
    UZK_TRY(w.fin_sums.reserve((size_t)3 * group * sizeof(Jac)));
    UZK_TRY(w.fin_terms.reserve((size_t)2 * group * sizeof(XYZZ)));
    UZK_TRY(w.fin_a.reserve((size_t)group * sizeof(Affine)));
    UZK_TRY(w.fin_b.reserve((size_t)group * sizeof(G2Affine)));
    UZK_TRY(w.fin_c.reserve((size_t)group * sizeof(Affine)));
    UZK_TRY(w.fin_proofs.reserve((size_t)group * sizeof(uzk_g16_proof)));
    if (!d_blobs_out) UZK_TRY(w.fin_blobs.reserve((size_t)group * UZK_G16_PROOF_BYTES));
    for (uint32_t b0 = 0; b0 < batch; b0 += group) {
        const uint32_t nb = std::min(group, batch - b0);
        Jac *ja = sums.data(), *jb1 = ja + nb, *jk = jb1 + nb;
        UZK_TRY(msm_group(c, k, z, z_on_device, r_host, s_host, b0, nb, ja, jb1, jk, nullptr, w.fin_b.as<G2Affine>()));
        HostScope hs(c, "host_g16_finish_device");
        UZK_HIP(hipMemcpyAsync(w.fin_sums.p, sums.data(), (size_t)3 * nb * sizeof(Jac), hipMemcpyHostToDevice, c.stream));
        UZK_TRY(finish_launch(c, w.fin_sums.as<Jac>(), w.rs.as<Fp>(), w.fin_terms.as<XYZZ>(), nb, w.fin_a.as<Affine>(), w.fin_c.as<Affine>()));
        uint8_t* d_blobs = d_blobs_out ? d_blobs_out + (size_t)b0 * UZK_G16_PROOF_BYTES : w.fin_blobs.as<uint8_t>();
        UZK_LAUNCH(c, "g16_encode", g16_encode_kernel, dim3((8 * nb + kFinBlock - 1) / kFinBlock), dim3(kFinBlock), 0, c.stream, w.fin_a.as<Affine>(),
                   w.fin_b.as<G2Affine>(), w.fin_c.as<Affine>(), w.fin_proofs.as<Fp>(), d_blobs, nb);
        if (proofs_out) UZK_HIP(hipMemcpyAsync(proofs_out + b0, w.fin_proofs.p, (size_t)nb * sizeof(uzk_g16_proof), hipMemcpyDeviceToHost, c.stream));
        if (blobs_out) UZK_HIP(hipMemcpyAsync(blobs_out + (size_t)b0 * UZK_G16_PROOF_BYTES, d_blobs, (size_t)nb * UZK_G16_PROOF_BYTES, hipMemcpyDeviceToHost, c.stream));
        UZK_HIP(hipStreamSynchronize(c.stream));                    // `sums` is reused by the next group; the results are complete on return
    }
    return UZK_OK;
}

// uzk_test_g16_finish: the chains, the combination and the affine maps on the caller's Jacobian points
int g16_finish_test_run(Ctx& c, const Jac* a, const Jac* b1, const Jac* kk, const Fp* r_host, const Fp* s_host, uint32_t n, Affine* a_out, Affine* c_out) {
    WsCarver cv;
    const auto a_sums = cv.array<Jac>((size_t)3 * n);
    const auto a_rs = cv.array<Fp>((size_t)2 * n);
    const auto a_terms = cv.array<XYZZ>((size_t)2 * n);
    const auto a_a = cv.array<Affine>(n), a_c = cv.array<Affine>(n);
    G16Work& w = work(c);
    UZK_TRY(cv.reserve(w.fin_test));
    Jac* d_sums = cv(a_sums);
    Fp* d_rs = cv(a_rs);
    UZK_HIP(hipMemcpyAsync(d_sums, a, (size_t)n * sizeof(Jac), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_sums + n, b1, (size_t)n * sizeof(Jac), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_sums + 2 * (size_t)n, kk, (size_t)n * sizeof(Jac), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_rs, r_host, (size_t)n * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_rs + n, s_host, (size_t)n * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    c.cur_stream = c.stream;
    UZK_TRY(finish_launch(c, d_sums, d_rs, cv(a_terms), n, cv(a_a), cv(a_c)));
    UZK_HIP(hipMemcpyAsync(a_out, cv(a_a), (size_t)n * sizeof(Affine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(c_out, cv(a_c), (size_t)n * sizeof(Affine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

}  // namespace uzk
