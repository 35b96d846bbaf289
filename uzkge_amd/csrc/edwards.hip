// Baby Jubjub on the device: the arithmetic a reveal is made of, batched one lane per item (ed29.hpp has the group law).
//
//   ed_check        one lane per point: canonical words, the curve equation, [L] P = identity (the bits of L are the same for every lane)
//   ed_mul          one lane per item: s_i P_i over the 256 bits of s_i by double-and-add with the unified addition, then the affine map
//                   with the inversion in the lane; a point stride of 0 shares one base
//   ed_sum          one lane per card j: sum_k P_kj over k rows of n points, or e2_j - sum_k P_kj (unmask)
//   cp_transcript   one lane per proof: Keccak-256 of the 448-byte transcript, c = digest mod L; for a prover also
//                   r = omega + c sk mod L and the proof blob
//   cp_check        ONE launch for the two chains of a verification, each kind of lane in workgroups of its own:
//                     one lane per point, five per proof (e1, reveal, pk from the statement, a and b from the 160-byte blob): decode,
//                     then ed_check's classification;
//                     one lane per equation, two per proof: r P - c Q by Straus / Shamir over the joint bits of (r, c) with the table
//                     {P, -Q, P - Q} in ONE doubling chain, compared projectively with a (or b):  r e1 = a + c reveal,  r G = b + c pk
//   cp_verdict      one lane per proof: the first failing check as the verdict byte
//   cp_prove_mul    one lane per multiplication of a batch of reveals, 3 m + 1: sk e1_i, omega_i e1_i, omega_i G and sk G
//
// Every chain is 256 unified additions-with-doubling long whatever the batch: the latency of a call is the chain, not the lane count
// (52 proofs are 104 lanes, two waves).  tests/ed_ref.py is the restatement on Python integers.
#include <cstring>

#include "ctx.hpp"
#include "ed29.hpp"

namespace uzk {

constexpr uint32_t kEdBlock = 64;
static_assert(sizeof(EdAffine) == 64, "a point is eight 64-bit words on the wire");
static_assert(UZK_CP_PROOF_BYTES == 160, "a proof is five 32-byte words");

// a 32-byte big-endian word of a blob as an integer
__device__ __forceinline__ Fp cp_word_be(const uint8_t* blob, uint32_t word) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(blob) + 8 * word;     // blobs are 160 bytes apart in a 256-byte aligned array
    Fp v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.v[j] = __builtin_bswap32(src[7 - j]);
    return v;
}
__device__ __forceinline__ void cp_store_word_be(uint8_t* blob, uint32_t word, const Fp& v) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(blob) + 8 * word;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[7 - j] = __builtin_bswap32(v.v[j]);
}

__global__ __launch_bounds__(kEdBlock) void ed_check_kernel(const EdAffine* __restrict__ pts, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= n) return;
    status[i] = (uint8_t)ed::classify(pts[i]);
#endif
}

__global__ __launch_bounds__(kEdBlock) void ed_mul_kernel(const EdAffine* __restrict__ pts, uint32_t point_stride, const Fp* __restrict__ scalars,
                                                           EdAffine* __restrict__ out, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = ed::to_affine(ed::mul(ed::from_affine(pts[(size_t)i * point_stride]), scalars[i]));
#endif
}

// out_j = sum_k rows[k n + j], or e2_j minus that sum
__global__ __launch_bounds__(kEdBlock) void ed_sum_kernel(const EdAffine* __restrict__ rows, uint32_t k, uint32_t n, const EdAffine* __restrict__ e2,
                                                           EdAffine* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t j = blockIdx.x * kEdBlock + threadIdx.x;
    if (j >= n) return;
    ed::P acc = ed::identity();
#pragma unroll 1
    for (uint32_t r = 0; r < k; ++r) acc = ed::add(acc, ed::from_affine(rows[(size_t)r * n + j]));
    if (e2) acc = ed::add(ed::from_affine(e2[j]), ed::neg(acc));
    out[j] = ed::to_affine(acc);
#endif
}

// The statement of proof i: e1, reveal, pk, each through its own pointer and stride (a verifier's buffer holds the three side by side,
// a prover has them in three arrays and one pk for all).
struct CpStatement {
    const EdAffine *e1, *reveal, *pk;
    uint32_t s_e1, s_reveal, s_pk;
};

// a (which = 0) or b (which = 1) of a blob in Montgomery words; false (and zeros) when a word is not below q
__device__ __forceinline__ bool cp_blob_point(const uint8_t* blob, uint32_t which, EdAffine* p) {
    const Fp x = cp_word_be(blob, 2 * which), y = cp_word_be(blob, 2 * which + 1);
    const bool canonical = ed_coord_canonical(x) && ed_coord_canonical(y);
    p->x = canonical ? Fr::to_mont(x) : Fr::zero();
    p->y = canonical ? Fr::to_mont(y) : Fr::zero();
    return canonical;
}

// c_i (plain words, below L) from the statement and a, b -- read from the blobs (a verifier: plain big-endian words as they are) or,
// with proofs_in == nullptr, from ab (a prover: Montgomery words of the points it has just computed); with omega also
// r_i = omega_i + c_i sk mod L and the blob a.x a.y b.x b.y r
__global__ __launch_bounds__(kEdBlock) void cp_transcript_kernel(CpStatement s, const uint8_t* __restrict__ proofs_in, const EdAffine* __restrict__ ab,
                                                                  Fp* __restrict__ c_out, const Fp* __restrict__ omega, const Fp* __restrict__ sk,
                                                                  uint8_t* __restrict__ proofs_out, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= m) return;
    const EdAffine g = ed_generator();
    const EdAffine pts[4] = {s.e1[(size_t)i * s.s_e1], g, s.reveal[(size_t)i * s.s_reveal], s.pk[(size_t)i * s.s_pk]};
    Fp w[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) { w[2 * k] = Fr::from_mont(pts[k].x); w[2 * k + 1] = Fr::from_mont(pts[k].y); }
    if (proofs_in) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[8 + k] = cp_word_be(proofs_in + (size_t)i * UZK_CP_PROOF_BYTES, k);
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) { w[8 + 2 * k] = Fr::from_mont(ab[2 * (size_t)i + k].x); w[9 + 2 * k] = Fr::from_mont(ab[2 * (size_t)i + k].y); }
    }
    const Fp c = ed_mod_order(cp_transcript_digest(w));
    c_out[i] = c;
    if (omega) {
        const Fp r = ed_muladd_order(ed_mod_order(omega[i]), c, ed_mod_order(*sk));
        uint8_t* blob = proofs_out + (size_t)i * UZK_CP_PROOF_BYTES;
#pragma unroll
        for (int k = 0; k < 4; ++k) cp_store_word_be(blob, k, w[8 + k]);
        cp_store_word_be(blob, 4, r);
    }
#endif
}

// The two chains of a verification in ONE launch, each kind of lane in workgroups of its own (a wave runs one control flow):
//   workgroups [0, point_blocks)   lane 5 i + w: point w of proof i -- 0 e1, 1 reveal, 2 pk from the statement, 3 a, 4 b from the blob --
//                                  through ed_check's classification into pst[5 i + w]
//   the workgroups behind them     lane 2 i + q: equation q of proof i into ok[2 i + q]:  r P - c Q = a (b) with P = e1 (G), Q = reveal (pk)
// The equation lanes do not wait for the points' verdicts: they refuse only what would break the limbs' contract (a word not below q)
// and compute on whatever else they are given -- cp_verdict reads an equation only where all five points passed.
__global__ __launch_bounds__(kEdBlock) void cp_check_kernel(CpStatement s, const uint8_t* __restrict__ proofs, const Fp* __restrict__ c,
                                                             uint8_t* __restrict__ pst, uint8_t* __restrict__ ok, uint32_t m, uint32_t point_blocks) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (blockIdx.x < point_blocks) {
        const uint32_t t = blockIdx.x * kEdBlock + threadIdx.x;
        if (t >= 5 * m) return;
        const uint32_t i = t / 5, w = t % 5;
        EdAffine p;
        uint32_t st = 0;
        if (w >= 3) st = cp_blob_point(proofs + (size_t)i * UZK_CP_PROOF_BYTES, w - 3, &p) ? 0 : 1;
        else p = w == 0 ? s.e1[(size_t)i * s.s_e1] : w == 1 ? s.reveal[(size_t)i * s.s_reveal] : s.pk[(size_t)i * s.s_pk];
        if (st == 0) st = ed::classify(p);
        pst[t] = (uint8_t)st;
        return;
    }
    const uint32_t t = (blockIdx.x - point_blocks) * kEdBlock + threadIdx.x;
    if (t >= 2 * m) return;
    const uint32_t i = t >> 1, q = t & 1;
    const uint8_t* blob = proofs + (size_t)i * UZK_CP_PROOF_BYTES;
    const EdAffine base = q == 0 ? s.e1[(size_t)i * s.s_e1] : ed_generator();
    const EdAffine other = q == 0 ? s.reveal[(size_t)i * s.s_reveal] : s.pk[(size_t)i * s.s_pk];
    EdAffine rhs;
    const bool canonical = cp_blob_point(blob, q, &rhs) && ed_coord_canonical(base.x) && ed_coord_canonical(base.y) && ed_coord_canonical(other.x) &&
                           ed_coord_canonical(other.y);
    if (!canonical) { ok[t] = 0; return; }
    const Fp r = cp_word_be(blob, 4);                               // any 256-bit integer: an integer multiple is defined on the whole curve
    const ed::P t1 = ed::from_affine(base), t2 = ed::neg(ed::from_affine(other)), t3 = ed::add(t1, t2);
    const ed::P lhs = ed::mul2(t1, t2, t3, r, c[i]);
    ok[t] = ed::eq_affine(lhs, ed::ld(rhs.x), ed::ld(rhs.y)) ? 1 : 0;
#endif
}

// 1 .. 3: the smallest nonzero status among the proof's five points (the codes are in the order of the checks); then 4, 5: the equations
__global__ __launch_bounds__(kEdBlock) void cp_verdict_kernel(const uint8_t* __restrict__ pst, const uint8_t* __restrict__ ok, uint8_t* __restrict__ verdict, uint32_t m) {
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= m) return;
    uint32_t v = 0;
    for (int k = 0; k < 5; ++k) {
        const uint32_t st = pst[5 * (size_t)i + k];
        if (st && (v == 0 || st < v)) v = st;
    }
    if (v == 0) v = !ok[2 * (size_t)i] ? 4 : !ok[2 * (size_t)i + 1] ? 5 : 0;
    verdict[i] = (uint8_t)v;
}

// lane 3 i + w: 0 reveal_i = sk e1_i, 1 a_i = omega_i e1_i, 2 b_i = omega_i G; lane 3 m: pk = sk G
__global__ __launch_bounds__(kEdBlock) void cp_prove_mul_kernel(const EdAffine* __restrict__ e1, const Fp* __restrict__ sk, const Fp* __restrict__ omega,
                                                                 EdAffine* __restrict__ reveal, EdAffine* __restrict__ ab, EdAffine* __restrict__ pk, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = blockIdx.x * kEdBlock + threadIdx.x;
    if (t > 3 * m) return;
    const uint32_t i = t / 3, w = t % 3;                            // t == 3 m: i = m, w = 0 -- no array is read at i then
    const bool is_pk = t == 3 * m;
    const EdAffine base = (is_pk || w == 2) ? ed_generator() : e1[i];
    const Fp k = (is_pk || w == 0) ? *sk : omega[i];
    const EdAffine r = ed::to_affine(ed::mul(ed::from_affine(base), k));
    if (is_pk) *pk = r;
    else if (w == 0) reveal[i] = r;
    else ab[2 * (size_t)i + (w - 1)] = r;
#endif
}

// The group law on RAW limbs (uzk_test_ed_raw_kat): coordinates are taken exactly as given -- nothing is re-limbed or reduced on the way
// in, nothing canonicalised on the way out -- so a test can put every coordinate at the edge of ed::C's bound.
struct EdRawPt {
    uint32_t c[4][9];                  // x, y, z, t, nine limbs each (op 5 out: eight wire words of x and y, the ninth 0)
};
struct EdRawIn {
    EdRawPt a, b;
};
struct EdRawOut {
    EdRawPt p;
    uint32_t flag;
};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ ed::C edraw_c(const uint32_t (&c)[9]) {
    ed::C r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v.l[i] = c[i];
    return r;
}
__device__ __forceinline__ void edraw_put(uint32_t (&c)[9], const ed::C& x) {
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = x.v.l[i];
}
__device__ __forceinline__ void edraw_put_wire(uint32_t (&c)[9], const Fp& w) {
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i] = w.v[i];
    c[8] = 0;
}
__device__ __forceinline__ ed::P edraw_point(const EdRawPt& r) {
    ed::P p;
    p.x = edraw_c(r.c[0]); p.y = edraw_c(r.c[1]); p.z = edraw_c(r.c[2]); p.t = edraw_c(r.c[3]);
    return p;
}
__device__ __forceinline__ void edraw_put_point(EdRawPt& r, const ed::P& p) {
    edraw_put(r.c[0], p.x); edraw_put(r.c[1], p.y); edraw_put(r.c[2], p.z); edraw_put(r.c[3], p.t);
}
#endif

// op 0 add(a, b), 1 neg(a), 2 is_identity(a), 3 eq_affine(a, b.x, b.y), 4 on_curve(a.x, a.y) (the answers in out.flag), 5 to_affine(a) as
// wire words, 6 inv(a.x)
__global__ __launch_bounds__(kEdBlock) void ed_raw_kat_kernel(int op, const EdRawIn* __restrict__ in, EdRawOut* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = (size_t)blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= n) return;
    const EdRawIn rec = in[i];
    EdRawOut r;
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 9; ++l) r.p.c[k][l] = 0;
    r.flag = 0;
    const ed::P a = edraw_point(rec.a);
    if (op == 0) edraw_put_point(r.p, ed::add(a, edraw_point(rec.b)));
    else if (op == 1) edraw_put_point(r.p, ed::neg(a));
    else if (op == 2) r.flag = ed::is_identity(a);
    else if (op == 3) r.flag = ed::eq_affine(a, edraw_c(rec.b.c[0]), edraw_c(rec.b.c[1]));
    else if (op == 4) r.flag = ed::on_curve(a.x, a.y);
    else if (op == 5) {
        const EdAffine w = ed::to_affine(a);
        edraw_put_wire(r.p.c[0], w.x); edraw_put_wire(r.p.c[1], w.y);
    } else {
        edraw_put(r.p.c[0], ed::inv(a.x));
    }
    out[i] = r;
#endif
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static size_t ed_align(size_t v) { return (v + 255) & ~(size_t)255; }
static unsigned ed_grid(size_t lanes) { return (unsigned)((lanes + kEdBlock - 1) / kEdBlock); }

// the first coordinate of `count` wire elements that is not below q, or count
size_t ed_first_noncanonical(const Fp* words, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!ed_coord_canonical(words[i])) return i;
    return count;
}

int ed_check_run(Ctx& c, const EdAffine* pts, size_t n, uint8_t* status_out) {
    const size_t o_st = ed_align(n * sizeof(EdAffine));
    UZK_TRY(c.ed_ws.reserve(o_st + ed_align(n)));
    EdAffine* d_pts = c.ed_ws.as<EdAffine>();
    uint8_t* d_st = c.ed_ws.as<uint8_t>() + o_st;
    UZK_HIP(hipMemcpyAsync(d_pts, pts, n * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    {
        KernelScope ks(c, "ed_check");
        hipLaunchKernelGGL(ed_check_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, d_pts, d_st, (uint32_t)n);
    }
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int ed_mul_run(Ctx& c, const EdAffine* pts, bool shared_base, const Fp* scalars, size_t n, EdAffine* out) {
    const size_t n_pts = shared_base ? 1 : n;
    const size_t o_sc = ed_align(n_pts * sizeof(EdAffine)), o_out = o_sc + ed_align(n * sizeof(Fp));
    UZK_TRY(c.ed_ws.reserve(o_out + ed_align(n * sizeof(EdAffine))));
    char* ws = c.ed_ws.as<char>();
    EdAffine* d_pts = reinterpret_cast<EdAffine*>(ws);
    Fp* d_sc = reinterpret_cast<Fp*>(ws + o_sc);
    EdAffine* d_out = reinterpret_cast<EdAffine*>(ws + o_out);
    UZK_HIP(hipMemcpyAsync(d_pts, pts, n_pts * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_sc, scalars, n * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    {
        KernelScope ks(c, "ed_mul");
        hipLaunchKernelGGL(ed_mul_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, d_pts, shared_base ? 0u : 1u, d_sc, d_out, (uint32_t)n);
    }
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(out, d_out, n * sizeof(EdAffine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// e2 == nullptr: the plain sum
int ed_sum_run(Ctx& c, const EdAffine* e2, const EdAffine* rows, uint32_t k, uint32_t n, EdAffine* out) {
    const size_t row_bytes = (size_t)k * n * sizeof(EdAffine), n_bytes = (size_t)n * sizeof(EdAffine);
    const size_t o_e2 = ed_align(row_bytes), o_out = o_e2 + ed_align(n_bytes);
    UZK_TRY(c.ed_ws.reserve(o_out + ed_align(n_bytes)));
    char* ws = c.ed_ws.as<char>();
    EdAffine* d_rows = reinterpret_cast<EdAffine*>(ws);
    EdAffine* d_e2 = reinterpret_cast<EdAffine*>(ws + o_e2);
    EdAffine* d_out = reinterpret_cast<EdAffine*>(ws + o_out);
    UZK_HIP(hipMemcpyAsync(d_rows, rows, row_bytes, hipMemcpyHostToDevice, c.stream));
    if (e2) UZK_HIP(hipMemcpyAsync(d_e2, e2, n_bytes, hipMemcpyHostToDevice, c.stream));
    {
        KernelScope ks(c, e2 ? "ed_unmask" : "ed_sum");
        hipLaunchKernelGGL(ed_sum_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, d_rows, k, n, e2 ? d_e2 : nullptr, d_out);
    }
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(out, d_out, n_bytes, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// statements: m x (e1, reveal, pk); proofs: m blobs; challenges_out optional (m x plain words)
int cp_verify_run(Ctx& c, const EdAffine* statements, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, Fp* challenges_out) {
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o = at; at += ed_align(bytes); return o; };
    const size_t o_stmt = carve((size_t)m * 3 * sizeof(EdAffine)), o_proofs = carve((size_t)m * UZK_CP_PROOF_BYTES), o_c = carve((size_t)m * sizeof(Fp)),
                 o_pst = carve((size_t)m * 5), o_ok = carve((size_t)m * 2), o_verdict = carve(m);
    UZK_TRY(c.ed_ws.reserve(at));
    char* ws = c.ed_ws.as<char>();
    EdAffine* d_stmt = reinterpret_cast<EdAffine*>(ws + o_stmt);
    uint8_t* d_proofs = reinterpret_cast<uint8_t*>(ws + o_proofs);
    Fp* d_c = reinterpret_cast<Fp*>(ws + o_c);
    uint8_t* d_pst = reinterpret_cast<uint8_t*>(ws + o_pst);
    uint8_t* d_ok = reinterpret_cast<uint8_t*>(ws + o_ok);
    uint8_t* d_verdict = reinterpret_cast<uint8_t*>(ws + o_verdict);
    UZK_HIP(hipMemcpyAsync(d_stmt, statements, (size_t)m * 3 * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_proofs, proofs, (size_t)m * UZK_CP_PROOF_BYTES, hipMemcpyHostToDevice, c.stream));
    CpStatement s;
    s.e1 = d_stmt; s.reveal = d_stmt + 1; s.pk = d_stmt + 2;
    s.s_e1 = s.s_reveal = s.s_pk = 3;
    {
        KernelScope ks(c, "cp_transcript");
        hipLaunchKernelGGL(cp_transcript_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, s, d_proofs, nullptr, d_c, nullptr, nullptr, nullptr, m);
    }
    UZK_HIP(hipGetLastError());
    {
        const unsigned point_blocks = ed_grid((size_t)m * 5);
        KernelScope ks(c, "cp_check");
        hipLaunchKernelGGL(cp_check_kernel, dim3(point_blocks + ed_grid((size_t)m * 2)), dim3(kEdBlock), 0, c.stream, s, d_proofs, d_c, d_pst, d_ok, m, point_blocks);
    }
    UZK_HIP(hipGetLastError());
    {
        KernelScope ks(c, "cp_verdict");
        hipLaunchKernelGGL(cp_verdict_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, d_pst, d_ok, d_verdict, m);
    }
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(verdict_out, d_verdict, m, hipMemcpyDeviceToHost, c.stream));
    if (challenges_out) UZK_HIP(hipMemcpyAsync(challenges_out, d_c, (size_t)m * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int cp_prove_run(Ctx& c, const Fp* sk, const EdAffine* e1, const Fp* omegas, uint32_t m, EdAffine* reveal_out, EdAffine* pk_out, uint8_t* proofs_out) {
    size_t at = 0;
    auto carve = [&](size_t bytes) { const size_t o = at; at += ed_align(bytes); return o; };
    const size_t o_e1 = carve((size_t)m * sizeof(EdAffine)), o_om = carve((size_t)m * sizeof(Fp)), o_sk = carve(sizeof(Fp)), o_rv = carve((size_t)m * sizeof(EdAffine)),
                 o_ab = carve((size_t)m * 2 * sizeof(EdAffine)), o_pk = carve(sizeof(EdAffine)), o_c = carve((size_t)m * sizeof(Fp)),
                 o_proofs = carve((size_t)m * UZK_CP_PROOF_BYTES);
    UZK_TRY(c.ed_ws.reserve(at));
    char* ws = c.ed_ws.as<char>();
    EdAffine* d_e1 = reinterpret_cast<EdAffine*>(ws + o_e1);
    Fp* d_om = reinterpret_cast<Fp*>(ws + o_om);
    Fp* d_sk = reinterpret_cast<Fp*>(ws + o_sk);
    EdAffine* d_rv = reinterpret_cast<EdAffine*>(ws + o_rv);
    EdAffine* d_ab = reinterpret_cast<EdAffine*>(ws + o_ab);
    EdAffine* d_pk = reinterpret_cast<EdAffine*>(ws + o_pk);
    Fp* d_c = reinterpret_cast<Fp*>(ws + o_c);
    uint8_t* d_proofs = reinterpret_cast<uint8_t*>(ws + o_proofs);
    UZK_HIP(hipMemcpyAsync(d_e1, e1, (size_t)m * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_om, omegas, (size_t)m * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_sk, sk, sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    {
        KernelScope ks(c, "cp_prove_mul");
        hipLaunchKernelGGL(cp_prove_mul_kernel, dim3(ed_grid((size_t)m * 3 + 1)), dim3(kEdBlock), 0, c.stream, d_e1, d_sk, d_om, d_rv, d_ab, d_pk, m);
    }
    UZK_HIP(hipGetLastError());
    CpStatement s;
    s.e1 = d_e1; s.reveal = d_rv; s.pk = d_pk;
    s.s_e1 = s.s_reveal = 1; s.s_pk = 0;
    {
        KernelScope ks(c, "cp_transcript");
        hipLaunchKernelGGL(cp_transcript_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, s, nullptr, d_ab, d_c, d_om, d_sk, d_proofs, m);
    }
    UZK_HIP(hipGetLastError());
    UZK_HIP(hipMemcpyAsync(reveal_out, d_rv, (size_t)m * sizeof(EdAffine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(pk_out, d_pk, sizeof(EdAffine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(proofs_out, d_proofs, (size_t)m * UZK_CP_PROOF_BYTES, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// n records of EdRawIn (72 words) -> n records of EdRawOut (37 words), both on the host
int ed_raw_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (n == 0) return UZK_OK;
    static_assert(sizeof(EdRawIn) == 72 * sizeof(uint32_t) && sizeof(EdRawOut) == 37 * sizeof(uint32_t), "records are packed words");
    EdRawIn* din = nullptr;
    EdRawOut* dout = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&din), n * sizeof(EdRawIn));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), n * sizeof(EdRawOut));
    if (e == hipSuccess) e = hipMemcpyAsync(din, in, n * sizeof(EdRawIn), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ed_raw_kat_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, op, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(EdRawOut), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

}  // namespace uzk
