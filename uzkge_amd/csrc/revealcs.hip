// The reveal circuit behind the C ABI (include/uzkge_gpu.h, "the reveal circuit"): the layout of revealcs_layout.cpp joined to the
// points of a Groth16 proving key as a resident key (groth16.hip), and the full assignments of a batch of cards under one secret.
//
// Every witness is an affine coordinate of a point of one of the two double-and-add chains, or a product of two.  Walked in affine
// form a card would pay about a thousand field inversions; instead
//   rcs_walk    one lane per chain.  Workgroup 0 holds the ONE lane of the fixed-base chain (sk is the call's, so g.scalar_mul_le(sk)
//               is the same for every card): tmp_i = res_i + 2^i G over the table of constants, 256 unified additions.  The
//               workgroups behind it hold one lane per card: tmp_i = res_i + 2^i e1 and the doubling, 512 unified additions in
//               extended coordinates (ed29.hpp: complete, so sk = 0 and points of small order take no other path).  The bits of sk
//               are the same in every lane: the select is wave-uniform.  Every step's (X, Y, Z) and the prefix product of the Z so
//               far go to the lane's column of a workspace ws[step][slot][limb][lane]; ONE inversion per lane and a walk back
//               along the chain (Montgomery's trick, as remark_kernel) give every point in affine form
//   rcs_fill    one lane per (card, chain, iteration), a workgroup of 256 per (card, chain): the 5, 10 or 13 values of the iteration
//               from the affine points (res_i is tmp_j of the highest set bit j < i of sk, or the neutral point) on canonical
//               Montgomery words, written at the offsets of revealcs.hpp; lane 0 of the fixed chain also writes the one, the
//               statement and the six squares, and each of its lanes one bit
// A call is the latency of 512 dependent additions and the walk back, whatever the batch.  tests/reveal_cs_ref.py is the restatement.
#include <cstring>

#include "ctx.hpp"
#include "cs_common.hpp"
#include "ed29.hpp"
#include "handles.hpp"
#include "revealcs.hpp"

namespace uzk {

constexpr uint32_t kRcsFixedSteps = kRcsBits, kRcsVarSteps = 2 * kRcsBits, kRcsWsWords = 36;
constexpr uint32_t kRcsAffPerCard = 2 * kRcsBits + 1;              // tmp_0 .. tmp_255, then 2^0 e1 .. 2^256 e1
constexpr uint32_t kRcsWalkBlock = 64, kRcsFillBlock = 256;
static_assert(kRcsFillBlock == kRcsBits, "rcs_fill: one lane per iteration");

struct RcsArgs {
    const EdAffine* table;             // [257]: 2^i G, then the neutral point
    const Fp* sk;                      // one 256-bit integer, plain words
    const EdAffine* e1;                // [m]
    uint32_t *ws_fixed, *ws_var;       // [256][36][1], [512][36][m]
    EdAffine *aff_fixed, *aff_var;     // [256], [m][kRcsAffPerCard]
    Fp* z;                             // [m][kRcsVars]
    uint32_t m;
};

#if defined(__HIP_DEVICE_COMPILE__)
// sk is read where it lies (eight words of global memory, the same for every lane): an index that varies would put a copy into scratch
__device__ __forceinline__ uint32_t rcs_bit(const Fp* k, uint32_t i) { return (k->v[i >> 5] >> (i & 31)) & 1; }

// step `step` of lane t of `lanes`: X, Y, Z and the prefix product
__device__ __forceinline__ void rcs_record(uint32_t* ws, uint32_t step, uint32_t lanes, uint32_t t, const ed::P& p, const ed::C& pre) {
    uint32_t* w = ws + (size_t)step * kRcsWsWords * lanes + t;
#pragma unroll
    for (int l = 0; l < 9; ++l) {
        w[(size_t)l * lanes] = p.x.v.l[l];
        w[(size_t)(9 + l) * lanes] = p.y.v.l[l];
        w[(size_t)(18 + l) * lanes] = p.z.v.l[l];
        w[(size_t)(27 + l) * lanes] = pre.v.l[l];
    }
}

// the walk back: put(step, point) for steps - 1 .. 0 from the inverse of the last prefix product
template <class Put>
__device__ __forceinline__ void rcs_unwind(const uint32_t* ws, uint32_t steps, uint32_t lanes, uint32_t t, const ed::C& pre, Put put) {
    ed::C inv = ed::inv(pre);
#pragma unroll 1
    for (int i = (int)steps - 1; i >= 0; --i) {
        const uint32_t* w = ws + (size_t)i * kRcsWsWords * lanes + t;
        ed::C x, y, z, before = ed::one();
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            x.v.l[l] = w[(size_t)l * lanes];
            y.v.l[l] = w[(size_t)(9 + l) * lanes];
            z.v.l[l] = w[(size_t)(18 + l) * lanes];
            if (i > 0) before.v.l[l] = (w - (size_t)kRcsWsWords * lanes)[(size_t)(27 + l) * lanes];
        }
        const ed::C zi = ed::Z::mul(inv, before);                  // 1 / Z_i
        inv = ed::Z::mul(inv, z);                                  // 1 / (Z_0 ... Z_{i-1})
        EdAffine r;
        r.x = ed::Z::to_wire(ed::Z::mul(x, zi)); r.y = ed::Z::to_wire(ed::Z::mul(y, zi));
        put((uint32_t)i, r);
    }
}

// the highest set bit of k below bit i (0 <= i <= 256), or -1
__device__ __forceinline__ int rcs_top_bit_below(const Fp* k, uint32_t i) {
    for (int w = 7; w >= 0; --w) {
        const uint32_t lo = 32u * (uint32_t)w;
        if (i <= lo) continue;
        uint32_t v = k->v[w];
        if (i - lo < 32) v &= (1u << (i - lo)) - 1;
        if (v) return (int)(lo + 31 - (uint32_t)__clz(v));
    }
    return -1;
}
// res before iteration i of a chain whose tmp_j lie at tmp[j]: a load through one of two pointers (a select between two points in
// registers goes through scratch); neutral: the point (0, 1) behind the table's multiples
__device__ __forceinline__ EdAffine rcs_res(const EdAffine* tmp, const EdAffine* neutral, const Fp* sk, uint32_t i) {
    const int j = rcs_top_bit_below(sk, i);
    return *(j < 0 ? neutral : tmp + j);
}
#endif

__global__ __launch_bounds__(kRcsWalkBlock) void rcs_walk_kernel(RcsArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const Fp* sk = a.sk;
    ed::P acc = ed::identity();
    ed::C pre = ed::one();
    if (blockIdx.x == 0) {                                         // the fixed-base chain: one lane
        if (threadIdx.x != 0) return;
#pragma unroll 1
        for (uint32_t i = 0; i < kRcsBits; ++i) {
            const ed::P tmp = ed::add(acc, ed::from_affine(a.table[i]));
            pre = ed::Z::mul(pre, tmp.z);
            rcs_record(a.ws_fixed, i, 1, 0, tmp, pre);
            if (rcs_bit(sk, i)) acc = tmp;
        }
        EdAffine* out = a.aff_fixed;
        rcs_unwind(a.ws_fixed, kRcsFixedSteps, 1, 0, pre, [&](uint32_t step, const EdAffine& p) { out[step] = p; });
        return;
    }
    const uint32_t t = (blockIdx.x - 1) * kRcsWalkBlock + threadIdx.x;
    if (t >= a.m) return;
    const EdAffine base = a.e1[t];
    EdAffine* out = a.aff_var + (size_t)t * kRcsAffPerCard;
    out[kRcsBits] = base;                                          // 2^0 e1
    ed::P mult = ed::from_affine(base);
#pragma unroll 1
    for (uint32_t i = 0; i < kRcsBits; ++i) {
        const ed::P tmp = ed::add(acc, mult);
        pre = ed::Z::mul(pre, tmp.z);
        rcs_record(a.ws_var, 2 * i, a.m, t, tmp, pre);
        if (rcs_bit(sk, i)) acc = tmp;
        mult = ed::add(mult, mult);
        pre = ed::Z::mul(pre, mult.z);
        rcs_record(a.ws_var, 2 * i + 1, a.m, t, mult, pre);
    }
    // step 2 i: tmp_i; step 2 i + 1: 2^(i+1) e1
    rcs_unwind(a.ws_var, kRcsVarSteps, a.m, t, pre, [&](uint32_t step, const EdAffine& p) { out[(step & 1) ? kRcsBits + (step + 1) / 2 : step / 2] = p; });
#endif
}

// workgroup 2 card + chain, lane = iteration
__global__ __launch_bounds__(kRcsFillBlock) void rcs_fill_kernel(RcsArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t card = blockIdx.x >> 1, chain = blockIdx.x & 1, it = threadIdx.x;
    if (card >= a.m) return;
    const Fp* sk = a.sk;
    const uint32_t bit = rcs_bit(sk, it);
    Fp* z = a.z + (size_t)card * kRcsVars;
    const EdAffine* tmp_v = a.aff_var + (size_t)card * kRcsAffPerCard;
    const EdAffine* mult_v = tmp_v + kRcsBits;
    const EdAffine* neutral = a.table + kRcsBits;
    if (chain == 0) {
        Fp b;
#pragma unroll
        for (int k = 0; k < 8; ++k) b.v[k] = FrCfg::R1[k] & (0u - bit);
        z[kRcsOffBits + it] = b;
        if (it == 0) {
            const EdAffine h = a.e1[card], reveal = rcs_res(tmp_v, neutral, sk, kRcsBits), pk = rcs_res(a.aff_fixed, neutral, sk, kRcsBits);
            z[0] = Fr::one();
            z[1] = h.x; z[2] = h.y; z[3] = reveal.x; z[4] = reveal.y; z[5] = pk.x; z[6] = pk.y;
            Fp* o = z + kRcsOffPoints;
            o[0] = Fr::sqr(h.x); o[1] = Fr::sqr(h.y); o[2] = Fr::sqr(reveal.x); o[3] = Fr::sqr(reveal.y); o[4] = Fr::sqr(pk.x); o[5] = Fr::sqr(pk.y);
            return;                                                // iteration 0 of the fixed chain is linear in the bit
        }
        const EdAffine res = rcs_res(a.aff_fixed, neutral, sk, it), mult = a.table[it], tmp = a.aff_fixed[it];
        const EdAffine sel = rcs_res(a.aff_fixed, neutral, sk, it + 1);       // bit ? tmp : res
        Fp* o = z + kRcsOffFixed + kRcsFixedPer * (it - 1);
        o[0] = Fr::mul(Fr::mul(mult.y, res.x), Fr::mul(mult.x, res.y));
        o[1] = tmp.x; o[2] = tmp.y; o[3] = sel.x; o[4] = sel.y;
        return;
    }
    const EdAffine res = rcs_res(tmp_v, neutral, sk, it), mult = mult_v[it], tmp = tmp_v[it], dbl = mult_v[it + 1];
    const EdAffine sel = rcs_res(tmp_v, neutral, sk, it + 1);                  // bit ? tmp : res
    const Fp v0 = Fr::mul(mult.y, res.x), v1 = Fr::mul(mult.x, res.y);
    Fp* o = z + (it == 0 ? kRcsOffVar : kRcsOffVar1 + kRcsVarPer * (it - 1));
    if (it > 0) {                                                  // iteration 0 adds to the constant neutral point: u, v0, v1 are linear
        o[0] = Fr::mul(Fr::sub(res.y, res.x), Fr::add(mult.x, mult.y));
        o[1] = v0; o[2] = v1;
        o += 3;
    }
    o[0] = Fr::mul(v0, v1);
    o[1] = tmp.x; o[2] = tmp.y; o[3] = sel.x; o[4] = sel.y;
    o[5] = Fr::mul(mult.x, mult.y); o[6] = Fr::sqr(mult.x); o[7] = Fr::sqr(mult.y);
    o[8] = dbl.x; o[9] = dbl.y;
#endif
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

struct RcsEntry {
    int device = 0;
    uint64_t key = 0;                  // the resident Groth16 key
    EdAffine* d_table = nullptr;
};
HandleTable<RcsEntry> g_rcs(3ull << 58);

const RevealLayout* rcs_layout() {
    static const RevealLayout* L = [] {
        RevealLayout* l = new RevealLayout();
        if (!reveal_layout_build(l)) { delete l; l = nullptr; }
        return l;
    }();
    return L;
}

void rcs_free(const RcsEntry& e) {
    DeviceGuard on(e.device);
    if (e.d_table) (void)hipFree(e.d_table);
    if (e.key) (void)g16_key_release(e.key);
}

bool rcs_on_curve(const EdAffine& p) {
    const Fp xx = Fr::sqr(p.x), yy = Fr::sqr(p.y);
    return Fr::eq(Fr::add(xx, yy), Fr::add(Fr::one(), Fr::mul(Fr::mul(xx, yy), ed_d_wire())));
}

int rcs_lookup(const char* who, uint64_t circuit, RcsEntry* e) {
    if (!g_rcs.get(circuit, e)) { set_error("%s: %llu is no circuit of uzk_reveal_circuit_create", who, (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

// everything of a witness call that needs no device
int rcs_check_inputs(const char* who, const uint64_t* sk, const uint64_t* e1_mont, uint32_t m) {
    if (m == 0 || m > UZK_REVEAL_CS_MAX_BATCH) { set_error("%s: %u cards (1 .. %d per call)", who, m, UZK_REVEAL_CS_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!sk || !e1_mont) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    const Fp* w = reinterpret_cast<const Fp*>(e1_mont);
    const size_t bad = ed_first_noncanonical(w, 2 * (size_t)m);
    if (bad < 2 * (size_t)m) { set_error("%s: e1[%zu]: the %c coordinate is not below q", who, bad / 2, bad % 2 ? 'y' : 'x'); return UZK_ERR_PARAMETER; }
    const EdAffine* pts = reinterpret_cast<const EdAffine*>(e1_mont);
    for (uint32_t i = 0; i < m; ++i)
        if (!rcs_on_curve(pts[i])) { set_error("%s: e1[%u] is not on the curve", who, i); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

// the assignments of m cards at d_z (device), the statements to the host; the stream is left running
int rcs_witness_launch(Ctx& c, const RcsEntry& e, const uint64_t* sk, const uint64_t* e1_mont, uint32_t m, Fp* d_z, uint64_t* statements_out) {
    WsCarver cv;
    const auto a_sk = cv.array<Fp>(1);
    const auto a_e1 = cv.array<EdAffine>(m);
    const auto a_wf = cv.array<uint32_t>((size_t)kRcsFixedSteps * kRcsWsWords), a_wv = cv.array<uint32_t>((size_t)kRcsVarSteps * kRcsWsWords * m);
    const auto a_af = cv.array<EdAffine>(kRcsBits), a_av = cv.array<EdAffine>((size_t)kRcsAffPerCard * m);
    UZK_TRY(cv.reserve(c.reveal_ws));
    UZK_HIP(hipMemcpyAsync(cv(a_sk), sk, sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_e1), e1_mont, a_e1.bytes(), hipMemcpyHostToDevice, c.stream));
    RcsArgs a = {};
    a.table = e.d_table; a.sk = cv(a_sk); a.e1 = cv(a_e1);
    a.ws_fixed = cv(a_wf); a.ws_var = cv(a_wv); a.aff_fixed = cv(a_af); a.aff_var = cv(a_av);
    a.z = d_z; a.m = m;
    UZK_LAUNCH(c, "rcs_walk", rcs_walk_kernel, dim3(1 + (m + kRcsWalkBlock - 1) / kRcsWalkBlock), dim3(kRcsWalkBlock), 0, c.stream, a);
    UZK_LAUNCH(c, "rcs_fill", rcs_fill_kernel, dim3(2 * m), dim3(kRcsFillBlock), 0, c.stream, a);
    // the statement of a card: variables 1 .. 6 of its assignment
    UZK_HIP(hipMemcpy2DAsync(statements_out, 6 * sizeof(Fp), d_z + 1, (size_t)kRcsVars * sizeof(Fp), 6 * sizeof(Fp), m, hipMemcpyDeviceToHost, c.stream));
    return UZK_OK;
}

int rcs_for_ctx(const char* who, const RcsEntry& e) {
    UZK_TRY(require_ready());
    if (e.device != ctx().device) { set_error("%s: the circuit lives on device %d, the calling context on device %d", who, e.device, ctx().device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

}  // namespace

int rcs_info(uint32_t* n_vars, uint32_t* n_inputs, uint32_t* n_constraints, uint64_t* domain, uint64_t nnz_out[3]) {
    const RevealLayout* L = rcs_layout();
    if (!L) { set_error("uzk_reveal_cs_info: the layout builder did not reach the circuit's counts"); return UZK_ERR_PARAMETER; }
    if (n_vars) *n_vars = L->n_vars;
    if (n_inputs) *n_inputs = L->n_inputs;
    if (n_constraints) *n_constraints = L->n_constraints;
    if (domain) *domain = L->domain;
    if (nnz_out)
        for (int k = 0; k < 3; ++k) nnz_out[k] = L->mat[k].col.size();
    return UZK_OK;
}

int rcs_matrices(uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]) {
    const RevealLayout* L = rcs_layout();
    if (!L) { set_error("uzk_reveal_cs_matrices: the layout builder did not reach the circuit's counts"); return UZK_ERR_PARAMETER; }
    if (!row_ptr || !col || !val) { set_error("uzk_reveal_cs_matrices: null pointer"); return UZK_ERR_PARAMETER; }
    for (int k = 0; k < 3; ++k)
        if (!row_ptr[k] || !col[k] || !val[k]) { set_error("uzk_reveal_cs_matrices: null buffer of matrix %d", k); return UZK_ERR_PARAMETER; }
    for (int k = 0; k < 3; ++k) {
        const RcsMatrix& m = L->mat[k];
        std::memcpy(row_ptr[k], m.row_ptr.data(), m.row_ptr.size() * sizeof(uint64_t));
        std::memcpy(col[k], m.col.data(), m.col.size() * sizeof(uint32_t));
        std::memcpy(val[k], m.val.data(), m.val.size() * sizeof(Fp));
    }
    return UZK_OK;
}

int rcs_circuit_create(const uzk_g16_key_desc* desc, uint64_t* circuit_out) {
    static const char* who = "uzk_reveal_circuit_create";
    if (!desc || !circuit_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    const RevealLayout* L = rcs_layout();
    if (!L) { set_error("%s: the layout builder did not reach the circuit's counts", who); return UZK_ERR_PARAMETER; }
    if (desc->n_vars != L->n_vars || desc->n_inputs != L->n_inputs) {
        set_error("%s: a key of %u variables and %u inputs, the circuit has %u and %u", who, desc->n_vars, desc->n_inputs, L->n_vars, L->n_inputs);
        return UZK_ERR_PARAMETER;
    }
    if (desc->n_constraints != 0 && desc->n_constraints != L->n_constraints) { set_error("%s: %u constraints, the circuit has %u (or 0: the circuit's)", who, desc->n_constraints, L->n_constraints); return UZK_ERR_PARAMETER; }
    if (desc->l_query_len != L->n_vars - L->n_inputs || desc->h_query_len != L->domain - 1) {
        set_error("%s: l_query of %llu and h_query of %llu points, the circuit needs %u and %llu", who, (unsigned long long)desc->l_query_len,
                  (unsigned long long)desc->h_query_len, L->n_vars - L->n_inputs, (unsigned long long)(L->domain - 1));
        return UZK_ERR_PARAMETER;
    }
    for (int k = 0; k < 3; ++k)
        if (desc->row_ptr[k] || desc->col[k] || desc->val[k]) { set_error("%s: the matrices are the circuit's own: matrix %d's pointers must be null", who, k); return UZK_ERR_PARAMETER; }
    uzk_g16_key_desc d = *desc;
    d.n_constraints = L->n_constraints;
    for (int k = 0; k < 3; ++k) {
        d.row_ptr[k] = L->mat[k].row_ptr.data();
        d.col[k] = L->mat[k].col.data();
        d.val[k] = reinterpret_cast<const uint64_t*>(L->mat[k].val.data());
    }
    uint64_t domain = 0;
    UZK_TRY(g16_key_check(&d, &domain));                           // host-only: before the device is touched
    API_LOCK;
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    RcsEntry e;
    e.device = c.device;
    UZK_TRY(g16_key_create(c, &d, &e.key));
    static_assert(sizeof(EdAffine) == 2 * sizeof(Fp), "a point is x then y");
    std::vector<Fp> table(L->multiples);                           // 2^i G, then the neutral point (0, 1)
    table.push_back(Fr::zero()); table.push_back(Fr::one());
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&e.d_table), table.size() * sizeof(Fp));
    if (err == hipSuccess) err = hipMemcpyAsync(e.d_table, table.data(), table.size() * sizeof(Fp), hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c.stream);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        rcs_free(e);
        set_error("%s: %s", who, hipGetErrorString(err));
        return UZK_ERR_DEVICE;
    }
    *circuit_out = g_rcs.insert(e);
    return UZK_OK;
}

// The caller makes sure no context still works with this circuit.
int rcs_circuit_release(uint64_t circuit) {
    API_LOCK;
    RcsEntry e;
    if (!g_rcs.take(circuit, &e)) { set_error("uzk_reveal_circuit_release: %llu is no circuit of uzk_reveal_circuit_create", (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    Ctx& c = ctx();
    if (c.ready) (void)hipStreamSynchronize(c.stream);
    rcs_free(e);
    return UZK_OK;
}

void rcs_release_all() { g_rcs.drain(rcs_free); }

int rcs_circuit_key(uint64_t circuit, uint64_t* key_out) {
    RcsEntry e;
    UZK_TRY(rcs_lookup("uzk_reveal_circuit_key", circuit, &e));
    if (!key_out) { set_error("uzk_reveal_circuit_key: null pointer"); return UZK_ERR_PARAMETER; }
    *key_out = e.key;
    return UZK_OK;
}

int rcs_witness_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, uint32_t m, void* d_z, uint64_t* statements_out) {
    static const char* who = "uzk_reveal_witness_batch";
    API_LOCK;
    RcsEntry e;
    UZK_TRY(rcs_lookup(who, circuit, &e));
    UZK_TRY(rcs_check_inputs(who, sk, e1_mont, m));
    if (!d_z || !statements_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(rcs_for_ctx(who, e));
    Ctx& c = ctx();
    UZK_TRY(rcs_witness_launch(c, e, sk, e1_mont, m, static_cast<Fp*>(d_z), statements_out));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int rcs_prove_snark_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                          uint64_t* statements_out, uzk_g16_proof* proofs_out) {
    static const char* who = "uzk_reveal_prove_snark_batch";
    API_LOCK;
    RcsEntry e;
    UZK_TRY(rcs_lookup(who, circuit, &e));
    UZK_TRY(rcs_check_inputs(who, sk, e1_mont, m));
    if (!r_mont || !s_mont || !statements_out || !proofs_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(rcs_for_ctx(who, e));
    Ctx& c = ctx();
    UZK_TRY(c.reveal_z.reserve((size_t)m * kRcsVars * sizeof(Fp)));
    UZK_TRY(rcs_witness_launch(c, e, sk, e1_mont, m, c.reveal_z.as<Fp>(), statements_out));
    // the prover reads the assignments where they lie, in stream order behind the kernels that wrote them
    return g16_prove_run(c, e.key, c.reveal_z.as<Fp>(), true, reinterpret_cast<const Fp*>(r_mont), reinterpret_cast<const Fp*>(s_mont), m, proofs_out);
}

int rcs_prove_snark_batch_finish(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                                 uint64_t* statements_out, uzk_g16_proof* proofs_out, uint8_t* blobs_out, void* d_blobs_out) {
    static const char* who = "uzk_reveal_prove_snark_batch_finish";
    API_LOCK;
    RcsEntry e;
    UZK_TRY(rcs_lookup(who, circuit, &e));
    UZK_TRY(rcs_check_inputs(who, sk, e1_mont, m));
    if (!r_mont || !s_mont || !statements_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    if (!proofs_out && !blobs_out && !d_blobs_out) { set_error("%s: no output asked for", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(rcs_for_ctx(who, e));
    Ctx& c = ctx();
    UZK_TRY(c.reveal_z.reserve((size_t)m * kRcsVars * sizeof(Fp)));
    UZK_TRY(rcs_witness_launch(c, e, sk, e1_mont, m, c.reveal_z.as<Fp>(), statements_out));
    return g16_prove_finish_run(c, e.key, c.reveal_z.as<Fp>(), true, reinterpret_cast<const Fp*>(r_mont), reinterpret_cast<const Fp*>(s_mont), m, proofs_out, blobs_out,
                                static_cast<uint8_t*>(d_blobs_out));
}

}  // namespace uzk
