// zshuffle's circuit on the device (include/uzkge_gpu.h, "the shuffle circuit"): the evaluation vectors of its tables and the
// witnesses of `batch` decks, from the compact layout of shufflecs.hpp.  One work item per row, per (row, wire) or per variable;
// every launch moves 32-byte elements and does next to no arithmetic, so each is bound by its stores (the loads are gathers out of
// arrays that fit the L2: a layout is under 2 MB, a lane's variable values under 1.5 MB):
//   cs_tables      per row: 9 q, 5 s (one product k[w] omega^i each), qb, 4 zero q_prk (cs_kernels.hip)     19 stores of 32 B, coalesced per column
//   shcs_key       per row: the 12 columns of one table (T_G or T_pk) at the rows of the remark blocks, and q_ecc where asked  12 or 13 stores
//   shcs_values    per (lane, variable): the variable's definition in Fr -- a load, a 0/1, a sum of at most 64 terms, or at most 32
//                  products a c + b d.  The longest items (sums of products) are 4 N ceil(N/6) of ~ 30 000 threads
//   cs_gather      per (lane, wire, row): extended[w][row] = value[wiring[w][row]]; the 8 N items behind them: the public inputs
//   shcs_wsel      per (lane, row): the three wire selectors from the card's digit
#include "shufflecs_dev.hpp"

namespace uzk {

// out[4 part + e][row] = table[j][e][part] on row j of a remark block (part: x, y, d x y), zero elsewhere; ecc (or null): q_ecc, one
// on the rows of the remark blocks
__global__ __launch_bounds__(kCsBlock) void shcs_key_kernel(const uint16_t* __restrict__ block, const Fp* __restrict__ table, Fp* __restrict__ out,
                                                            Fp* __restrict__ ecc, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t row = blockIdx.x * kCsBlock + threadIdx.x;
    if (row >= n) return;
    const uint32_t b = block[row];
    const Fp* t = table + (size_t)((b ? b - 1 : 0) % kShcsIters) * 12;
    for (uint32_t part = 0; part < 3; ++part)
        for (uint32_t e = 0; e < 4; ++e) out[(size_t)(4 * part + e) * n + row] = b ? t[e * 3 + part] : Fr::zero();
    if (ecc) ecc[row] = cs_bit(b != 0);
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
// the remasked card k's coordinate c: entry 83 of its trace
__device__ __forceinline__ const Fp& shcs_remarked(const Fp* trace, uint32_t k, uint32_t c) {
    return trace[((size_t)k * kShcsIters + kShcsIters - 1) * 4 + c];
}
__device__ __forceinline__ Fp shcs_product(const uint32_t* perm, const Fp* trace, uint32_t N, uint32_t i, uint32_t c, uint32_t t) {
    const uint32_t j = 2 * t;
    Fp r = Fr::mul(cs_bit(perm[i] == j), shcs_remarked(trace, j, c));
    if (j + 1 < N) r = Fr::add(r, Fr::mul(cs_bit(perm[i] == j + 1), shcs_remarked(trace, j + 1, c)));
    return r;
}
#endif

__global__ __launch_bounds__(kCsBlock) void shcs_values_kernel(ShcsWitnessArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t v = blockIdx.x * kCsBlock + threadIdx.x, lane = blockIdx.y, N = a.cards;
    if (v >= a.num_vars) return;
    const uint32_t d = a.defs[v], kind = cs_def_kind(d), x = cs_def_a(d), y = cs_def_b(d), z = cs_def_c(d);
    const uint32_t* perm = a.perm + (size_t)lane * N;
    const Fp* trace = a.trace + (size_t)lane * N * kShcsIters * 4;
    Fp r = Fr::zero();
    switch (kind) {
    case kShcsConst: r = cs_bit(x != 0); break;
    case kShcsInput: r = (y < 2 ? a.e1 : a.e2)[((size_t)lane * N + x) * 2 + (y & 1)]; break;
    case kShcsTrace: r = trace[((size_t)x * kShcsIters + y) * 4 + z]; break;
    case kShcsMatrix: r = cs_bit(perm[x] == y); break;
    case kShcsRowSum:
        for (uint32_t j = 0; j < z; ++j) r = Fr::add(r, cs_bit(perm[x] == j));
        break;
    case kShcsColSum:
        for (uint32_t i = 0; i < z; ++i) r = Fr::add(r, cs_bit(perm[i] == x));
        break;
    case kShcsProduct: r = shcs_product(perm, trace, N, x, y, z); break;
    default:
        for (uint32_t t = 0; t < z; ++t) r = Fr::add(r, shcs_product(perm, trace, N, x, y, t));
        break;
    }
    a.values[(size_t)lane * a.num_vars + v] = r;
#endif
}

// compute_witness_selectors over trace.bits = (bit 0, bit 1, +-1 by bit 2)
__global__ __launch_bounds__(kCsBlock) void shcs_wsel_kernel(ShcsWitnessArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = blockIdx.x * kCsBlock + threadIdx.x, lane = blockIdx.y, n = a.n;
    if (t >= n) return;
    const uint32_t b = a.block[t];
    const uint32_t d = b ? a.digits[(size_t)lane * a.cards * kShcsIters + (b - 1)] : 0;
    Fp* out = a.wsel + (size_t)lane * 3 * n + t;
    out[0] = cs_bit(b && (d & 1));
    out[n] = cs_bit(b && (d & 2));
    out[2 * (size_t)n] = !b ? Fr::zero() : (d & 4) ? Fr::one() : Fr::neg(Fr::one());
#endif
}

int shcs_tables_run(Ctx& c, const CsTableArgs& a, const uint16_t* d_block, const Fp* d_gen, const Fp* d_pk) {
    const dim3 grid(cs_grid(a.n)), block(kCsBlock);
    UZK_TRY(cs_tables_run(c, a));
    UZK_LAUNCH(c, "shcs_key", shcs_key_kernel, grid, block, 0, c.stream, d_block, d_pk, a.out + (size_t)kShcsTabPk * a.n, (Fp*)nullptr, a.n);
    UZK_LAUNCH(c, "shcs_key", shcs_key_kernel, grid, block, 0, c.stream, d_block, d_gen, a.out + (size_t)kShcsTabGen * a.n, a.out + (size_t)kShcsTabEcc * a.n, a.n);
    return UZK_OK;
}

int shcs_key_run(Ctx& c, const uint16_t* d_block, const Fp* d_table, Fp* d_out, uint32_t n) {
    UZK_LAUNCH(c, "shcs_key", shcs_key_kernel, dim3(cs_grid(n)), dim3(kCsBlock), 0, c.stream, d_block, d_table, d_out, (Fp*)nullptr, n);
    return UZK_OK;
}

int shcs_witness_run(Ctx& c, const ShcsWitnessArgs& a, uint32_t batch) {
    const dim3 block(kCsBlock);
    UZK_LAUNCH(c, "shcs_values", shcs_values_kernel, dim3(cs_grid(a.num_vars), batch), block, 0, c.stream, a);
    UZK_TRY(cs_gather_run(c, {a.n, a.num_vars, a.pi_count, a.wiring, a.pi_vars, a.values, a.witness, a.pi}, batch));
    UZK_LAUNCH(c, "shcs_wsel", shcs_wsel_kernel, dim3(cs_grid(a.n), batch), block, 0, c.stream, a);
    return UZK_OK;
}

}  // namespace uzk
