// The two kernels every circuit built on a TurboCS runs unchanged (cs_common.hpp): the common columns of its tables and the gather of
// a batch of witnesses.  One work item per row or per (row, wire); both move 32-byte elements and do next to no arithmetic, so each
// is bound by its stores (the loads are gathers out of arrays that fit the L2).
#include "cs_common.hpp"

namespace uzk {

__global__ __launch_bounds__(kCsBlock) void cs_tables_kernel(CsTableArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t row = blockIdx.x * kCsBlock + threadIdx.x, n = a.n;
    if (row >= n) return;
    for (uint32_t i = 0; i < kCsSelectors; ++i) {
        const int v = a.sel[(size_t)i * n + row];
        a.out[(size_t)i * n + row] = v == 0 ? Fr::zero() : cs_small(v);
    }
    for (uint32_t w = 0; w < kCsWires; ++w) {                      // encode_perm_to_group: k[perm / n] group[perm mod n]
        const uint32_t p = a.perm[(size_t)w * n + row];
        a.out[(size_t)(kCsTabS + w) * n + row] = Fr::mul(a.k[p / n], a.group[p % n]);
    }
    a.out[(size_t)kCsTabQb * n + row] = cs_bit(a.qb[row] != 0);
    const uint32_t r = a.prk_row ? a.prk_row[row] : 0;             // 0, or 1 + the row of prk
    for (uint32_t i = 0; i < 4; ++i) a.out[(size_t)(kCsTabPrk + i) * n + row] = r ? a.prk[(r - 1) * 4 + i] : Fr::zero();
#endif
}

__global__ __launch_bounds__(kCsBlock) void cs_gather_kernel(CsGatherArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t p = blockIdx.x * kCsBlock + threadIdx.x, lane = blockIdx.y, total = kCsWires * a.n;
    const Fp* values = a.values + (size_t)lane * a.num_vars;
    if (p < total) a.witness[(size_t)lane * total + p] = values[a.wiring[p]];
    else if (p - total < a.pi_count) a.pi[(size_t)lane * a.pi_count + (p - total)] = values[a.pi_vars[p - total]];
#endif
}

int cs_tables_run(Ctx& c, const CsTableArgs& a) {
    UZK_LAUNCH(c, "cs_tables", cs_tables_kernel, dim3(cs_grid(a.n)), dim3(kCsBlock), 0, c.stream, a);
    return UZK_OK;
}

int cs_gather_run(Ctx& c, const CsGatherArgs& a, uint32_t batch) {
    UZK_LAUNCH(c, "cs_gather", cs_gather_kernel, dim3(cs_grid((size_t)kCsWires * a.n + a.pi_count), batch), dim3(kCsBlock), 0, c.stream, a);
    return UZK_OK;
}

}  // namespace uzk
