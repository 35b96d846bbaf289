// What the circuits built on a TurboCS (shufflecs.*, matchcs.*) share beyond their layout (cs_layout.hpp): the resident copy of a
// layout, the creation of an ordinary Circuit that carries it, the common columns of the tables and the gather of a witness
// (cs_kernels.hip), and the helpers their kernels are written with.  A circuit's module keeps what only it has: its kinds of
// variables, its extra columns, its witness.
#pragma once
#include <functional>
#include <memory>

#include "cs_layout.hpp"
#include "ctx.hpp"
#include "handles.hpp"
#include "prover.hpp"

#define API_LOCK std::lock_guard<std::mutex> _lk(ctx_mutex())        // as api.cpp and prover.cpp spell it: the same macro

namespace uzk {

// ---- the device side: every pointer a device address
constexpr uint32_t kCsBlock = 256;
inline uint32_t cs_grid(size_t items) { return (uint32_t)((items + kCsBlock - 1) / kCsBlock); }

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Fp cs_bit(bool on) { return on ? Fr::one() : Fr::zero(); }
// an integer of magnitude below 2^15 as an element of Fr
__device__ __forceinline__ Fp cs_small(int v) {
    Fp p = Fr::zero();
    p.v[0] = (uint32_t)(v < 0 ? -v : v);
    const Fp r = Fr::to_mont(p);
    return v < 0 ? Fr::neg(r) : r;
}
#endif

struct CsTableArgs {
    uint32_t n;
    const int16_t* sel;                // [9][n]
    const uint8_t* qb;                 // [n]
    const uint8_t* prk_row;            // [n]: 0, or 1 + the row of prk; null: no q_prk gates, the four columns are zero
    const uint32_t* perm;              // [5][n]
    const Fp* group;                   // [n]: omega^i
    const Fp* prk;                     // [rows][4], or null with prk_row
    Fp k[kCsWires];
    Fp* out;                           // [at least kCsCommonTables][n]
};
struct CsGatherArgs {
    uint32_t n, num_vars, pi_count;
    const uint32_t *wiring, *pi_vars;
    const Fp* values;                  // [batch][num_vars]
    Fp *witness, *pi;                  // [batch][5][n], [batch][pi_count]
};
// cs_tables: per row, 9 q (small signed integers into Fr), 5 s (one product k[w] omega^i each), qb, 4 q_prk: 19 stores of 32 B
int cs_tables_run(Ctx& c, const CsTableArgs& a);
// cs_gather: per (lane, wire, row), witness[w][row] = value[wiring[w][row]]; the pi_count items behind them: the public inputs
int cs_gather_run(Ctx& c, const CsGatherArgs& a, uint32_t batch);

// ---- the host side (cs_common.cpp)
struct CsResident {
    std::shared_ptr<DevBlock> blk;                                 // the device copies below and the module's own, carved out of one block
    const uint32_t *d_wiring = nullptr, *d_defs = nullptr, *d_pi_vars = nullptr;
    const int16_t* d_sel = nullptr;
    const uint8_t* d_qb = nullptr;
};

template <class T>
int cs_put(Ctx& c, T* dst, const std::vector<T>& src) {
    UZK_HIP(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c.stream));
    return UZK_OK;
}
// One block for the layout's common arrays and, behind them, the arrays `declare` adds to the carver; `fill` copies the module's
// arrays into the bound carver and keeps their addresses.  One synchronisation at the end.
int cs_make_resident(Ctx& c, const CsLayout& L, CsResident* r, const std::function<void(WsCarver&)>& declare,
                     const std::function<int(const WsCarver&)>& fill);
CsTableArgs cs_table_args(const Circuit& cir, const CsResident& r, const uint8_t* d_prk_row, const Fp* d_prk, Fp* d_out);

// what a module hung on a circuit under its tag, or null: the tag says whose ext is
template <class T>
std::shared_ptr<T> cs_ext(const std::shared_ptr<Circuit>& cir, uint32_t kind) {
    return cir && cir->ext_kind == kind ? std::static_pointer_cast<T>(cir->ext) : nullptr;
}
int cs_circuit_here(const Circuit& cir, const char* who);          // the context is ready, and on the circuit's device
void cs_info(const CsLayout& L, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out);

// the fields uzk_shuffle_circuit_desc and uzk_match_circuit_desc share
struct CsCircuitDesc {
    uint32_t precompute;
    const uzk_g1_affine *lagrange_bases, *blind_bases;
    const uint64_t (*k)[4];
    const uint64_t* group_gen;
};
template <class Desc>
CsCircuitDesc cs_desc_of(const Desc& d) { return {d.precompute, d.lagrange_bases, d.blind_bases, d.k, d.group_gen}; }
// An ordinary circuit over the layout's permutation with empty tables (l1 = the iFFT of (n, 0, ..): n ones); `fill` sets what the
// desc has for this kind of circuit alone (shuffle, edwards_a, anemoi_g).  Then, under the context lock, `install` makes the layout
// resident and installs the tables, and the circuit takes `ext` under the tag `kind`.  A failure releases the circuit.
int cs_circuit_create(const CsCircuitDesc& d, const CsLayout& L, const std::function<void(uzk_circuit_desc&)>& fill, uint32_t kind,
                      const std::shared_ptr<void>& ext, const std::function<int(Ctx&, Circuit&)>& install, uint64_t* circuit_out);
// The tables of a fresh circuit: a block of `tables` evaluation vectors in *evals, `run` over it (the table kernels), then the two
// refreshes every circuit does, UZK_CS_Q x 14 and UZK_CS_QB x 5 (slot 14, l1, and slot 20, coset_quotient, are the circuit's own);
// cm: their kCsCommonTables commitments in slot order.  The block stays with the caller for the refreshes only it does.
int cs_install_common(Ctx& c, Circuit& cir, uint32_t tables, const std::function<int(Fp*)>& run, std::shared_ptr<DevBlock>* evals, Jac* cm);
// the wiring and the permutation of a circuit, each optional, onto the host: queued on the stream, the caller synchronises
int cs_test_tables_common(Ctx& c, const Circuit& cir, const CsResident& r, uint32_t* wiring_out, uint32_t* perm_out);

}  // namespace uzk
