// The host side the circuits built on a TurboCS share (cs_common.hpp): a layout made resident, the ordinary Circuit that carries it,
// the tables every circuit installs.
#include "cs_common.hpp"

#include <cstring>

namespace uzk {

int cs_make_resident(Ctx& c, const CsLayout& L, CsResident* r, const std::function<void(WsCarver&)>& declare,
                     const std::function<int(const WsCarver&)>& fill) {
    WsCarver cv;
    const auto a_w = cv.array<uint32_t>(L.wiring.size()), a_d = cv.array<uint32_t>(L.defs.size()), a_p = cv.array<uint32_t>(L.pi_vars.size());
    const auto a_s = cv.array<int16_t>(L.sel.size());
    const auto a_q = cv.array<uint8_t>(L.qb.size());
    declare(cv);
    UZK_TRY(dev_block(cv.total(), &r->blk));
    cv.bind(r->blk->p);
    UZK_TRY(cs_put(c, cv(a_w), L.wiring)); UZK_TRY(cs_put(c, cv(a_d), L.defs)); UZK_TRY(cs_put(c, cv(a_p), L.pi_vars));
    UZK_TRY(cs_put(c, cv(a_s), L.sel)); UZK_TRY(cs_put(c, cv(a_q), L.qb));
    UZK_TRY(fill(cv));
    UZK_HIP(hipStreamSynchronize(c.stream));
    r->d_wiring = cv(a_w); r->d_defs = cv(a_d); r->d_pi_vars = cv(a_p); r->d_sel = cv(a_s); r->d_qb = cv(a_q);
    return UZK_OK;
}

CsTableArgs cs_table_args(const Circuit& cir, const CsResident& r, const uint8_t* d_prk_row, const Fp* d_prk, Fp* d_out) {
    CsTableArgs a = {};
    a.n = cir.n; a.sel = r.d_sel; a.qb = r.d_qb; a.prk_row = d_prk_row; a.perm = cir.d_perm; a.group = cir.d_group; a.prk = d_prk; a.out = d_out;
    for (uint32_t w = 0; w < kCsWires; ++w) a.k[w] = cir.k[w];
    return a;
}

int cs_circuit_here(const Circuit& cir, const char* who) {
    UZK_TRY(require_ready());
    if (ctx().device != cir.device) { set_error("%s: the circuit lives on device %d, the calling context on device %d", who, cir.device, ctx().device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

void cs_info(const CsLayout& L, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out) {
    if (size_out) *size_out = L.size;
    if (n_out) *n_out = L.n;
    if (num_vars_out) *num_vars_out = L.num_vars;
    if (pi_count_out) *pi_count_out = (uint32_t)L.pi_rows.size();
    if (pi_rows_out) std::memcpy(pi_rows_out, L.pi_rows.data(), L.pi_rows.size() * sizeof(uint32_t));
}

int cs_circuit_create(const CsCircuitDesc& d, const CsLayout& L, const std::function<void(uzk_circuit_desc&)>& fill, uint32_t kind,
                      const std::shared_ptr<void>& ext, const std::function<int(Ctx&, Circuit&)>& install, uint64_t* circuit_out) {
    const uint32_t n = L.n;
    uzk_circuit_desc cd = {};
    cd.n = n; cd.precompute = d.precompute;
    cd.lagrange_bases = d.lagrange_bases; cd.blind_bases = d.blind_bases;
    cd.permutation = L.perm.data();
    std::memcpy(cd.k, d.k, sizeof cd.k);
    std::memcpy(cd.group_gen, d.group_gen, sizeof cd.group_gen);
    fill(cd);
    const std::vector<Fp> l1(n, Fr::one());
    cd.polys[UZK_CS_L1] = reinterpret_cast<const uint64_t*>(l1.data());
    cd.poly_lens[UZK_CS_L1] = n;
    uint64_t h = 0;
    UZK_TRY(uzk_circuit_create(&cd, &h));                          // takes the context lock itself
    int rc;
    {
        API_LOCK;
        auto cir = find_circuit(h);
        rc = install(ctx(), *cir);
        if (rc == UZK_OK) { cir->ext = ext; cir->ext_kind = kind; }
    }
    if (rc != UZK_OK) { (void)uzk_circuit_release(h); return rc; }
    *circuit_out = h;
    return UZK_OK;
}

int cs_install_common(Ctx& c, Circuit& cir, uint32_t tables, const std::function<int(Fp*)>& run, std::shared_ptr<DevBlock>* evals, Jac* cm) {
    const uint32_t n = cir.n;
    UZK_TRY(dev_block((size_t)tables * n * sizeof(Fp), evals));
    Fp* d = static_cast<Fp*>((*evals)->p);
    UZK_TRY(run(d));
    UZK_TRY(circuit_refresh_device(c, cir, UZK_CS_Q, 14, d, cm));
    return circuit_refresh_device(c, cir, UZK_CS_QB, 5, d + (size_t)kCsTabQb * n, cm + kCsTabQb);
}

int cs_test_tables_common(Ctx& c, const Circuit& cir, const CsResident& r, uint32_t* wiring_out, uint32_t* perm_out) {
    const size_t words = (size_t)kCsWires * cir.n * sizeof(uint32_t);
    if (wiring_out) UZK_HIP(hipMemcpyAsync(wiring_out, r.d_wiring, words, hipMemcpyDeviceToHost, c.stream));
    if (perm_out) UZK_HIP(hipMemcpyAsync(perm_out, cir.d_perm, words, hipMemcpyDeviceToHost, c.stream));
    return UZK_OK;
}

}  // namespace uzk
