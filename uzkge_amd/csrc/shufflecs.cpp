// The shuffle circuit behind the C ABI (include/uzkge_gpu.h, "the shuffle circuit"): the layout of shufflecs_layout.cpp made resident,
// its tables through the circuit's refresh path, and the witnesses of a batch of decks from a remask that never leaves the device.
// A circuit made here is an ordinary Circuit (prover.hpp) that carries its layout in `ext`; the layout goes with the circuit's last
// reference.
#include <cstring>

#include "host_math.hpp"
#include "shufflecs_dev.hpp"

using namespace uzk;

namespace {

struct ShuffleCs : CsResident {
    ShuffleLayout host;
    const uint16_t* d_block = nullptr;
};

std::shared_ptr<ShuffleCs> shuffle_of(const std::shared_ptr<Circuit>& cir) { return cs_ext<ShuffleCs>(cir, kExtShuffle); }

int make_resident(Ctx& c, ShuffleCs& s) {
    const ShuffleLayout& L = s.host;
    WsArray<uint16_t> a_b;
    return cs_make_resident(c, L, &s, [&](WsCarver& cv) { a_b = cv.array<uint16_t>(L.block.size()); },
                            [&](const WsCarver& cv) { s.d_block = cv(a_b); return cs_put(c, cv(a_b), L.block); });
}

// the tables of a fresh circuit: one pass of the table kernels, then four refreshes; cms: the 32 key commitments in the verifier
// key's order, or null
int install_tables(Ctx& c, Circuit& cir, const ShuffleCs& s, Jac* cms) {
    const uint32_t n = cir.n;
    const Fp* d_gen = nullptr;
    std::shared_ptr<DevBlock> evals;
    std::vector<Jac> cm(kShcsTables);
    UZK_TRY(cs_install_common(c, cir, kShcsTables, [&](Fp* d) {
        UZK_TRY(remark_device_tables(c, 0, nullptr, &d_gen));      // no key yet: the public-key columns start as the generator's
        return shcs_tables_run(c, cs_table_args(cir, s, nullptr, nullptr, d), s.d_block, d_gen, d_gen);
    }, &evals, cm.data()));
    const Fp* d = static_cast<const Fp*>(evals->p);
    UZK_TRY(circuit_refresh_device(c, cir, UZK_CS_QPK, 12, d + (size_t)kShcsTabPk * n, cm.data() + kShcsTabPk));
    UZK_TRY(circuit_refresh_device(c, cir, UZK_CS_QG, 13, d + (size_t)kShcsTabGen * n, cm.data() + kShcsTabGen));
    if (cms) {
        std::memcpy(cms, cm.data(), kCsCommonTables * sizeof(Jac));                            // cm_q, cm_s, cm_qb, cm_prk
        cms[19] = cm[kShcsTabEcc];
        std::memcpy(cms + 20, cm.data() + kShcsTabGen, 12 * sizeof(Jac));
    }
    return UZK_OK;
}

}  // namespace

// The entry points proper: api.cpp wraps each in its function-try-block.  They take the context lock themselves (the creation calls
// uzk_circuit_create, which takes it too).
namespace uzk {

int shcs_info(uint32_t cards, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out) {
    ShuffleLayout L;
    if (!shuffle_layout_build(cards, &L)) { set_error("uzk_shuffle_cs_info: %u cards (1 .. %d)", cards, UZK_SHUFFLE_CS_MAX_CARDS); return UZK_ERR_PARAMETER; }
    cs_info(L, size_out, n_out, num_vars_out, pi_count_out, pi_rows_out);
    return UZK_OK;
}

int shcs_circuit_create(const uzk_shuffle_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out) {
    if (!desc || !circuit_out) { set_error("uzk_shuffle_circuit_create: null pointer"); return UZK_ERR_PARAMETER; }
    auto s = std::make_shared<ShuffleCs>();
    if (!shuffle_layout_build(desc->cards, &s->host)) { set_error("uzk_shuffle_circuit_create: %u cards (1 .. %d)", desc->cards, UZK_SHUFFLE_CS_MAX_CARDS); return UZK_ERR_PARAMETER; }
    return cs_circuit_create(cs_desc_of(*desc), s->host, [](uzk_circuit_desc& cd) {
        const Fp one = Fr::one();
        cd.shuffle = 1;
        std::memcpy(cd.edwards_a, &one, sizeof one);               // Baby Jubjub: a = 1; no anemoi gates: generator and inverse zero
    }, kExtShuffle, s, [&](Ctx& c, Circuit& cir) {
        UZK_TRY(make_resident(c, *s));
        return install_tables(c, cir, *s, reinterpret_cast<Jac*>(commitments_out));
    }, circuit_out);
}

int shcs_circuit_set_key(uint64_t circuit, uint64_t remark_key, uzk_g1_jac* commitments_out) {
    API_LOCK;
    auto cir = find_circuit(circuit);
    auto s = shuffle_of(cir);
    if (!s) { set_error("uzk_shuffle_circuit_set_key: %llu is no circuit of uzk_shuffle_circuit_create", (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    if (!remark_key_known(remark_key, nullptr)) { set_error("uzk_shuffle_circuit_set_key: unknown remask key %llu", (unsigned long long)remark_key); return UZK_ERR_PARAMETER; }
    UZK_TRY(cs_circuit_here(*cir, "uzk_shuffle_circuit_set_key"));
    Ctx& c = ctx();
    const Fp* d_pk = nullptr;
    UZK_TRY(remark_device_tables(c, remark_key, &d_pk, nullptr));
    UZK_TRY(c.shuffle_ws.reserve((size_t)12 * cir->n * sizeof(Fp)));
    UZK_TRY(shcs_key_run(c, s->d_block, d_pk, c.shuffle_ws.as<Fp>(), cir->n));
    return circuit_refresh_device(c, *cir, UZK_CS_QPK, 12, c.shuffle_ws.as<Fp>(), reinterpret_cast<Jac*>(commitments_out));
}

int shcs_witness_batch(uint64_t circuit, uint64_t remark_key, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* digits,
                              const uint32_t* perms, uint32_t cards, uint32_t batch, void* d_witness, void* d_wsel, uint64_t* pi_values_out,
                       uint64_t* e1_out, uint64_t* e2_out) {
    static const char* who = "uzk_shuffle_witness_batch";
    API_LOCK;
    auto cir = find_circuit(circuit);
    auto s = shuffle_of(cir);
    if (!s) { set_error("%s: %llu is no circuit of uzk_shuffle_circuit_create", who, (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    if (cards != s->host.cards) { set_error("%s: decks of %u cards, the circuit is for %u", who, cards, s->host.cards); return UZK_ERR_PARAMETER; }
    if (batch == 0 || batch > UZK_SHUFFLE_CS_MAX_BATCH) { set_error("%s: %u decks (1 .. %d per call)", who, batch, UZK_SHUFFLE_CS_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!e1_mont || !e2_mont || !digits || !d_witness || !d_wsel || !pi_values_out || !e1_out || !e2_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    const ShuffleLayout& L = s->host;
    const uint32_t N = L.cards, total = batch * N, pi_count = (uint32_t)L.pi_vars.size();
    const Fp* pts[2] = {reinterpret_cast<const Fp*>(e1_mont), reinterpret_cast<const Fp*>(e2_mont)};
    for (int w = 0; w < 2; ++w) {
        const size_t bad = ed_first_noncanonical(pts[w], 2 * (size_t)total);
        if (bad < 2 * (size_t)total) { set_error("%s: e%d[%zu]: the %c coordinate is not below q", who, w + 1, bad / 2, bad % 2 ? 'y' : 'x'); return UZK_ERR_PARAMETER; }
    }
    for (size_t i = 0; i < (size_t)total * kShcsIters; ++i)
        if (digits[i] > 7) { set_error("%s: digit %zu of card %zu is %u (three bits: 0 .. 7)", who, i % kShcsIters, i / kShcsIters, digits[i]); return UZK_ERR_PARAMETER; }
    // perm of every deck (the identity where none is given) and slot[b N + perm_b[i]] = b N + i: where the remasked card goes
    std::vector<uint32_t> perm(total), slot(total, 0xffffffffu);
    for (uint32_t b = 0; b < batch; ++b)
        for (uint32_t i = 0; i < N; ++i) {
            const uint32_t p = perms ? perms[(size_t)b * N + i] : i;
            if (p >= N || slot[(size_t)b * N + p] != 0xffffffffu) { set_error("%s: deck %u: perm[%u] = %u: not a permutation of 0 .. %u", who, b, i, p, N - 1); return UZK_ERR_PARAMETER; }
            slot[(size_t)b * N + p] = b * N + i;
            perm[(size_t)b * N + i] = p;
        }
    if (!remark_key_known(remark_key, nullptr)) { set_error("%s: unknown remask key %llu", who, (unsigned long long)remark_key); return UZK_ERR_PARAMETER; }
    UZK_TRY(cs_circuit_here(*cir, who));
    Ctx& c = ctx();
    const size_t pt_words = 2 * (size_t)total;
    WsCarver cv;
    const auto a_e1 = cv.array<Fp>(pt_words), a_e2 = cv.array<Fp>(pt_words), a_o1 = cv.array<Fp>(pt_words), a_o2 = cv.array<Fp>(pt_words);
    const auto a_dg = cv.array<uint8_t>((size_t)total * kShcsIters);
    const auto a_perm = cv.array<uint32_t>(total), a_slot = cv.array<uint32_t>(total);
    const auto a_trace = cv.array<Fp>((size_t)total * kShcsIters * 4);
    const auto a_val = cv.array<Fp>((size_t)batch * L.num_vars), a_pi = cv.array<Fp>((size_t)batch * pi_count);
    UZK_TRY(cv.reserve(c.shuffle_ws));
    UZK_HIP(hipMemcpyAsync(cv(a_e1), e1_mont, a_e1.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_e2), e2_mont, a_e2.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_dg), digits, a_dg.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_perm), perm.data(), a_perm.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_slot), slot.data(), a_slot.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_TRY(remark_device_run(c, remark_key, reinterpret_cast<const EdAffine*>(cv(a_e1)), reinterpret_cast<const EdAffine*>(cv(a_e2)), cv(a_dg), cv(a_slot), total,
                              reinterpret_cast<EdAffine*>(cv(a_o1)), reinterpret_cast<EdAffine*>(cv(a_o2)), cv(a_trace)));
    ShcsWitnessArgs a = {};
    a.cards = N; a.n = L.n; a.num_vars = L.num_vars; a.pi_count = pi_count;
    a.defs = s->d_defs; a.wiring = s->d_wiring; a.pi_vars = s->d_pi_vars; a.block = s->d_block;
    a.e1 = cv(a_e1); a.e2 = cv(a_e2); a.digits = cv(a_dg); a.perm = cv(a_perm); a.trace = cv(a_trace);
    a.values = cv(a_val); a.witness = static_cast<Fp*>(d_witness); a.wsel = static_cast<Fp*>(d_wsel); a.pi = cv(a_pi);
    UZK_TRY(shcs_witness_run(c, a, batch));
    UZK_HIP(hipMemcpyAsync(pi_values_out, cv(a_pi), a_pi.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(e1_out, cv(a_o1), a_o1.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(e2_out, cv(a_o2), a_o2.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int shcs_test_tables(uint64_t circuit, uint64_t remark_key, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out) {
    API_LOCK;
    auto cir = find_circuit(circuit);
    auto s = shuffle_of(cir);
    if (!s) { set_error("uzk_test_shuffle_cs_tables: %llu is no circuit of uzk_shuffle_circuit_create", (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    if (remark_key && !remark_key_known(remark_key, nullptr)) { set_error("uzk_test_shuffle_cs_tables: unknown remask key %llu", (unsigned long long)remark_key); return UZK_ERR_PARAMETER; }
    UZK_TRY(cs_circuit_here(*cir, "uzk_test_shuffle_cs_tables"));
    Ctx& c = ctx();
    const size_t n = cir->n;
    UZK_TRY(cs_test_tables_common(c, *cir, *s, wiring_out, perm_out));
    if (evals_out) {
        const Fp *d_gen = nullptr, *d_pk = nullptr;
        UZK_TRY(remark_device_tables(c, 0, nullptr, &d_gen));
        if (remark_key) UZK_TRY(remark_device_tables(c, remark_key, &d_pk, nullptr));
        UZK_TRY(c.shuffle_ws.reserve(kShcsTables * n * sizeof(Fp)));
        UZK_TRY(shcs_tables_run(c, cs_table_args(*cir, *s, nullptr, nullptr, c.shuffle_ws.as<Fp>()), s->d_block, d_gen, remark_key ? d_pk : d_gen));
        UZK_HIP(hipMemcpyAsync(evals_out, c.shuffle_ws.p, kShcsTables * n * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    }
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

}  // namespace uzk
