// The matchmaking circuit behind the C ABI (include/uzkge_gpu.h, "the matchmaking circuit"): the layout of matchcs_layout.cpp made
// resident, its tables through the circuit's refresh path, and the witnesses of a batch of matches from two Anemoi sponges whose
// traces never leave the device.  A circuit made here is an ordinary Circuit (prover.hpp, shuffle = 0) that carries its layout in
// `ext` under the tag kExtMatch; the layout goes with the circuit's last reference.
#include <cstring>

#include "host_math.hpp"
#include "matchcs_dev.hpp"
#include "matchcs_consts.inc"

using namespace uzk;

namespace {

struct MatchCs : CsResident {
    MatchLayout host;
    const uint8_t* d_prk_row = nullptr;
    const Fp* d_prk = nullptr;                                     // [14][4]: the round keys after the linear layer
};

std::shared_ptr<MatchCs> match_of(const std::shared_ptr<Circuit>& cir) { return cs_ext<MatchCs>(cir, kExtMatch); }

int make_resident(Ctx& c, MatchCs& s) {
    const MatchLayout& L = s.host;
    WsArray<uint8_t> a_r;
    WsArray<Fp> a_k;
    return cs_make_resident(c, L, &s, [&](WsCarver& cv) { a_r = cv.array<uint8_t>(L.prk_row.size()); a_k = cv.array<Fp>(kMcsRounds * 4); },
                            [&](const WsCarver& cv) {
        s.d_prk_row = cv(a_r); s.d_prk = cv(a_k);
        UZK_TRY(cs_put(c, cv(a_r), L.prk_row));
        static_assert(sizeof kMcsPrk == kMcsRounds * 4 * sizeof(Fp), "one Fp per round key");
        UZK_HIP(hipMemcpyAsync(cv(a_k), kMcsPrk, sizeof kMcsPrk, hipMemcpyHostToDevice, c.stream));
        return UZK_OK;
    });
}

CsTableArgs table_args(const Circuit& cir, const MatchCs& s, Fp* d_out) { return cs_table_args(cir, s, s.d_prk_row, s.d_prk, d_out); }

}  // namespace

// The entry points proper: api.cpp wraps each in its function-try-block.  They take the context lock themselves (the creation calls
// uzk_circuit_create, which takes it too).
namespace uzk {

int mcs_info(uint32_t players, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out) {
    MatchLayout L;
    if (!match_layout_build(players, &L)) { set_error("uzk_match_cs_info: %u players (%d .. %d)", players, UZK_MATCH_CS_MIN_PLAYERS, UZK_MATCH_CS_MAX_PLAYERS); return UZK_ERR_PARAMETER; }
    cs_info(L, size_out, n_out, num_vars_out, pi_count_out, pi_rows_out);
    return UZK_OK;
}

int mcs_circuit_create(const uzk_match_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out) {
    if (!desc || !circuit_out) { set_error("uzk_match_circuit_create: null pointer"); return UZK_ERR_PARAMETER; }
    auto s = std::make_shared<MatchCs>();
    if (!match_layout_build(desc->players, &s->host)) { set_error("uzk_match_circuit_create: %u players (%d .. %d)", desc->players, UZK_MATCH_CS_MIN_PLAYERS, UZK_MATCH_CS_MAX_PLAYERS); return UZK_ERR_PARAMETER; }
    // without the "shuffle" feature; the tables: one pass of the table kernel and the two common refreshes; commitments_out: the 19
    // key commitments in the verifier key's order (cm_q, cm_s, cm_qb, cm_prk), or null
    return cs_circuit_create(cs_desc_of(*desc), s->host, [](uzk_circuit_desc& cd) {
        const Fp g = fr_from_u64(5), g_inv = fr_inv(g);            // AnemoiJive254: generator 5 and delta = 1 / 5; no edwards_a
        std::memcpy(cd.anemoi_g, &g, sizeof g);
        std::memcpy(cd.anemoi_g_inv, &g_inv, sizeof g_inv);
    }, kExtMatch, s, [&](Ctx& c, Circuit& cir) {
        UZK_TRY(make_resident(c, *s));
        std::shared_ptr<DevBlock> evals;
        std::vector<Jac> cm(kMcsTables);
        UZK_TRY(cs_install_common(c, cir, kMcsTables, [&](Fp* d) { return cs_tables_run(c, table_args(cir, *s, d)); }, &evals, cm.data()));
        if (commitments_out) std::memcpy(commitments_out, cm.data(), kMcsTables * sizeof(Jac));
        return UZK_OK;
    }, circuit_out);
}

int mcs_witness_batch(uint64_t circuit, const uint64_t* inputs_mont, const uint64_t* seeds_mont, const uint64_t* randoms_mont, uint32_t players,
                      uint32_t batch, void* d_witness, uint64_t* pi_values_out, uint64_t* outputs_out, uint64_t* commitments_out) {
    static const char* who = "uzk_match_witness_batch";
    API_LOCK;
    auto cir = find_circuit(circuit);
    auto s = match_of(cir);
    if (!s) { set_error("%s: %llu is no circuit of uzk_match_circuit_create", who, (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    if (players != s->host.players) { set_error("%s: matches of %u players, the circuit is for %u", who, players, s->host.players); return UZK_ERR_PARAMETER; }
    if (batch == 0 || batch > UZK_MATCH_CS_MAX_BATCH) { set_error("%s: %u matches (1 .. %d per call)", who, batch, UZK_MATCH_CS_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!inputs_mont || !seeds_mont || !randoms_mont || !d_witness || !pi_values_out || !outputs_out || !commitments_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    const MatchLayout& L = s->host;
    const uint32_t N = L.players, P = L.stream_perms, pi_count = (uint32_t)L.pi_vars.size();
    const struct { const char* name; const uint64_t* words; size_t per; } checked[3] = {{"input", inputs_mont, N}, {"seed", seeds_mont, 1}, {"random number", randoms_mont, 1}};
    for (const auto& ck : checked) {
        const size_t count = (size_t)batch * ck.per, bad = ed_first_noncanonical(reinterpret_cast<const Fp*>(ck.words), count);
        if (bad < count) { set_error("%s: %s %zu of match %zu is not below r", who, ck.name, bad % ck.per, bad / ck.per); return UZK_ERR_PARAMETER; }
    }
    UZK_TRY(cs_circuit_here(*cir, who));
    Ctx& c = ctx();
    // the cipher's input of a match: (seed, random number)
    std::vector<Fp> pairs(2 * (size_t)batch);
    for (uint32_t b = 0; b < batch; ++b) {
        std::memcpy(&pairs[2 * (size_t)b], seeds_mont + 4 * (size_t)b, sizeof(Fp));
        std::memcpy(&pairs[2 * (size_t)b + 1], randoms_mont + 4 * (size_t)b, sizeof(Fp));
    }
    WsCarver cv;
    const auto a_in = cv.array<Fp>((size_t)batch * N), a_seed = cv.array<Fp>(batch), a_rand = cv.array<Fp>(batch), a_pair = cv.array<Fp>(2 * (size_t)batch);
    const auto a_commit = cv.array<Fp>(batch), a_htr = cv.array<Fp>((size_t)batch * kMcsTraceElems);
    const auto a_sout = cv.array<Fp>((size_t)batch * (N - 1)), a_str = cv.array<Fp>((size_t)batch * P * kMcsTraceElems);
    const auto a_quot = cv.array<Fp>((size_t)batch * kMcsLanes);
    const auto a_rem = cv.array<uint8_t>((size_t)batch * kMcsLanes), a_state = cv.array<uint8_t>((size_t)batch * (N + 1) * kMcsLanes);
    const auto a_val = cv.array<Fp>((size_t)batch * L.num_vars), a_pi = cv.array<Fp>((size_t)batch * pi_count);
    UZK_TRY(cv.reserve(c.match_ws));
    UZK_HIP(hipMemcpyAsync(cv(a_in), inputs_mont, a_in.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_seed), seeds_mont, a_seed.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_rand), randoms_mont, a_rand.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_pair), pairs.data(), a_pair.bytes(), hipMemcpyHostToDevice, c.stream));
    // eval_variable_length_hash_with_trace(seed) and eval_stream_cipher_with_trace((seed, random), N - 1): outputs and traces stay in HBM
    UZK_TRY(anemoi_sponge_device(c, cv(a_seed), 1, batch, 0, cv(a_commit), cv(a_htr)));
    UZK_TRY(anemoi_sponge_device(c, cv(a_pair), 2, batch, N - 1, cv(a_sout), cv(a_str)));
    McsWitnessArgs a = {};
    a.players = N; a.n = L.n; a.num_vars = L.num_vars; a.pi_count = pi_count; a.stream_perms = P;
    a.defs = s->d_defs; a.wiring = s->d_wiring; a.pi_vars = s->d_pi_vars;
    a.inputs = cv(a_in); a.seeds = cv(a_seed); a.randoms = cv(a_rand); a.commit = cv(a_commit); a.hash_trace = cv(a_htr);
    a.stream_out = cv(a_sout); a.stream_trace = cv(a_str); a.quot = cv(a_quot); a.rem = cv(a_rem); a.state = cv(a_state);
    a.values = cv(a_val); a.witness = static_cast<Fp*>(d_witness); a.pi = cv(a_pi);
    UZK_TRY(mcs_witness_run(c, a, batch));
    UZK_HIP(hipMemcpyAsync(pi_values_out, cv(a_pi), a_pi.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(commitments_out, cv(a_commit), a_commit.bytes(), hipMemcpyDeviceToHost, c.stream));
    // the matched order: public inputs N .. 2 N of every match
    UZK_HIP(hipMemcpy2DAsync(outputs_out, (size_t)N * sizeof(Fp), cv(a_pi) + N, (size_t)pi_count * sizeof(Fp), (size_t)N * sizeof(Fp), batch, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int mcs_test_tables(uint64_t circuit, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out) {
    API_LOCK;
    auto cir = find_circuit(circuit);
    auto s = match_of(cir);
    if (!s) { set_error("uzk_test_match_cs_tables: %llu is no circuit of uzk_match_circuit_create", (unsigned long long)circuit); return UZK_ERR_PARAMETER; }
    UZK_TRY(cs_circuit_here(*cir, "uzk_test_match_cs_tables"));
    Ctx& c = ctx();
    const size_t n = cir->n;
    UZK_TRY(cs_test_tables_common(c, *cir, *s, wiring_out, perm_out));
    if (evals_out) {
        UZK_TRY(c.match_ws.reserve(kMcsTables * n * sizeof(Fp)));
        UZK_TRY(cs_tables_run(c, table_args(*cir, *s, c.match_ws.as<Fp>())));
        UZK_HIP(hipMemcpyAsync(evals_out, c.match_ws.p, kMcsTables * n * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    }
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int mcs_test_divrem(const uint64_t* values, uint32_t m, uint32_t count, uint64_t* quot_out, uint32_t* rem_out) {
    static const char* who = "uzk_test_match_divrem";
    API_LOCK;
    if (m < 2 || m > kMcsMaxPlayers) { set_error("%s: divisor %u (2 .. %u)", who, m, kMcsMaxPlayers); return UZK_ERR_PARAMETER; }
    if (count == 0 || count > (1u << 20)) { set_error("%s: %u values (1 .. 2^20)", who, count); return UZK_ERR_PARAMETER; }
    if (!values || !quot_out || !rem_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    const size_t bad = ed_first_noncanonical(reinterpret_cast<const Fp*>(values), count);
    if (bad < count) { set_error("%s: value %zu is not below r", who, bad); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    WsCarver cv;
    const auto a_v = cv.array<Fp>(count), a_q = cv.array<Fp>(count);
    const auto a_r = cv.array<uint32_t>(count);
    UZK_TRY(cv.reserve(c.match_ws));
    UZK_HIP(hipMemcpyAsync(cv(a_v), values, a_v.bytes(), hipMemcpyHostToDevice, c.stream));
    UZK_TRY(mcs_divrem_run(c, cv(a_v), m, count, cv(a_q), cv(a_r)));
    UZK_HIP(hipMemcpyAsync(quot_out, cv(a_q), a_q.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(rem_out, cv(a_r), a_r.bytes(), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

}  // namespace uzk
