// The layout of zmatchmaking's circuit: the calls build_cs and Matchmaking::generate_constraints (matchmaking.rs:42-229) make on a
// TurboCS, in their order, with a definition in place of every value.  Plain C++17: tests/cpp/matchcs_host.cpp builds this file with
// g++ and sanitizers.
#include "matchcs.hpp"

namespace uzk {

namespace {

constexpr int16_t kG = 5, kG2 = 26;                                // the MDS matrix [[1, g], [g, g^2 + 1]] of AnemoiJive254
constexpr uint32_t kNone = 0xffffffffu;

// anemoi_permutation_round (constraint_system/anemoi/mod.rs:10-196) without salt and checksum: the 56 variables of the rounds
// (trace elements 4 + 4 r + c of permutation `perm`), the 14 gates, one gate per wanted output word (kNone: not wanted)
void permutation(CsBuilder& B, MatchLayout& L, const uint32_t (&in)[4], const uint32_t (&out)[4], uint32_t kind, uint32_t perm) {
    const uint32_t v0 = (uint32_t)L.defs.size();                   // round r, word c = v0 + 4 r + c
    for (uint32_t r = 0; r < kMcsRounds; ++r)
        for (uint32_t c = 0; c < 4; ++c) B.var(cs_def(kind, perm, 4 + 4 * r + c));
    const int16_t none[kCsSelectors] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t row = B.size();
    L.block_rows.push_back(row);
    for (uint32_t r = 0; r < kMcsRounds; ++r) L.prk_row[row + r] = (uint8_t)(1 + r);
    B.gate(none, in[0], in[1], in[2], in[3], v0 + 3);
    for (uint32_t r = 1; r < kMcsRounds; ++r) B.gate(none, v0 + 4 * (r - 1), v0 + 4 * (r - 1) + 1, v0 + 4 * (r - 1) + 2, v0 + 4 * (r - 1) + 3, v0 + 4 * r + 3);
    const uint32_t last = v0 + 4 * (kMcsRounds - 1);
    const int16_t rows[4][4] = {{2, 2 * kG, kG, 1}, {2 * kG, 2 * kG2, kG2, kG}, {1, kG, kG, 1}, {kG, kG2, kG2, kG}};
    for (uint32_t o = 0; o < 4; ++o)
        if (out[o] != kNone) B.gate({rows[o][0], rows[o][1], rows[o][2], rows[o][3], 0, 0, 0, 0, 1}, last, last + 1, last + 2, last + 3, out[o]);
}

uint32_t stream_perms_of(uint32_t players) { return players <= 4 ? 1 : (players - 1 + 2) / 3; }

}  // namespace

uint32_t match_layout_size(uint32_t players) {
    const uint32_t n = players, p = stream_perms_of(players);
    uint32_t steps = 0;
    for (uint32_t i = 1; i < n; ++i) steps += 3 * i + 4 + 2 * ((i + 1 + 2) / 3);
    return n + 15 + (14 * p + (n - 1) + (p > 1 ? 1 : 0)) + steps + 2 * n + 2;
}

bool match_layout_build(uint32_t players, MatchLayout* out) {
    if (players < kMcsMinPlayers || players > kMcsMaxPlayers) return false;
    MatchLayout& L = *out;
    L = MatchLayout();
    L.players = players;
    L.stream_perms = stream_perms_of(players);
    CsBuilder B(L);
    B.begin(match_layout_size(players));
    const uint32_t N = players;
    L.prk_row.assign(L.n, 0);
    // build_cs: the inputs, the random number, the seed, its hash
    std::vector<uint32_t> outputs(N);
    for (uint32_t i = 0; i < N; ++i) outputs[i] = B.var(cs_def(kMcsInput, i));
    const std::vector<uint32_t> inputs = outputs;
    const uint32_t random_var = B.var(cs_def(kMcsRandom, 0)), seed_var = B.var(cs_def(kMcsSeed, 0)), commit_var = B.var(cs_def(kMcsCommit, 0));
    // generate_constraints: the constants 2 .. N - 1
    std::vector<uint32_t> index_vars = {0, 1};
    for (uint32_t i = 2; i < N; ++i) {
        const uint32_t v = B.var(cs_def(kMcsConst, i));
        B.constant_gate(v, (int16_t)i);
        index_vars.push_back(v);
    }
    // anemoi_variable_length_hash of one element: the chunk (seed, 1, 0), one permutation, one output gate
    permutation(B, L, {seed_var, 1, 0, 0}, {commit_var, kNone, kNone, kNone}, kMcsHashTrace, 0);
    // anemoi_stream_cipher over (seed, random): the chunk (seed, random, 1), sigma = zero_var; the one-input-chunk path
    std::vector<uint32_t> stream_out(N - 1);
    for (uint32_t i = 0; i + 1 < N; ++i) stream_out[i] = B.var(cs_def(kMcsStreamOut, i));
    auto chunk = [&](uint32_t rr, uint32_t (&o)[4]) {
        for (uint32_t c = 0; c < 3; ++c) o[c] = 3 * rr + c < N - 1 ? stream_out[3 * rr + c] : kNone;
        o[3] = kNone;
    };
    uint32_t o[4], state[4] = {seed_var, random_var, 1, 0};
    chunk(0, o);
    permutation(B, L, state, o, kMcsStreamTrace, 0);
    if (L.stream_perms > 1) {
        uint32_t next[4];
        for (uint32_t c = 0; c < 4; ++c) next[c] = B.var(cs_def(kMcsStreamTrace, 0, 60 + c));
        const uint32_t with_sigma = B.var(cs_def(kMcsStreamTrace, 0, 63));           // add(y1, zero_var): the same value
        B.gate({1, 1, 0, 0, 0, 0, 0, 0, 1}, next[3], 0, 0, 0, with_sigma);
        next[3] = with_sigma;
        for (uint32_t rr = 1; rr < L.stream_perms; ++rr) {
            for (uint32_t c = 0; c < 4; ++c) state[c] = next[c];
            if (rr != L.stream_perms - 1)
                for (uint32_t c = 0; c < 4; ++c) next[c] = B.var(cs_def(kMcsStreamTrace, rr, 60 + c));
            chunk(rr, o);
            permutation(B, L, state, o, kMcsStreamTrace, rr);
        }
    }
    // the N - 1 steps
    std::vector<uint32_t> bits, products;
    for (uint32_t i = 1; i < N; ++i) {
        const uint32_t n_var = B.var(cs_def(kMcsStreamOut, i - 1)), q_var = B.var(cs_def(kMcsQuot, i)), r_var = B.var(cs_def(kMcsRem, i));
        B.gate({(int16_t)(i + 1), 1, 0, 0, 0, 0, 0, 0, 1}, q_var, r_var, 0, 0, n_var);
        bits.clear();
        for (uint32_t j = 0; j <= i; ++j) bits.push_back(B.var(cs_def(kMcsBit, i, j)));
        B.constant_gate(B.sum_chunks(bits, true, [i](uint32_t count) { return cs_def(kMcsBitSum, i, count); }), 1);
        for (uint32_t j = 0; j <= i; ++j) B.gate({0, 0, 0, 0, 1, -1, 0, 0, 0}, index_vars[j], bits[j], r_var, bits[j], 0);
        const uint32_t output_i = outputs[i];
        products.clear();
        for (uint32_t j = 0; j <= i; ++j) {
            const uint32_t p = B.var(cs_def(kMcsProduct, i, j));
            B.gate({0, 0, 0, 0, 1, 0, 0, 0, 1}, bits[j], outputs[j], 0, 0, p);
            products.push_back(p);
        }
        outputs[i] = B.sum_chunks(products, false, [i](uint32_t count) { return cs_def(kMcsProdSum, i, count); });
        for (uint32_t j = 0; j < i; ++j) {
            const uint32_t s = B.var(cs_def(kMcsSelect, i, j));
            B.gate({0, 1, 0, 0, -1, 1, 0, 0, 1}, bits[j], outputs[j], bits[j], output_i, s);
            outputs[j] = s;
        }
    }
    // the public inputs: verify_matchmaking's online inputs
    for (uint32_t v : inputs) B.pi_gate(v);
    for (uint32_t v : outputs) B.pi_gate(v);
    B.pi_gate(random_var);
    B.pi_gate(commit_var);
    return B.finish();                                             // false: the formula and the construction disagree, a bug here
}

}  // namespace uzk
