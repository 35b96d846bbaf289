// The layout of zshuffle's circuit: the calls build_cs makes on a TurboCS, in their order, with a definition in place of every value.
// Plain C++17: tests/cpp/shufflecs_host.cpp builds this file with g++ and sanitizers.
#include "shufflecs.hpp"

#include <algorithm>

#include "csperm.hpp"

namespace uzk {

namespace {

struct Builder {
    std::vector<uint32_t> w[kShcsWires];
    std::vector<int8_t> q[kShcsSelectors];
    ShuffleLayout& L;
    explicit Builder(ShuffleLayout& l) : L(l) {}

    uint32_t size() const { return (uint32_t)w[0].size(); }
    uint32_t var(uint32_t def) {                                   // new_variable
        L.defs.push_back(def);
        return (uint32_t)L.defs.size() - 1;
    }
    // finish_new_gate after the nine push_*_selector calls: q = (q1, q2, q3, q4, qm1, qm2, qc, q_ecc, qo)
    void gate(const int8_t (&qs)[kShcsSelectors], uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t o) {
        const uint32_t wires[kShcsWires] = {a, b, c, d, o};
        for (uint32_t i = 0; i < kShcsSelectors; ++i) q[i].push_back(qs[i]);
        for (uint32_t i = 0; i < kShcsWires; ++i) w[i].push_back(wires[i]);
    }
    void constant_gate(uint32_t v, int8_t constant) { gate({0, 0, 0, 0, 0, 0, constant, 0, 1}, v, v, v, v, v); }
    void pi_gate(uint32_t v) {                                     // prepare_pi_variable
        L.pi_vars.push_back(v);
        L.pi_rows.push_back(size());
        constant_gate(v, 0);
    }
    void equal_one(uint32_t v) { gate({1, -1, 0, 0, 0, 0, 0, 0, 1}, v, 1, 0, 0, 0); }     // equal(v, one_var) = insert_sub_gate(v, 1, zero_var)
    // the running sum of `vars` in chunks of 3 (linear_combine with the absent entries on zero_var and a zero selector); the sum
    // after the chunk that ends at entry `count` is the variable shcs_def(kind, a, b, count)
    uint32_t sum_chunks(const std::vector<uint32_t>& vars, bool boolean, uint32_t kind, uint32_t a, uint32_t b) {
        uint32_t acc = 0;
        for (size_t at = 0; at < vars.size(); at += 3) {
            const size_t len = std::min<size_t>(3, vars.size() - at);
            const uint32_t out = var(shcs_def(kind, a, b, (uint32_t)(at + len)));
            gate({1, 1, (int8_t)(len > 1), (int8_t)(len > 2), 0, 0, 0, 0, 1}, acc, vars[at], len > 1 ? vars[at + 1] : 0, len > 2 ? vars[at + 2] : 0, out);
            if (boolean) L.qb[size() - 1] = 1;
            acc = out;
        }
        return acc;
    }
};

}  // namespace

uint32_t shuffle_layout_size(uint32_t cards) {
    const uint32_t n = cards, h = (n + 1) / 2;
    return 2 + 89 * n + 2 * n * ((n + 2) / 3 + 1) + 4 * n * (h + (h + 2) / 3) + 4 * n;
}

bool shuffle_layout_build(uint32_t cards, ShuffleLayout* out) {
    if (cards < 1 || cards > kShcsMaxCards) return false;
    ShuffleLayout& L = *out;
    L = ShuffleLayout();
    L.cards = cards;
    L.size = shuffle_layout_size(cards);
    L.n = 1;
    while (L.n < L.size) L.n *= 2;
    const uint32_t n = L.n, N = cards;
    L.qb.assign(n, 0);
    L.block.assign(n, 0);
    Builder B(L);
    // TurboCS::new(): zero_var, one_var and their constant gates
    B.var(shcs_def(kConst, 0, 0, 0));
    B.var(shcs_def(kConst, 1, 0, 0));
    B.constant_gate(0, 0);
    B.constant_gate(1, 1);
    const int8_t none[kShcsSelectors] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> remarked((size_t)N * 4);                 // the CardVar eval_card_remark returns: trace entry 83
    for (uint32_t k = 0; k < N; ++k) {
        // new_card_variable: e1.x, e1.y, e2.x, e2.y; the CardVar is (e2.x, e2.y, e1.x, e1.y)
        uint32_t in[4];
        for (uint32_t c = 0; c < 4; ++c) in[c] = B.var(shcs_def(kInput, k, c, 0));
        const uint32_t card[4] = {in[2], in[3], in[0], in[1]};
        for (uint32_t c = 0; c < 4; ++c) B.pi_gate(card[c]);
        // eval_card_remark: the block row is recorded first, then the 84 x 4 variables, then the 85 gates
        const uint32_t row = B.size();
        L.block_rows.push_back(row);
        for (uint32_t j = 0; j < kShcsIters; ++j) L.block[row + j] = (uint16_t)(1 + kShcsIters * k + j);
        const uint32_t v0 = (uint32_t)L.defs.size();               // trace variable (i, c) = v0 + 4 i + c
        for (uint32_t i = 0; i < kShcsIters; ++i)
            for (uint32_t c = 0; c < 4; ++c) B.var(shcs_def(kTrace, k, i, c));
        B.gate(none, card[0], card[1], card[2], card[3], v0 + 3);
        for (uint32_t r = 0; r + 1 < kShcsIters; ++r) B.gate(none, v0 + 4 * r, v0 + 4 * r + 1, v0 + 4 * r + 2, v0 + 4 * r + 3, v0 + 4 * (r + 1) + 3);
        const uint32_t last = v0 + 4 * (kShcsIters - 1);
        B.gate(none, last, last + 1, last + 2, last + 3, 0);
        for (uint32_t c = 0; c < 4; ++c) remarked[(size_t)k * 4 + c] = last + c;
    }
    // shuffle_card: the matrix row-major, row sums (boolean), column sums, then per output row and coordinate products and their sums
    const uint32_t m0 = (uint32_t)L.defs.size();                   // matrix variable (i, j) = m0 + N i + j
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t j = 0; j < N; ++j) B.var(shcs_def(kMatrix, i, j, 0));
    std::vector<uint32_t> line(N);
    for (uint32_t i = 0; i < N; ++i) {
        for (uint32_t j = 0; j < N; ++j) line[j] = m0 + N * i + j;
        B.equal_one(B.sum_chunks(line, true, kRowSum, i, 0));
    }
    for (uint32_t j = 0; j < N; ++j) {
        for (uint32_t i = 0; i < N; ++i) line[i] = m0 + N * i + j;
        B.equal_one(B.sum_chunks(line, false, kColSum, j, 0));
    }
    std::vector<uint32_t> outputs((size_t)N * 4), products;
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t c = 0; c < 4; ++c) {
            products.clear();
            for (uint32_t at = 0; at < N; at += 2) {
                const uint32_t r = B.var(shcs_def(kProduct, i, c, at / 2));
                const bool two = at + 1 < N;
                B.gate({0, 0, 0, 0, 1, 1, 0, 0, 1}, m0 + N * i + at, remarked[(size_t)at * 4 + c], two ? m0 + N * i + at + 1 : 0,
                       two ? remarked[(size_t)(at + 1) * 4 + c] : 0, r);
                products.push_back(r);
            }
            outputs[(size_t)i * 4 + c] = B.sum_chunks(products, false, kProdSum, i, c);
        }
    for (uint32_t v : outputs) B.pi_gate(v);
    if (B.size() != L.size) return false;                          // the formula and the construction disagree: a bug here
    // pad, and the flattening
    L.num_vars = (uint32_t)L.defs.size();
    L.wiring.assign((size_t)kShcsWires * n, 0);
    L.sel.assign((size_t)kShcsSelectors * n, 0);
    for (uint32_t i = 0; i < kShcsWires; ++i) std::copy(B.w[i].begin(), B.w[i].end(), L.wiring.begin() + (size_t)i * n);
    for (uint32_t i = 0; i < kShcsSelectors; ++i) std::copy(B.q[i].begin(), B.q[i].end(), L.sel.begin() + (size_t)i * n);
    cs_compute_permutation(L.wiring, L.num_vars, &L.perm);
    return true;
}

}  // namespace uzk
