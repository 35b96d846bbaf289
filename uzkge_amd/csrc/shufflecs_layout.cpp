// The layout of zshuffle's circuit: the calls build_cs makes on a TurboCS, in their order, with a definition in place of every value.
// Plain C++17: tests/cpp/shufflecs_host.cpp builds this file with g++ and sanitizers.
#include "shufflecs.hpp"

namespace uzk {

uint32_t shuffle_layout_size(uint32_t cards) {
    const uint32_t n = cards, h = (n + 1) / 2;
    return 2 + 89 * n + 2 * n * ((n + 2) / 3 + 1) + 4 * n * (h + (h + 2) / 3) + 4 * n;
}

bool shuffle_layout_build(uint32_t cards, ShuffleLayout* out) {
    if (cards < 1 || cards > kShcsMaxCards) return false;
    ShuffleLayout& L = *out;
    L = ShuffleLayout();
    L.cards = cards;
    CsBuilder B(L);
    B.begin(shuffle_layout_size(cards));
    const uint32_t N = cards;
    L.block.assign(L.n, 0);
    const auto equal_one = [&B](uint32_t v) { B.gate({1, -1, 0, 0, 0, 0, 0, 0, 1}, v, 1, 0, 0, 0); };   // equal(v, one_var) = insert_sub_gate(v, 1, zero_var)
    const int16_t none[kCsSelectors] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> remarked((size_t)N * 4);                 // the CardVar eval_card_remark returns: trace entry 83
    for (uint32_t k = 0; k < N; ++k) {
        // new_card_variable: e1.x, e1.y, e2.x, e2.y; the CardVar is (e2.x, e2.y, e1.x, e1.y)
        uint32_t in[4];
        for (uint32_t c = 0; c < 4; ++c) in[c] = B.var(cs_def(kShcsInput, k, c));
        const uint32_t card[4] = {in[2], in[3], in[0], in[1]};
        for (uint32_t c = 0; c < 4; ++c) B.pi_gate(card[c]);
        // eval_card_remark: the block row is recorded first, then the 84 x 4 variables, then the 85 gates
        const uint32_t row = B.size();
        L.block_rows.push_back(row);
        for (uint32_t j = 0; j < kShcsIters; ++j) L.block[row + j] = (uint16_t)(1 + kShcsIters * k + j);
        const uint32_t v0 = (uint32_t)L.defs.size();               // trace variable (i, c) = v0 + 4 i + c
        for (uint32_t i = 0; i < kShcsIters; ++i)
            for (uint32_t c = 0; c < 4; ++c) B.var(cs_def(kShcsTrace, k, i, c));
        B.gate(none, card[0], card[1], card[2], card[3], v0 + 3);
        for (uint32_t r = 0; r + 1 < kShcsIters; ++r) B.gate(none, v0 + 4 * r, v0 + 4 * r + 1, v0 + 4 * r + 2, v0 + 4 * r + 3, v0 + 4 * (r + 1) + 3);
        const uint32_t last = v0 + 4 * (kShcsIters - 1);
        B.gate(none, last, last + 1, last + 2, last + 3, 0);
        for (uint32_t c = 0; c < 4; ++c) remarked[(size_t)k * 4 + c] = last + c;
    }
    // shuffle_card: the matrix row-major, row sums (boolean), column sums, then per output row and coordinate products and their sums
    const uint32_t m0 = (uint32_t)L.defs.size();                   // matrix variable (i, j) = m0 + N i + j
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t j = 0; j < N; ++j) B.var(cs_def(kShcsMatrix, i, j));
    std::vector<uint32_t> line(N);
    for (uint32_t i = 0; i < N; ++i) {
        for (uint32_t j = 0; j < N; ++j) line[j] = m0 + N * i + j;
        equal_one(B.sum_chunks(line, true, [i](uint32_t count) { return cs_def(kShcsRowSum, i, 0, count); }));
    }
    for (uint32_t j = 0; j < N; ++j) {
        for (uint32_t i = 0; i < N; ++i) line[i] = m0 + N * i + j;
        equal_one(B.sum_chunks(line, false, [j](uint32_t count) { return cs_def(kShcsColSum, j, 0, count); }));
    }
    std::vector<uint32_t> outputs((size_t)N * 4), products;
    for (uint32_t i = 0; i < N; ++i)
        for (uint32_t c = 0; c < 4; ++c) {
            products.clear();
            for (uint32_t at = 0; at < N; at += 2) {
                const uint32_t r = B.var(cs_def(kShcsProduct, i, c, at / 2));
                const bool two = at + 1 < N;
                B.gate({0, 0, 0, 0, 1, 1, 0, 0, 1}, m0 + N * i + at, remarked[(size_t)at * 4 + c], two ? m0 + N * i + at + 1 : 0,
                       two ? remarked[(size_t)(at + 1) * 4 + c] : 0, r);
                products.push_back(r);
            }
            outputs[(size_t)i * 4 + c] = B.sum_chunks(products, false, [i, c](uint32_t count) { return cs_def(kShcsProdSum, i, c, count); });
        }
    for (uint32_t v : outputs) B.pi_gate(v);
    return B.finish();                                             // false: the formula and the construction disagree, a bug here
}

}  // namespace uzk
