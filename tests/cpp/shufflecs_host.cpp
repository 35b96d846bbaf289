// The layout builder of zshuffle's circuit (uzkge_amd/csrc/shufflecs_layout.cpp) on the CPU: plain C++, so g++ builds it alone, with
// sanitizers too.  For every deck size on the command line the program checks the layout's own invariants and writes it to
// <out>/<cards>.bin as little-endian uint32 words for tests/test_shufflecs_host.py to compare with the Python restatement:
//   cards size n num_vars pi_count | wiring 5n | perm 5n | sel 9n (as value + 1) | qb n | block n | defs num_vars | pi_rows | pi_vars
#include "cs_layout_check.hpp"
#include "../../uzkge_amd/csrc/shufflecs_layout.cpp"

using namespace uzk;

static int check(const ShuffleLayout& L) {
    if (cs_check_common(L, shuffle_layout_size(L.cards))) return 1;
    CHECK(L.block.size() == L.n && L.pi_rows.size() == 8 * (size_t)L.cards && L.block_rows.size() == L.cards);
    for (uint32_t k = 0; k < L.cards; ++k)
        for (uint32_t j = 0; j < kShcsBlockRows; ++j)
            CHECK(L.block[L.block_rows[k] + j] == (j < kShcsIters ? 1 + kShcsIters * k + j : 0));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: shufflecs_host <out dir> <cards>...\n"); return 2; }
    ShuffleLayout L;
    CHECK(!shuffle_layout_build(0, &L) && !shuffle_layout_build(kShcsMaxCards + 1, &L));
    for (int a = 2; a < argc; ++a) {
        const uint32_t cards = (uint32_t)std::atoi(argv[a]);
        CHECK(shuffle_layout_build(cards, &L));
        if (check(L)) return 1;
        std::FILE* f = std::fopen((std::string(argv[1]) + "/" + std::to_string(cards) + ".bin").c_str(), "wb");
        CHECK(f);
        put(f, L.cards); put(f, L.size); put(f, L.n); put(f, L.num_vars); put(f, (uint32_t)L.pi_rows.size());
        for (uint32_t v : L.wiring) put(f, v);
        for (uint32_t v : L.perm) put(f, v);
        for (int16_t v : L.sel) put(f, (uint32_t)(v + 1));
        for (uint8_t v : L.qb) put(f, v);
        for (uint16_t v : L.block) put(f, v);
        for (uint32_t v : L.defs) put(f, v);
        for (uint32_t v : L.pi_rows) put(f, v);
        for (uint32_t v : L.pi_vars) put(f, v);
        std::fclose(f);
    }
    std::printf("OK\n");
    return 0;
}
