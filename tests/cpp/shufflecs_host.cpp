// The layout builder of zshuffle's circuit (uzkge_amd/csrc/shufflecs_layout.cpp) on the CPU: plain C++, so g++ builds it alone, with
// sanitizers too.  For every deck size on the command line the program checks the layout's own invariants and writes it to
// <out>/<cards>.bin as little-endian uint32 words for tests/test_shufflecs_host.py to compare with the Python restatement:
//   cards size n num_vars pi_count | wiring 5n | perm 5n | sel 9n (as value + 1) | qb n | block n | defs num_vars | pi_rows | pi_vars
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../uzkge_amd/csrc/shufflecs_layout.cpp"

using namespace uzk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int check(const ShuffleLayout& L) {
    const size_t total = (size_t)kShcsWires * L.n;
    CHECK(L.size == shuffle_layout_size(L.cards) && L.size <= L.n && (L.n & (L.n - 1)) == 0 && L.n < 2 * L.size);
    CHECK(L.wiring.size() == total && L.perm.size() == total && L.sel.size() == (size_t)kShcsSelectors * L.n);
    CHECK(L.qb.size() == L.n && L.block.size() == L.n && L.defs.size() == L.num_vars);
    CHECK(L.pi_rows.size() == 8 * (size_t)L.cards && L.pi_vars.size() == L.pi_rows.size() && L.block_rows.size() == L.cards);
    // the permutation: a bijection that never leaves a variable, and walks every position of a variable in one cycle
    std::vector<uint8_t> hit(total, 0);
    std::vector<uint32_t> uses(L.num_vars, 0);
    for (size_t p = 0; p < total; ++p) {
        CHECK(L.wiring[p] < L.num_vars && L.perm[p] < total && !hit[L.perm[p]]);
        hit[L.perm[p]] = 1;
        CHECK(L.wiring[L.perm[p]] == L.wiring[p]);
        ++uses[L.wiring[p]];
    }
    for (size_t p = 0; p < total; ++p) {
        if (L.perm[p] > p) continue;                               // the one step back of a cycle: from its last position to its first
        uint32_t len = 1;
        for (size_t at = L.perm[p]; at != p; at = L.perm[at]) { CHECK(L.perm[at] > at); ++len; }
        CHECK(len == uses[L.wiring[p]]);
    }
    for (uint32_t v = 0; v < L.num_vars; ++v) CHECK(uses[v] > 0);  // no dangling variable
    for (uint32_t row = L.size; row < L.n; ++row)
        for (uint32_t i = 0; i < kShcsWires; ++i) CHECK(L.wiring[(size_t)i * L.n + row] == 0);
    for (uint32_t k = 0; k < L.cards; ++k)
        for (uint32_t j = 0; j < kShcsBlockRows; ++j)
            CHECK(L.block[L.block_rows[k] + j] == (j < kShcsIters ? 1 + kShcsIters * k + j : 0));
    return 0;
}

static void put(std::FILE* f, uint32_t v) { std::fwrite(&v, 4, 1, f); }

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
        for (int8_t v : L.sel) put(f, (uint32_t)(v + 1));
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
