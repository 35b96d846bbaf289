// The layout builder of zmatchmaking's circuit (uzkge_amd/csrc/matchcs_layout.cpp) on the CPU: plain C++, so g++ builds it alone, with
// sanitizers too.  For every player count on the command line the program checks the layout's own invariants and writes it to
// <out>/<players>.bin as little-endian uint32 words for tests/test_match_cs_ref_host.py to compare with the Python restatement:
//   players size n num_vars pi_count blocks | wiring 5n | perm 5n | sel 9n (as value + 32768) | qb n | prk_row n | defs num_vars |
//   pi_rows | pi_vars | block_rows
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../uzkge_amd/csrc/matchcs_layout.cpp"

using namespace uzk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int check(const MatchLayout& L) {
    const size_t total = (size_t)kMcsWires * L.n;
    CHECK(L.size == match_layout_size(L.players) && L.size <= L.n && (L.n & (L.n - 1)) == 0 && L.n < 2 * L.size);
    CHECK(L.wiring.size() == total && L.perm.size() == total && L.sel.size() == (size_t)kMcsSelectors * L.n);
    CHECK(L.qb.size() == L.n && L.prk_row.size() == L.n && L.defs.size() == L.num_vars);
    CHECK(L.pi_rows.size() == 2 * (size_t)L.players + 2 && L.pi_vars.size() == L.pi_rows.size() && L.block_rows.size() == 1 + (size_t)L.stream_perms);
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
        for (uint32_t i = 0; i < kMcsWires; ++i) CHECK(L.wiring[(size_t)i * L.n + row] == 0);
    // every definition's operands stay inside what the witness kernel indexes with them
    for (uint32_t d : L.defs) {
        const uint32_t kind = d >> 28, a = (d >> 16) & 0xfff, b = (d >> 8) & 0xff, c = d & 0xff;
        CHECK(kind <= kMcsSelect && c == 0);
        switch (kind) {
        case kMcsConst: case kMcsInput: CHECK(a < L.players); break;
        case kMcsSeed: case kMcsRandom: case kMcsCommit: CHECK(a == 0); break;
        case kMcsHashTrace: CHECK(a == 0 && b < kMcsTraceElems); break;
        case kMcsStreamTrace: CHECK(a < L.stream_perms && b < kMcsTraceElems); break;
        case kMcsStreamOut: CHECK(a + 1 < L.players); break;
        case kMcsQuot: case kMcsRem: CHECK(a >= 1 && a < L.players); break;
        case kMcsBit: case kMcsProduct: CHECK(a >= 1 && a < L.players && b <= a); break;
        case kMcsBitSum: case kMcsProdSum: CHECK(a >= 1 && a < L.players && b >= 1 && b <= a + 1); break;
        default: CHECK(a >= 1 && a < L.players && b < a); break;
        }
    }
    for (size_t k = 0; k < L.block_rows.size(); ++k)
        for (uint32_t r = 0; r < kMcsRounds + 1; ++r) CHECK(L.prk_row[L.block_rows[k] + r] == (r < kMcsRounds ? 1 + r : 0));
    return 0;
}

static void put(std::FILE* f, uint32_t v) { std::fwrite(&v, 4, 1, f); }

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: matchcs_host <out dir> <players>...\n"); return 2; }
    MatchLayout L;
    CHECK(!match_layout_build(0, &L) && !match_layout_build(kMcsMinPlayers - 1, &L) && !match_layout_build(kMcsMaxPlayers + 1, &L));
    for (int a = 2; a < argc; ++a) {
        const uint32_t players = (uint32_t)std::atoi(argv[a]);
        CHECK(match_layout_build(players, &L));
        if (check(L)) return 1;
        std::FILE* f = std::fopen((std::string(argv[1]) + "/" + std::to_string(players) + ".bin").c_str(), "wb");
        CHECK(f);
        put(f, L.players); put(f, L.size); put(f, L.n); put(f, L.num_vars); put(f, (uint32_t)L.pi_rows.size()); put(f, (uint32_t)L.block_rows.size());
        for (uint32_t v : L.wiring) put(f, v);
        for (uint32_t v : L.perm) put(f, v);
        for (int16_t v : L.sel) put(f, (uint32_t)(v + 32768));
        for (uint8_t v : L.qb) put(f, v);
        for (uint8_t v : L.prk_row) put(f, v);
        for (uint32_t v : L.defs) put(f, v);
        for (uint32_t v : L.pi_rows) put(f, v);
        for (uint32_t v : L.pi_vars) put(f, v);
        for (uint32_t v : L.block_rows) put(f, v);
        std::fclose(f);
    }
    std::printf("OK\n");
    return 0;
}
