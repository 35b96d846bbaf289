// The layout builder of zmatchmaking's circuit (uzkge_amd/csrc/matchcs_layout.cpp) on the CPU: plain C++, so g++ builds it alone, with
// sanitizers too.  For every player count on the command line the program checks the layout's own invariants and writes it to
// <out>/<players>.bin as little-endian uint32 words for tests/test_match_cs_ref_host.py to compare with the Python restatement:
//   players size n num_vars pi_count blocks | wiring 5n | perm 5n | sel 9n (as value + 32768) | qb n | prk_row n | defs num_vars |
//   pi_rows | pi_vars | block_rows
#include "cs_layout_check.hpp"
#include "../../uzkge_amd/csrc/matchcs_layout.cpp"

using namespace uzk;

static int check(const MatchLayout& L) {
    if (cs_check_common(L, match_layout_size(L.players))) return 1;
    CHECK(L.prk_row.size() == L.n && L.pi_rows.size() == 2 * (size_t)L.players + 2 && L.block_rows.size() == 1 + (size_t)L.stream_perms);
    // every definition's operands stay inside what the witness kernel indexes with them
    for (uint32_t d : L.defs) {
        const uint32_t kind = cs_def_kind(d), a = cs_def_a(d), b = cs_def_b(d), c = cs_def_c(d);
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
