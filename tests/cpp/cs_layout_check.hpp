// What the host programs of the circuit layouts (shufflecs_host.cpp, matchcs_host.cpp) share: the CHECK that ends a check, the
// invariants every layout of uzkge_amd/csrc/cs_layout.hpp holds, and the one word of a dump.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../uzkge_amd/csrc/cs_layout.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// `size` is the circuit's own formula for the gates before the pad
static int cs_check_common(const uzk::CsLayout& L, uint32_t size) {
    using namespace uzk;
    const size_t total = (size_t)kCsWires * L.n;
    CHECK(L.size == size && L.size <= L.n && (L.n & (L.n - 1)) == 0 && L.n < 2 * L.size);
    CHECK(L.wiring.size() == total && L.perm.size() == total && L.sel.size() == (size_t)kCsSelectors * L.n);
    CHECK(L.qb.size() == L.n && L.defs.size() == L.num_vars && L.pi_vars.size() == L.pi_rows.size());
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
        for (uint32_t i = 0; i < kCsWires; ++i) CHECK(L.wiring[(size_t)i * L.n + row] == 0);
    return 0;
}

static void put(std::FILE* f, uint32_t v) { std::fwrite(&v, 4, 1, f); }
