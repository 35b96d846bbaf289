// compute_permutation (constraint_system/mod.rs:64-92) over the wire-major flattening of a circuit's wiring, shared by the layout
// builders (shufflecs_layout.cpp, matchcs_layout.cpp).  Plain C++17.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace uzk {

// Every position points to the next later one that holds the same variable, the last back to the first.  Positions are bucketed per
// variable by a counting sort: O(len), where the reference scans.  Every entry of `wiring` is below num_vars.
inline void cs_compute_permutation(const std::vector<uint32_t>& wiring, uint32_t num_vars, std::vector<uint32_t>* perm) {
    const size_t total = wiring.size();
    std::vector<uint32_t> start(num_vars + 1, 0), order(total);
    for (size_t p = 0; p < total; ++p) ++start[wiring[p] + 1];
    for (uint32_t v = 0; v < num_vars; ++v) start[v + 1] += start[v];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (size_t p = 0; p < total; ++p) order[fill[wiring[p]]++] = (uint32_t)p;
    perm->assign(total, 0);
    for (uint32_t v = 0; v < num_vars; ++v)
        for (uint32_t s = start[v]; s < start[v + 1]; ++s) (*perm)[order[s]] = order[s + 1 < start[v + 1] ? s + 1 : start[v]];
}

}  // namespace uzk
