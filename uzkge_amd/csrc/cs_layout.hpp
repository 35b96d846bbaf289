// What every circuit built on a TurboCS shares once the values are taken out of it: the shape of a layout, the definition word of a
// variable, the builder that mirrors TurboCS's own calls, and compute_permutation.  The circuits (shufflecs_layout.cpp,
// matchcs_layout.cpp) keep only what mirrors their build_cs.  Plain C++17, no HIP in it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace uzk {

constexpr uint32_t kCsWires = 5, kCsSelectors = 9;
// The evaluation vectors every circuit starts with, in slot order, without l1 and coset_quotient (which have no evaluation form of
// their own): q (9), s (5), qb, q_prk (4)
constexpr uint32_t kCsTabS = 9, kCsTabQb = 14, kCsTabPrk = 15, kCsCommonTables = 19;

// How a variable's value follows from the circuit's inputs: kind << 28 | a << 16 | b << 8 | c.  The kinds are the circuit's own but
// for the first: kCsConst, the integer a
constexpr uint32_t kCsConst = 0;
constexpr uint32_t cs_def(uint32_t kind, uint32_t a, uint32_t b = 0, uint32_t c = 0) { return kind << 28 | a << 16 | b << 8 | c; }
constexpr uint32_t cs_def_kind(uint32_t d) { return d >> 28; }
constexpr uint32_t cs_def_a(uint32_t d) { return (d >> 16) & 0xfff; }
constexpr uint32_t cs_def_b(uint32_t d) { return (d >> 8) & 0xff; }
constexpr uint32_t cs_def_c(uint32_t d) { return d & 0xff; }

struct CsLayout {
    uint32_t size = 0, n = 0, num_vars = 0;                        // size: gates before the pad; n: after it
    std::vector<uint32_t> wiring;                                  // [5][n] variable indices
    std::vector<uint32_t> perm;                                    // [5][n]: compute_permutation over the wire-major flattening
    std::vector<int16_t> sel;                                      // [9][n]: small integers (zshuffle: 0 and +-1 only)
    std::vector<uint8_t> qb;                                       // [n]: 1 on the boolean rows
    std::vector<uint32_t> defs;                                    // [num_vars]
    std::vector<uint32_t> pi_rows, pi_vars;                        // the public inputs: their gates, their variables
    std::vector<uint32_t> block_rows;                              // the first row of every block of gates the custom selectors cover
};

// compute_permutation (constraint_system/mod.rs:64-92) over the wire-major flattening of a circuit's wiring: every position points
// to the next later one that holds the same variable, the last back to the first.  Positions are bucketed per variable by a
// counting sort: O(len), where the reference scans.  Every entry of `wiring` is below num_vars.
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

// The calls a build_cs makes on a TurboCS, with a definition in place of every value.  The layout must be a fresh one.
struct CsBuilder {
    std::vector<uint32_t> w[kCsWires];
    std::vector<int16_t> q[kCsSelectors];
    CsLayout& L;
    explicit CsBuilder(CsLayout& l) : L(l) {}

    // TurboCS::new(): zero_var, one_var and their constant gates;
    // n is the next power of two at or above `size`, the gates the circuit will have made by finish()
    void begin(uint32_t size) {
        L.size = size;
        L.n = 1;
        while (L.n < size) L.n *= 2;
        L.qb.assign(L.n, 0);
        var(cs_def(kCsConst, 0));
        var(cs_def(kCsConst, 1));
        constant_gate(0, 0);
        constant_gate(1, 1);
    }
    uint32_t size() const { return (uint32_t)w[0].size(); }
    uint32_t var(uint32_t def) {                                   // new_variable
        L.defs.push_back(def);
        return (uint32_t)L.defs.size() - 1;
    }
    // finish_new_gate after the nine push_*_selector calls: q = (q1, q2, q3, q4, qm1, qm2, qc, q_ecc, qo)
    void gate(const int16_t (&qs)[kCsSelectors], uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t o) {
        const uint32_t wires[kCsWires] = {a, b, c, d, o};
        for (uint32_t i = 0; i < kCsSelectors; ++i) q[i].push_back(qs[i]);
        for (uint32_t i = 0; i < kCsWires; ++i) w[i].push_back(wires[i]);
    }
    void constant_gate(uint32_t v, int16_t constant) { gate({0, 0, 0, 0, 0, 0, constant, 0, 1}, v, v, v, v, v); }
    void pi_gate(uint32_t v) {                                     // prepare_pi_variable
        L.pi_vars.push_back(v);
        L.pi_rows.push_back(size());
        constant_gate(v, 0);
    }
    // the running sum of `vars` in chunks of 3 (linear_combine with the absent entries on zero_var and a zero selector); the sum
    // after the chunk that ends at entry `count` is the variable def_of(count)
    template <class DefOf>
    uint32_t sum_chunks(const std::vector<uint32_t>& vars, bool boolean, DefOf def_of) {
        uint32_t acc = 0;
        for (size_t at = 0; at < vars.size(); at += 3) {
            const size_t len = std::min<size_t>(3, vars.size() - at);
            const uint32_t out = var(def_of((uint32_t)(at + len)));
            gate({1, 1, (int16_t)(len > 1), (int16_t)(len > 2), 0, 0, 0, 0, 1}, acc, vars[at], len > 1 ? vars[at + 1] : 0, len > 2 ? vars[at + 2] : 0, out);
            if (boolean) L.qb[size() - 1] = 1;
            acc = out;
        }
        return acc;
    }
    // the pad and the flattening; false: the gates made are not the `size` begin() was told, a bug in the circuit's formula
    bool finish() {
        if (size() != L.size) return false;
        const uint32_t n = L.n;
        L.num_vars = (uint32_t)L.defs.size();
        L.wiring.assign((size_t)kCsWires * n, 0);
        L.sel.assign((size_t)kCsSelectors * n, 0);
        for (uint32_t i = 0; i < kCsWires; ++i) std::copy(w[i].begin(), w[i].end(), L.wiring.begin() + (size_t)i * n);
        for (uint32_t i = 0; i < kCsSelectors; ++i) std::copy(q[i].begin(), q[i].end(), L.sel.begin() + (size_t)i * n);
        cs_compute_permutation(L.wiring, L.num_vars, &L.perm);
        return true;
    }
};

}  // namespace uzk
