// The layout builder of the reveal circuit (uzkge_amd/csrc/revealcs_layout.cpp) on the CPU: plain C++, so g++ builds it alone, with
// sanitizers too.  The program checks the layout's own invariants and writes it to <out>/reveal.bin as little-endian uint32 words for
// tests/test_reveal_cs_layout_host.py to compare with the Python restatement:
//   n_vars n_inputs n_constraints domain | per matrix A, B, C: nnz, row_ptr (n_constraints + 1), col (nnz), val (8 nnz) |
//   roles (n_vars) | multiples (256 x 2 x 8)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../uzkge_amd/csrc/revealcs_layout.cpp"

using namespace uzk;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static void put(std::FILE* f, uint32_t v) { std::fwrite(&v, 4, 1, f); }

static int check(const RevealLayout& L) {
    CHECK(L.n_vars == kRcsVars && L.n_inputs == kRcsInputs && L.n_constraints == kRcsConstraints && L.domain == kRcsDomain);
    CHECK(L.roles.size() == L.n_vars && L.multiples.size() == 2 * kRcsBits);
    for (const RcsMatrix& m : L.mat) {
        CHECK(m.row_ptr.size() == (size_t)L.n_constraints + 1 && m.row_ptr[0] == 0 && m.row_ptr.back() == m.col.size() && m.col.size() == m.val.size());
        for (uint32_t i = 0; i < L.n_constraints; ++i) {
            CHECK(m.row_ptr[i] <= m.row_ptr[i + 1]);
            for (uint64_t e = m.row_ptr[i]; e < m.row_ptr[i + 1]; ++e) {
                CHECK(m.col[e] < L.n_vars && !Fr::is_zero(m.val[e]));
                CHECK(e == m.row_ptr[i] || m.col[e - 1] < m.col[e]);
            }
        }
    }
    // the sections of the assignment, as the witness kernels index them
    for (uint32_t v = 0; v < kRcsInputs; ++v) CHECK(L.roles[v] == kRcsNoRole);
    for (uint32_t k = 0; k < 3; ++k) CHECK(L.roles[kRcsOffPoints + 2 * k] == rcs_role(kRcsPoint, k, kRcsX2) && L.roles[kRcsOffPoints + 2 * k + 1] == rcs_role(kRcsPoint, k, kRcsY2));
    for (uint32_t i = 0; i < kRcsBits; ++i) CHECK(L.roles[kRcsOffBits + i] == rcs_role(kRcsBit, i, kRcsBitRole));
    const uint32_t fixed[5] = {kRcsV0V1, kRcsX3, kRcsY3, kRcsSelX, kRcsSelY};
    const uint32_t var0[10] = {kRcsV0V1, kRcsX3, kRcsY3, kRcsSelX, kRcsSelY, kRcsXY, kRcsDX2, kRcsDY2, kRcsDX3, kRcsDY3};
    const uint32_t var[13] = {kRcsU, kRcsV0, kRcsV1, kRcsV0V1, kRcsX3, kRcsY3, kRcsSelX, kRcsSelY, kRcsXY, kRcsDX2, kRcsDY2, kRcsDX3, kRcsDY3};
    for (uint32_t i = 1; i < kRcsBits; ++i)
        for (uint32_t r = 0; r < kRcsFixedPer; ++r) CHECK(L.roles[kRcsOffFixed + kRcsFixedPer * (i - 1) + r] == rcs_role(kRcsFixed, i, fixed[r]));
    for (uint32_t r = 0; r < 10; ++r) CHECK(L.roles[kRcsOffVar + r] == rcs_role(kRcsVar, 0, var0[r]));
    for (uint32_t i = 1; i < kRcsBits; ++i)
        for (uint32_t r = 0; r < kRcsVarPer; ++r) CHECK(L.roles[kRcsOffVar1 + kRcsVarPer * (i - 1) + r] == rcs_role(kRcsVar, i, var[r]));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: revealcs_host <out dir>\n"); return 2; }
    RevealLayout L;
    CHECK(reveal_layout_build(&L));
    if (check(L)) return 1;
    std::FILE* f = std::fopen((std::string(argv[1]) + "/reveal.bin").c_str(), "wb");
    CHECK(f);
    put(f, L.n_vars); put(f, L.n_inputs); put(f, L.n_constraints); put(f, (uint32_t)L.domain);
    for (const RcsMatrix& m : L.mat) {
        put(f, (uint32_t)m.col.size());
        for (uint64_t v : m.row_ptr) put(f, (uint32_t)v);
        for (uint32_t v : m.col) put(f, v);
        for (const Fp& v : m.val)
            for (int i = 0; i < 8; ++i) put(f, v.v[i]);
    }
    for (uint32_t v : L.roles) put(f, v);
    for (const Fp& v : L.multiples)
        for (int i = 0; i < 8; ++i) put(f, v.v[i]);
    std::fclose(f);
    std::printf("OK\n");
    return 0;
}
