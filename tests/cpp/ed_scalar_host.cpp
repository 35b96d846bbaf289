// Host driver of the plain C++ of uzkge_amd/csrc/ed29.hpp -- the reduction of a 256-bit integer mod the subgroup order L, the
// multiply-add mod L of a Chaum-Pedersen response, and the Keccak-256 digest of the 448-byte reveal transcript -- so that
// tests/test_ed_ref_host.py can hold the very code the kernels compile to Python integers, without a GPU (and under sanitizers).
//   ed_scalar_host mod <v>            v mod L
//   ed_scalar_host mad <w> <c> <s>    (w + c s) mod L for w, c, s below L
//   ed_scalar_host dig <12 words>     the digest over x, y of e1, G, reveal, pk, a, b, as a big-endian integer
// Every number is 64 hexadecimal digits, in and out.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ed29.hpp"

using namespace uzk;

static bool rd(const char* hex, Fp* out) {
    if (std::strlen(hex) != 64) return false;
    for (int i = 0; i < 8; ++i) {
        char b[9];
        std::memcpy(b, hex + 8 * (7 - i), 8);
        b[8] = 0;
        out->v[i] = (uint32_t)std::strtoul(b, nullptr, 16);
    }
    return true;
}
static void pr(const Fp& a) {
    for (int i = 7; i >= 0; --i) std::printf("%08x", a.v[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    Fp w[12];
    const int n = argc - 2;
    if (argc < 3 || n > 12) return 2;
    for (int i = 0; i < n; ++i)
        if (!rd(argv[2 + i], &w[i])) return 2;
    if (!std::strcmp(argv[1], "mod") && n == 1) pr(ed_mod_order(w[0]));
    else if (!std::strcmp(argv[1], "mad") && n == 3) pr(ed_muladd_order(w[0], w[1], w[2]));
    else if (!std::strcmp(argv[1], "dig") && n == 12) pr(cp_transcript_digest(w));
    else return 2;
    return 0;
}
