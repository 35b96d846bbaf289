// Host driver of the label-parametrised transcript digest of uzkge_amd/csrc/ed29.hpp -- plain C++ shared by host and device -- so that
// tests/test_shuffle_ref_host.py can hold the very code the kernels compile to Python integers, without a GPU (and under sanitizers).
//   cp_label_host masking <12 words>     the digest under "Masking" over x, y of g, h, u, v, a, b, as a big-endian integer
//   cp_label_host revealing <12 words>   the same under "Revealing", through the explicit label argument
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

int main(int argc, char** argv) {
    Fp w[12];
    if (argc != 14) return 2;
    for (int i = 0; i < 12; ++i)
        if (!rd(argv[2 + i], &w[i])) return 2;
    Fp d;
    if (!std::strcmp(argv[1], "masking")) d = cp_transcript_digest(w, cp_label_masking());
    else if (!std::strcmp(argv[1], "revealing")) d = cp_transcript_digest(w, cp_label_revealing());
    else return 2;
    for (int i = 7; i >= 0; --i) std::printf("%08x", d.v[i]);
    std::printf("\n");
    return 0;
}
