// Host driver of the plain C++ of uzkge_amd/csrc/lane_tools.hpp -- a coordinate against its modulus, the big-endian word codec, the G1
// curve equation, the fixed-exponent power behind the two inversions and the square root -- so that tests/test_lane_tools_host.py can
// hold the very code the kernels compile to Python integers, without a GPU (and under sanitizers).  One command per line of the
// standard input, one line of output each; every number is a canonical integer in 64 hexadecimal digits, in and out:
//   below q|r <v>      1 if v is below the modulus, else 0
//   be <v>             the 32 bytes store_be32 writes, then the word load_be32 reads back from them
//   curve <x> <y>      1 if y^2 = x^3 + 3 in Fq, else 0
//   inv q|r <a>        a^(M - 2)
//   sqrt <a>           a^((p + 1) / 4) in Fq
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../uzkge_amd/csrc/lane_tools.hpp"

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
static void pr(const Fp& a, const char* end) {
    for (int i = 7; i >= 0; --i) std::printf("%08x", a.v[i]);
    std::printf("%s", end);
}

int main() {
    char line[256], cmd[8], a0[80], a1[80], a2[80];
    while (std::fgets(line, sizeof line, stdin)) {
        a0[0] = a1[0] = a2[0] = 0;
        const int n = std::sscanf(line, "%7s %79s %79s %79s", cmd, a0, a1, a2);
        if (n < 2) return 2;
        const bool fq = a0[0] == 'q';
        Fp v, w;
        if (!std::strcmp(cmd, "below") && n == 3 && rd(a1, &v)) {
            std::printf("%d\n", (fq ? below_modulus<FqCfg>(v) : below_modulus<FrCfg>(v)) ? 1 : 0);
        } else if (!std::strcmp(cmd, "be") && n == 2 && rd(a0, &v)) {
            alignas(4) uint8_t buf[32];
            store_be32(buf, v);
            for (int i = 0; i < 32; ++i) std::printf("%02x", buf[i]);
            std::printf(" ");
            pr(load_be32(buf), "\n");
        } else if (!std::strcmp(cmd, "curve") && n == 3 && rd(a0, &v) && rd(a1, &w)) {
            Affine p;
            p.x = Fq::to_mont(v); p.y = Fq::to_mont(w);
            std::printf("%d\n", g1_on_curve(p) ? 1 : 0);
        } else if (!std::strcmp(cmd, "inv") && n == 3 && rd(a1, &v)) {
            pr(fq ? Fq::from_mont(fq_inv_lane(Fq::to_mont(v))) : Fr::from_mont(fr_inv_lane(Fr::to_mont(v))), "\n");
        } else if (!std::strcmp(cmd, "sqrt") && n == 2 && rd(a0, &v)) {
            pr(Fq::from_mont(fq_sqrt_candidate(Fq::to_mont(v))), "\n");
        } else {
            return 2;
        }
    }
    return 0;
}
