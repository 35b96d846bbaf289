// Keccak-f[1600], shared by host and device code: the permutation behind the verifier's transcript sponge (verify.hip) and the
// weight derivation of the SRS check (srscheck.hip).  Keccak-256 here always means rate 136, padding byte 0x01 (the original
// Keccak padding the reference's transcript uses, utils/transcript.rs), not SHA-3's 0x06.
#pragma once
#include <cstdint>

#include "fp256.hpp"

namespace uzk {

UZK_HD uint64_t vf_rol(uint64_t v, int s) { return s ? (v << s) | (v >> (64 - s)) : v; }
// lane x + 5 y; the rounds stay a loop (the round constant is the only thing that changes), every index is static
UZK_HD void vf_keccak_f(uint64_t (&a)[25]) {
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
                                 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
                                 0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
                                 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    constexpr int ROT[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t d = c[(x + 4) % 5] ^ vf_rol(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = vf_rol(a[x + 5 * y] ^ d, ROT[x][y]);
        }
#pragma unroll
        for (int y = 0; y < 5; ++y) {
#pragma unroll
            for (int x = 0; x < 5; ++x) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        }
        a[0] ^= RC[r];
    }
}

}  // namespace uzk
