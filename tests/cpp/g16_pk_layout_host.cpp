// uzkge_amd/csrc/g16_pk_layout.hpp on the CPU: the walk over a compressed Groth16 proving key has no HIP in it, so plain g++ builds
// this program (tests/test_g16_pk_layout_host.py: once plain, once under Address- and UBSanitizer).  Every candidate key is copied
// into a heap block of exactly its length, so that a read past the end is the sanitizer's to see.
//   g16_pk_layout_host head.bin b-queries.bin tail.bin     the three parts of the key; prints OK and exits 0, or says which check
//                                                          failed and exits 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../uzkge_amd/csrc/g16_pk_layout.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

static uzk::PkParse parse(const std::vector<uint8_t>& key, size_t len, bool whole, uzk_g16_pk_sections* out, int* bad) {
    uint8_t* exact = new uint8_t[len ? len : 1];
    if (len) std::memcpy(exact, key.data(), len);
    const uzk::PkParse rc = uzk::g16_pk_layout_parse(exact, len, whole, out, bad);
    delete[] exact;
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::printf("usage: g16_pk_layout_host head.bin b-queries.bin tail.bin\n"); return 2; }
    std::vector<uint8_t> key;
    for (int i = 1; i < 4; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { std::printf("cannot read %s\n", argv[i]); return 2; }
        key.insert(key.end(), std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    CHECK(key.size() == 1041488);
    uzk_g16_pk_sections lay;
    int bad = -1;

    // the real key
    CHECK(parse(key, key.size(), true, &lay, &bad) == uzk::PK_PARSE_OK);
    const uint64_t counts[UZK_G16_PK_SECTIONS] = {1, 1, 1, 1, 7, 1, 1, 4869, 4869, 4869, 8191, 4862};
    const uint64_t infs[UZK_G16_PK_SECTIONS] = {0, 0, 0, 0, 0, 0, 0, 2046, 775, 775, 0, 0};
    for (int s = 0; s < UZK_G16_PK_SECTIONS; ++s) { CHECK(lay.count[s] == counts[s]); CHECK(lay.infinities[s] == infs[s]); }
    CHECK(lay.offset[UZK_PK_ALPHA_G1] == 0 && lay.offset[UZK_PK_GAMMA_ABC_G1] == 232 && lay.offset[UZK_PK_BETA_G1] == 456 && lay.bytes == key.size());
    CHECK(lay.offset[UZK_PK_L_QUERY] + 32 * lay.count[UZK_PK_L_QUERY] == key.size());
    // its head alone is a verifying key, with or without bytes behind it
    uzk_g16_pk_sections vk;
    CHECK(parse(key, 456, false, &vk, &bad) == uzk::PK_PARSE_OK && vk.bytes == 456 && vk.count[UZK_PK_GAMMA_ABC_G1] == 7 && vk.count[UZK_PK_A_QUERY] == 0);
    CHECK(parse(key, key.size(), false, &vk, &bad) == uzk::PK_PARSE_OK && vk.bytes == 456);
    CHECK(parse(key, 455, false, &vk, &bad) == uzk::PK_PARSE_LENGTH && bad == UZK_PK_GAMMA_ABC_G1);

    // cut at every section boundary, one byte before and one after: nothing but the whole key parses
    for (int s = 0; s < UZK_G16_PK_SECTIONS; ++s) {
        const size_t begin = (size_t)lay.offset[s], end = begin + (size_t)lay.count[s] * uzk::g16_pk_section_width(s);
        for (size_t at : {begin, end}) {
            for (int d = -1; d <= 1; ++d) {
                const size_t len = at + d;
                if (len > key.size() || (at == 0 && d < 0)) continue;
                uzk_g16_pk_sections t;
                std::memset(&t, 0x5a, sizeof t);
                const uzk::PkParse rc = parse(key, len, true, &t, &bad);
                if (len == key.size()) { CHECK(rc == uzk::PK_PARSE_OK); continue; }
                CHECK(rc == uzk::PK_PARSE_TRUNCATED || rc == uzk::PK_PARSE_LENGTH);
                CHECK(bad >= 0 && bad < UZK_G16_PK_SECTIONS);
                CHECK(t.bytes == 0x5a5a5a5a5a5a5a5aull);                 // out is written only on success
            }
        }
    }
    // a byte behind the key
    {
        std::vector<uint8_t> longer = key;
        longer.push_back(0);
        CHECK(parse(longer, longer.size(), true, &lay, &bad) == uzk::PK_PARSE_TRAILING);
    }
    // a length word of 2^63 (its byte size overflows 64 bits), of 2^64 - 1, and one too many
    for (uint64_t n : {1ull << 63, ~0ull, 4870ull}) {
        std::vector<uint8_t> k2 = key;
        for (int b = 0; b < 8; ++b) k2[520 + b] = (uint8_t)(n >> (8 * b));                 // a_query's length word
        CHECK(parse(k2, k2.size(), true, &lay, &bad) != uzk::PK_PARSE_OK);
        if (n != 4870) CHECK(bad == UZK_PK_A_QUERY);
    }
    // the empty input, and every length below a verifying key's fixed part
    CHECK(parse(key, 0, true, &lay, &bad) == uzk::PK_PARSE_TRUNCATED && bad == UZK_PK_ALPHA_G1);
    for (size_t len = 0; len < 232; ++len) CHECK(parse(key, len, false, &lay, &bad) == uzk::PK_PARSE_TRUNCATED);

    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("OK\n");
    return 0;
}
