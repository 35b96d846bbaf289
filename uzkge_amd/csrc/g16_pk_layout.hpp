// Where the points of an ark-serialize (compressed) Groth16 ProvingKey<Bn254> lie: the walk over the key's sections that
// uzk_g16_pk_layout returns and the two key-level decoders start from.  Plain C++17, no HIP in it and nothing of the library behind it:
// tests/cpp/g16_pk_layout_host.cpp builds it with g++ (and under the sanitizers) as a stand-alone program.
//
//     vk = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | Vec gamma_abc_g1,  then  beta_g1 | delta_g1 | Vec a_query | Vec b_g1_query |
//     Vec b_g2_query | Vec h_query | Vec l_query          (a Vec: u64 little-endian length, then the elements; G1 32 bytes, G2 64)
// The sections are numbered in the order of uzk_g16_pk_sections' arrays (UZK_PK_*), which is not the order of the bytes.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/uzkge_gpu.h"

namespace uzk {

enum PkParse { PK_PARSE_OK = 0, PK_PARSE_TRUNCATED = 1, PK_PARSE_LENGTH = 2, PK_PARSE_TRAILING = 3 };

inline const char* g16_pk_section_name(int s) {
    static const char* const names[UZK_G16_PK_SECTIONS] = {"alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1",
                                                          "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query"};
    return s >= 0 && s < UZK_G16_PK_SECTIONS ? names[s] : "?";
}
inline bool g16_pk_section_is_g2(int s) { return s == UZK_PK_BETA_G2 || s == UZK_PK_GAMMA_G2 || s == UZK_PK_DELTA_G2 || s == UZK_PK_B_G2_QUERY; }
inline size_t g16_pk_section_width(int s) { return g16_pk_section_is_g2(s) ? 64 : 32; }

// The sections of pk[0 .. len).  whole_key: the five sections of the verifying key, then the seven of the proving key, and nothing
// behind them; otherwise the verifying key alone, and bytes behind it are not looked at.  On an error *bad_section is the section the
// walk stood in.  out is written only on success.
inline PkParse g16_pk_layout_parse(const uint8_t* pk, size_t len, bool whole_key, uzk_g16_pk_sections* out, int* bad_section) {
    static const int order[UZK_G16_PK_SECTIONS] = {UZK_PK_ALPHA_G1, UZK_PK_BETA_G2, UZK_PK_GAMMA_G2, UZK_PK_DELTA_G2, UZK_PK_GAMMA_ABC_G1, UZK_PK_BETA_G1,
                                                   UZK_PK_DELTA_G1, UZK_PK_A_QUERY, UZK_PK_B_G1_QUERY, UZK_PK_B_G2_QUERY, UZK_PK_H_QUERY, UZK_PK_L_QUERY};
    uzk_g16_pk_sections lay = {};
    size_t pos = 0;
    const int sections = whole_key ? UZK_G16_PK_SECTIONS : 5;
    for (int k = 0; k < sections; ++k) {
        const int s = order[k];
        const bool vec = s == UZK_PK_GAMMA_ABC_G1 || s >= UZK_PK_A_QUERY;
        const size_t width = g16_pk_section_width(s);
        uint64_t count = 1;
        *bad_section = s;
        if (vec) {
            if (len - pos < 8) return PK_PARSE_TRUNCATED;
            count = 0;
            for (int b = 7; b >= 0; --b) count = (count << 8) | pk[pos + b];
            pos += 8;
            if (count > (len - pos) / width) return PK_PARSE_LENGTH;       // also every count whose byte size would overflow
        } else if (len - pos < width) {
            return PK_PARSE_TRUNCATED;
        }
        lay.offset[s] = pos;
        lay.count[s] = count;
        for (uint64_t i = 0; i < count; ++i) lay.infinities[s] += (pk[pos + (size_t)i * width + width - 1] >> 6) & 1;
        pos += (size_t)count * width;
    }
    if (whole_key && pos != len) { *bad_section = UZK_PK_L_QUERY; return PK_PARSE_TRAILING; }
    lay.bytes = pos;
    *out = lay;
    return PK_PARSE_OK;
}

}  // namespace uzk
