// The circuit of a zmatchmaking proof as a function of the number of players: what build_cs (matchmaking/src/build_cs.rs:27-66) leaves
// in a TurboCS once the values are taken out of it.  The layout half is plain C++17 with no HIP in it (matchcs_layout.cpp builds with
// g++); the device half (matchcs.hip) turns a layout and the Anemoi traces of a batch of matches into evaluation vectors and witnesses.
#pragma once
#include "cs_layout.hpp"

namespace uzk {

constexpr uint32_t kMcsMinPlayers = 3, kMcsMaxPlayers = 64, kMcsRounds = 14, kMcsTraceElems = 64;
constexpr uint32_t kMcsWires = kCsWires, kMcsSelectors = kCsSelectors;     // the circuit's own names for the common shape
constexpr uint32_t kMcsTables = kCsCommonTables;                 // the evaluation vectors of a circuit: the common ones and no more

// How a variable's value follows from a match (inputs, seed, random number), its two Anemoi traces and the remainders
// rem_i = stream output i - 1 mod (i + 1) (cs_def).  The running output vector before step i is the inputs
// under an index vector idx_i (idx_1 = the identity; step i exchanges positions i and rem_i):
//   kMcsConst        the integer a (0 .. players - 1)
//   kMcsInput        input a
//   kMcsSeed, kMcsRandom, kMcsCommit    the committed seed, the random number, the hash of the seed
//   kMcsHashTrace    element b of permutation a of the hash's trace (AnemoiVLHTrace, the C ABI's layout: before 4, rounds 56, after 4)
//   kMcsStreamTrace  element b of permutation a of the stream cipher's trace
//   kMcsStreamOut    stream output a
//   kMcsQuot, kMcsRem    quotient and remainder of step a
//   kMcsBit          step a, position b: rem_a == b
//   kMcsBitSum       the first b bits of step a: rem_a < b
//   kMcsProduct      step a, position b: bit * output = rem_a == b ? input[idx_a[b]] : 0
//   kMcsProdSum      the first b products of step a: rem_a < b ? input[idx_a[rem_a]] : 0
//   kMcsSelect       step a, position b < a, after the step: input[idx_{a+1}[b]]
enum McsKind : uint32_t {
    kMcsConst = kCsConst, kMcsInput, kMcsSeed, kMcsRandom, kMcsCommit, kMcsHashTrace, kMcsStreamTrace, kMcsStreamOut, kMcsQuot, kMcsRem, kMcsBit,
    kMcsBitSum, kMcsProduct, kMcsProdSum, kMcsSelect
};

// CsLayout: the selector values are 0, +-1, 1 5 26 and their doubles, i + 1 <= 64, the constants; qb marks the running sums of the
// bits; pi: 2 players + 2, inputs, outputs, random number, commitment; block_rows: the first row of every permutation block, the
// hash's, then the cipher's
struct MatchLayout : CsLayout {
    uint32_t players = 0;
    uint32_t stream_perms = 0;                                     // permutations of the stream cipher: 1, or ceil((players - 1) / 3)
    std::vector<uint8_t> prk_row;                                  // [n]: 0, or 1 + round on row a + round of a permutation block
};

// gates before the pad: players + 15 + (14 P + players - 1 + [P > 1]) + sum_{i=1}^{players-1} (3 i + 4 + 2 ceil((i + 1) / 3)) + 2 players + 2
uint32_t match_layout_size(uint32_t players);
// false: players outside kMcsMinPlayers .. kMcsMaxPlayers
bool match_layout_build(uint32_t players, MatchLayout* out);

}  // namespace uzk
