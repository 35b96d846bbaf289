// The circuit of a zshuffle proof as a function of the deck size: what build_cs (shuffle/src/build_cs.rs:26-55) leaves in a TurboCS
// once the values are taken out of it.  The layout half is plain C++17 with no HIP in it (shufflecs_layout.cpp builds with g++);
// the device half (shufflecs.hip) turns a layout, a remask key's tables and a remark trace into evaluation vectors and witnesses.
#pragma once
#include "cs_layout.hpp"

namespace uzk {

constexpr uint32_t kShcsMaxCards = 64, kShcsIters = 84, kShcsBlockRows = 85;
constexpr uint32_t kShcsWires = kCsWires, kShcsSelectors = kCsSelectors;   // the circuit's own names for the common shape
// The evaluation vectors of a circuit in slot order: the common 19 (q_prk zero), then q_shuffle_public_key (12),
// q_shuffle_generator (12), q_ecc
constexpr uint32_t kShcsTables = 44, kShcsTabPk = kCsCommonTables, kShcsTabGen = 31, kShcsTabEcc = 43;

// How a variable's value follows from a deck, its remark trace and the permutation (cs_def):
//   kShcsConst    a: 0 or 1
//   kShcsInput    card a, coordinate b (0 e1.x, 1 e1.y, 2 e2.x, 3 e2.y)
//   kShcsTrace    card a, iteration b, component c of (c2.x, c2.y, c1.x, c1.y)
//   kShcsMatrix   row a, column b of the permutation matrix: perm[a] == b
//   kShcsRowSum   the first c entries of row a;  kShcsColSum  the first c entries of column a
//   kShcsProduct  row a, coordinate b, pair c: M[a][2c] card[2c][b] + M[a][2c + 1] card[2c + 1][b] over the remasked cards
//   kShcsProdSum  the first c products of row a, coordinate b
enum ShcsKind : uint32_t { kShcsConst = kCsConst, kShcsInput, kShcsTrace, kShcsMatrix, kShcsRowSum, kShcsColSum, kShcsProduct, kShcsProdSum };

// CsLayout: every selector value is 0, 1 or -1; qb marks the row sums of the matrix; pi: 8 cards each, the deck, then the new deck;
// block_rows: the first row of every card's remark block
struct ShuffleLayout : CsLayout {
    uint32_t cards = 0;
    std::vector<uint16_t> block;                                   // [n]: 1 + 84 card + j on row j < 84 of a card's remark block, else 0
};

// gates before the pad: 2 + 89 N + 2 N (ceil(N/3) + 1) + 4 N (ceil(N/2) + ceil(ceil(N/2)/3)) + 4 N
uint32_t shuffle_layout_size(uint32_t cards);
// false: cards outside 1 .. kShcsMaxCards
bool shuffle_layout_build(uint32_t cards, ShuffleLayout* out);

}  // namespace uzk
