// The circuit of a zshuffle proof as a function of the deck size: what build_cs (shuffle/src/build_cs.rs:26-55) leaves in a TurboCS
// once the values are taken out of it.  The layout half is plain C++17 with no HIP in it (shufflecs_layout.cpp builds with g++);
// the device half (shufflecs.hip) turns a layout, a remask key's tables and a remark trace into evaluation vectors and witnesses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace uzk {

constexpr uint32_t kShcsMaxCards = 64, kShcsWires = 5, kShcsSelectors = 9, kShcsIters = 84, kShcsBlockRows = 85;
// The evaluation vectors of a circuit in slot order, without l1 and coset_quotient (which have no evaluation form of their own):
// q (9), s (5), qb, q_prk (4, zero), q_shuffle_public_key (12), q_shuffle_generator (12), q_ecc
constexpr uint32_t kShcsTables = 44, kShcsTabS = 9, kShcsTabQb = 14, kShcsTabPrk = 15, kShcsTabPk = 19, kShcsTabGen = 31, kShcsTabEcc = 43;

// How a variable's value follows from a deck, its remark trace and the permutation: kind << 28 | a << 16 | b << 8 | c
//   kConst    a: 0 or 1
//   kInput    card a, coordinate b (0 e1.x, 1 e1.y, 2 e2.x, 3 e2.y)
//   kTrace    card a, iteration b, component c of (c2.x, c2.y, c1.x, c1.y)
//   kMatrix   row a, column b of the permutation matrix: perm[a] == b
//   kRowSum   the first c entries of row a;  kColSum  the first c entries of column a
//   kProduct  row a, coordinate b, pair c: M[a][2c] card[2c][b] + M[a][2c + 1] card[2c + 1][b] over the remasked cards
//   kProdSum  the first c products of row a, coordinate b
enum ShcsKind : uint32_t { kConst = 0, kInput, kTrace, kMatrix, kRowSum, kColSum, kProduct, kProdSum };
constexpr uint32_t shcs_def(uint32_t kind, uint32_t a, uint32_t b, uint32_t c) { return kind << 28 | a << 16 | b << 8 | c; }

struct ShuffleLayout {
    uint32_t cards = 0, size = 0, n = 0, num_vars = 0;             // size: gates before the pad; n: after it
    std::vector<uint32_t> wiring;                                  // [5][n] variable indices
    std::vector<uint32_t> perm;                                    // [5][n]: compute_permutation over the wire-major flattening
    std::vector<int8_t> sel;                                       // [9][n]: every selector value of this circuit is 0, 1 or -1
    std::vector<uint8_t> qb;                                       // [n]: 1 on the boolean rows (the row sums of the matrix)
    std::vector<uint16_t> block;                                   // [n]: 1 + 84 card + j on row j < 84 of a card's remark block, else 0
    std::vector<uint32_t> defs;                                    // [num_vars]
    std::vector<uint32_t> pi_rows, pi_vars;                        // 8 cards each: the deck, then the new deck
    std::vector<uint32_t> block_rows;                              // the first row of every card's remark block
};

// gates before the pad: 2 + 89 N + 2 N (ceil(N/3) + 1) + 4 N (ceil(N/2) + ceil(ceil(N/2)/3)) + 4 N
uint32_t shuffle_layout_size(uint32_t cards);
// false: cards outside 1 .. kShcsMaxCards
bool shuffle_layout_build(uint32_t cards, ShuffleLayout* out);

}  // namespace uzk
