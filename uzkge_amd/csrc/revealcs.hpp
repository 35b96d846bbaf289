// The R1CS of a Groth16 reveal proof: RevealCircuit (shuffle/src/reveal_with_snark.rs) over ark-r1cs-std 0.4's twisted Edwards gadget,
// as ark-relations leaves it once the values are taken out.  The layout half is plain C++17 with no HIP in it (revealcs_layout.cpp
// builds with g++); the device half (revealcs.hip) turns a secret and a batch of cards into full assignments.
//
//   variable 0           the constant one
//   1 .. 6               h.x h.y reveal.x reveal.y pk.x pk.y                                   (h = masked.e1; l = 7)
//   7 .. 12              x^2, y^2 of h, reveal, pk                                             (kRcsOffPoints)
//   13 .. 268            the 256 little-endian bits of sk                                      (kRcsOffBits)
//   269 + 5 (i - 1)      fixed-base chain, iteration i = 1 .. 255: v0v1 x3 y3 sel_x sel_y      (kRcsOffFixed; iteration 0 is linear)
//   1544 ..              variable-base chain, iteration 0: v0v1 x3 y3 sel_x sel_y xy x2 y2 dx3 dy3   (kRcsOffVar)
//   1554 + 13 (i - 1)    iteration i = 1 .. 255: u v0 v1 v0v1 x3 y3 sel_x sel_y xy x2 y2 dx3 dy3
// 4869 variables, 4869 rows: 9 curve checks, 256 bit rows, 255 x 5 + 2, 10 + 255 x 13 + 2.
#pragma once
#include <cstdint>
#include <vector>

#include "fp256.hpp"

namespace uzk {

constexpr uint32_t kRcsBits = 256, kRcsInputs = 7, kRcsVars = 4869, kRcsConstraints = 4869;
constexpr uint64_t kRcsDomain = 8192;
constexpr uint32_t kRcsOffPoints = 7, kRcsOffBits = 13, kRcsOffFixed = 269, kRcsOffVar = 1544, kRcsOffVar1 = 1554;
constexpr uint32_t kRcsFixedPer = 5, kRcsVarPer = 13;
static_assert(kRcsOffFixed + kRcsFixedPer * (kRcsBits - 1) == kRcsOffVar && kRcsOffVar1 + kRcsVarPer * (kRcsBits - 1) == kRcsVars, "the sections tile the assignment");

// what a witness is: chain, iteration, role (tests/reveal_cs_ref.py has the same codes)
enum RcsChain : uint32_t { kRcsPoint = 0, kRcsBit, kRcsFixed, kRcsVar };
enum RcsRole : uint32_t {
    kRcsX2 = 0, kRcsY2, kRcsBitRole, kRcsU, kRcsV0, kRcsV1, kRcsV0V1, kRcsX3, kRcsY3, kRcsSelX, kRcsSelY, kRcsXY, kRcsDX2, kRcsDY2, kRcsDX3, kRcsDY3
};
constexpr uint32_t kRcsNoRole = 0xffffffffu;                       // the instance variables
constexpr uint32_t rcs_role(uint32_t chain, uint32_t iteration, uint32_t role) { return (chain << 24) | (iteration << 8) | role; }

struct RcsMatrix {
    std::vector<uint64_t> row_ptr;                                 // [rows + 1]
    std::vector<uint32_t> col;                                     // sorted within a row, no zero coefficient
    std::vector<Fp> val;                                           // Montgomery words
};

struct RevealLayout {
    uint32_t n_vars = 0, n_inputs = 0, n_constraints = 0;
    uint64_t domain = 0;
    RcsMatrix mat[3];                                              // A, B, C
    std::vector<uint32_t> roles;                                   // [n_vars]: rcs_role, or kRcsNoRole
    std::vector<Fp> multiples;                                     // [256][2]: 2^i G affine, x then y
};

// false if the synthesis does not end at the counts above (a mistake in the builder: the callers refuse to go on)
bool reveal_layout_build(RevealLayout* out);

}  // namespace uzk
