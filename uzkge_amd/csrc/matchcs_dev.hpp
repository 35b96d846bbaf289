// What matchcs.cpp (the C ABI of the matchmaking circuit) and matchcs.hip (its kernels) share.
#pragma once
#include "cs_common.hpp"
#include "matchcs.hpp"

namespace uzk {

constexpr uint32_t kMcsLanes = 64;     // the lanes of the step kernel's one wave: lane j holds position j of the running output vector

// every pointer a device address
struct McsWitnessArgs {
    uint32_t players, n, num_vars, pi_count, stream_perms;
    const uint32_t *defs, *wiring, *pi_vars;
    const Fp *inputs, *seeds, *randoms;   // [batch][players], [batch], [batch]
    const Fp *commit, *hash_trace;     // [batch], [batch][64]: the hash of the seed and its trace
    const Fp *stream_out, *stream_trace;  // [batch][players - 1], [batch][stream_perms][64]
    Fp* quot;                          // [batch][64]: quotient of step i at i
    uint8_t* rem;                      // [batch][64]: remainder of step i at i
    uint8_t* state;                    // [batch][players + 1][64]: row i = the index vector before step i (row players: the outputs')
    Fp *values, *witness, *pi;         // [batch][num_vars], [batch][5][n], [batch][pi_count]
};

// steps (division, bits, the chain of exchanges), values, gather (cs_gather): three launches over traces that are already on the device
int mcs_witness_run(Ctx& c, const McsWitnessArgs& a, uint32_t batch);
// the step kernel's own division on `count` plain integers (device arrays): quot plain, rem words
int mcs_divrem_run(Ctx& c, const Fp* d_values, uint32_t m, uint32_t count, Fp* d_quot, uint32_t* d_rem);

// matchcs.cpp: what api.cpp's uzk_match_* and uzk_test_match_* forward to, argument for argument
int mcs_info(uint32_t players, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out);
int mcs_circuit_create(const uzk_match_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out);
int mcs_witness_batch(uint64_t circuit, const uint64_t* inputs_mont, const uint64_t* seeds_mont, const uint64_t* randoms_mont, uint32_t players,
                      uint32_t batch, void* d_witness, uint64_t* pi_values_out, uint64_t* outputs_out, uint64_t* commitments_out);
int mcs_test_tables(uint64_t circuit, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out);
int mcs_test_divrem(const uint64_t* values, uint32_t m, uint32_t count, uint64_t* quot_out, uint32_t* rem_out);

}  // namespace uzk
