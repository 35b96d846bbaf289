// What shufflecs.cpp (the C ABI of the shuffle circuit) and shufflecs.hip (its kernels) share.
#pragma once
#include "cs_common.hpp"
#include "shufflecs.hpp"

namespace uzk {

// every pointer a device address
struct ShcsWitnessArgs {
    uint32_t cards, n, num_vars, pi_count;
    const uint32_t *defs, *wiring, *pi_vars;
    const uint16_t* block;
    const Fp *e1, *e2;                 // [batch][cards] points, x then y
    const uint8_t* digits;             // [batch][cards][84]
    const uint32_t* perm;              // [batch][cards]
    const Fp* trace;                   // [batch][cards][84][4]
    Fp *values, *witness, *wsel, *pi;  // [batch][num_vars], [batch][5][n], [batch][3][n], [batch][pi_count]
};

// all 44 evaluation vectors into a.out: the common ones, T_pk's columns, T_G's columns, q_ecc
int shcs_tables_run(Ctx& c, const CsTableArgs& a, const uint16_t* d_block, const Fp* d_gen, const Fp* d_pk);
// the 12 columns of one table: d_out [12][n]
int shcs_key_run(Ctx& c, const uint16_t* d_block, const Fp* d_table, Fp* d_out, uint32_t n);
// values, gather (cs_gather), wire selectors: three launches over a remask that is already on the device
int shcs_witness_run(Ctx& c, const ShcsWitnessArgs& a, uint32_t batch);

// shufflecs.cpp: what api.cpp's uzk_shuffle_* and uzk_test_shuffle_cs_tables forward to, argument for argument
int shcs_info(uint32_t cards, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out);
int shcs_circuit_create(const uzk_shuffle_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out);
int shcs_circuit_set_key(uint64_t circuit, uint64_t remark_key, uzk_g1_jac* commitments_out);
int shcs_witness_batch(uint64_t circuit, uint64_t remark_key, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* digits,
                       const uint32_t* perms, uint32_t cards, uint32_t batch, void* d_witness, void* d_wsel, uint64_t* pi_values_out,
                       uint64_t* e1_out, uint64_t* e2_out);
int shcs_test_tables(uint64_t circuit, uint64_t remark_key, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out);

}  // namespace uzk
