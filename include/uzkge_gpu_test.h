/* uzkge_gpu_test.h -- TEST HOOKS of libuzkge_gpu.so.  NOT part of the drop-in ABI (include/uzkge_gpu.h): no host binding
 * declares them (rust/uzkge-gpu-sys binds uzkge_gpu.h only).  They are exported by the same shared library so that the known-answer
 * tests run against the very binary that ships -- a separate test build would check other machine code than the product's.
 * Users: tests/ (through uzkge_amd/_native.py TEST_PROTOTYPES) and tests/cpp/prover_rounds.cpp. */
#ifndef UZKGE_GPU_TEST_H
#define UZKGE_GPU_TEST_H
#include "uzkge_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- known-answer entry points: the DEVICE primitives applied element-wise to host arrays -------- */
/* field: 0 = Fq, 1 = Fr.  op: 0 mul (assembly FIPS), 1 add, 2 sub, 3 mul (portable CIOS), 4 sqr,
 * 5 neg, 6 from_mont, 7 to_mont, 8 add (portable), 9 sub (portable); 10..23 exercise the 9 x 29-bit
 * limb representation of the hot loops (fp29.hpp): 10 mul, 11 add, 12/13 sub with 4M / 12M offsets,
 * 14 a lazy-carry chain, 15 form round trip, 16/17 squaring vs product of a lazy operand, 18/19 the
 * multi-subtrahend offsets of ec29.hpp, 20 the dual product, 21..23 the C++ forms of the
 * assembly products 10 / 16 / 20; 24 / 25 the constant-operand product (a * b as PLAIN integers mod M, b canonical; 25 with a lazy
 * first operand 2 (a + 4M)), 26 its companion constant floor(b 2^261 / M) mod 2^256, 27 the NTT's lazy reduction of a + b + 4M, raw
 * (value < 3M, congruent to a + b); 28..33 the typed lazy arithmetic of lz29.hpp on canonical operands: 28 re-limb at offset -5 and
 * back by exact division by 32 (identity), 29 a b, 30 a - b, 31 a b + b b (ld -> typed operation -> to_wire), 32 into the 2^266-form
 * and back by exact division by 2^10 (identity), 33 a lazy chain 4 a - b across every offset the types generate.
 * a, b, out: n elements (host memory). */
int uzk_test_field_kat(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* The same primitives on operands the COMPILER can see: every (op, form_a, form_b) accepted here is a kernel of its own in which the
 * forms' fixed words are literals and only the rest is loaded from a / b (n elements each; the fixed words of the inputs are ignored).
 * op: 0 mul, 1 mul_rx (then canon), 2 sqr, 3 add, 4 sub, 5 add_rx, 6 sub_rx (then canon), 7 dbl; on 9 x 29-bit limbs re-limbed from
 * the loaded words, result through canon and to_fp: 8 mul(a, b), 9 sqr(a), 10 mul2(a, b, a, a), 11 mulc(a, w = b, wq_of(w)) (b
 * canonical).  form: 0 all eight words loaded, 1 words 0..3 loaded and 4..7 literal zero, 2 word 0 loaded and the rest zero, 3 the
 * literal R^2, 4 the literal (1, 0, .., 0), 5 zero(), 6 one(), 7 modulus() - 1; of the limbs: 8 limbs 0..4 loaded and 5..8 literal
 * zero, 9 limb 0 loaded and the rest zero, 10 LzOps::one() (form 0: all nine limbs from the loaded words).  portable: 0 the assembly
 * entry points, 1 mul_portable / add_portable / sub_portable / the _cpp products in the same shapes.  The accepted triples are the
 * CO_CASES list of csrc/fieldops.hip (mirrored by tests/test_gpu_asm_constant_operands.py); any other is UZK_ERR_PARAMETER. */
int uzk_test_const_operands(int field, int op, int form_a, int form_b, int portable, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* op: 0 a + b (mixed add), 1 a + b (full XYZZ add), 2 2a, 3 a - b, 4 2(a + b); 5..7 the four-lane addition of the
 * small-MSM folds (ecquad.hpp): 5 a + b, 6 2(a + b) (its doubling branch), 7 (a + b) + (a - b); 8..10 the same three on the
 * 29-bit-limb form (ecquad29.hpp), 11 4(a + b) by two quad doublings, 12 2(a + b) by one, 13 4a; 14..17 the one-lane additions on
 * the lazy 29-bit limbs with re-limbed operands (ec29l.hpp): 14 a + b, 15 2(a + b) (doubling branch), 16 (a + b) + (a - b),
 * 17 ((a + b) - (a + b)) + a + (b + infinity) (cancellation, infinity on either side); 18..21 the same four by quads.
 * Inputs affine (infinity = zeros), outputs Jacobian. */
int uzk_test_g1_kat(int op, const uzk_g1_affine* a, const uzk_g1_affine* b, uzk_g1_jac* out, size_t n);
/* The G2 primitives (csrc/fq2_29.hpp, g2_29.hpp).  op 0..5 on Fq2 elements (a, b, out: n x 8 words, c0 then c1): 0 mul (two dual
 * products), 1 sqr, 2 add, 3 sub, 4 neg, 5 mul (Karatsuba).  op 10..14 on points (a, b: n affine points of 16 words, infinity =
 * zeros; out: n Jacobian points of 24 words): 10 a + b by the accumulator's mixed addition (complete: doubling, cancellation,
 * infinity on either side), 11 a + b by the full XYZZ addition, 12 2a, 13 a - b (mixed, negated operand), 14 2(a + b). */
int uzk_test_g2_kat(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* The finish kernels of uzk_g16_prove_batch_finish (csrc/groth16.hip g16_chains, g16_combine) on the caller's points: record i is three
 * Jacobian points A, B1, K (any Z; infinity <=> z = 0) and the blinds r, s (Montgomery words); a_out[i] = the affine A, c_out[i] = the
 * affine s A + r B1 + K, canonical words, infinity all zeros.  A real key cannot be steered into the degenerate branches (equal or
 * opposite terms, an infinite operand or sum); this can.  n <= 4096. */
int uzk_test_g16_finish(const uzk_g1_jac* a_jac, const uzk_g1_jac* b1_jac, const uzk_g1_jac* k_jac, const uint64_t* r_mont, const uint64_t* s_mont, size_t n,
                        uzk_g1_affine* a_out, uzk_g1_affine* c_out);
/* How uzk_g16_prove_batch* would run a key of this shape, with no key: uzk_g16_key_create's rules for the three sizes (their error
 * codes), then *group_out = the proofs of one launch sequence, lens_out = the lengths of the G1 MSMs A, B1, K (n_vars + 2 twice,
 * (n_vars - n_inputs) + n) and admitted_out[i] = 1 iff the MSM code takes `group` vectors of lens_out[i] points in one call under the
 * calling context's tuning -- the very function the MSM entry refuses by.  Launches nothing, allocates nothing on the device. */
int uzk_test_g16_plan(uint32_t n_vars, uint32_t n_inputs, uint32_t n_constraints, uint32_t* group_out, uint64_t lens_out[3], int admitted_out[3]);

/* ---- raw 9 x 29-bit limbs: the primitives of the hot loops (fp29.hpp) and the typed lazy operations (lz29.hpp) at their bounds ----
 * in: n records of four operands a, b, c, d, 9 limbs (uint32) each, taken EXACTLY as given; out: n x 9 words, the raw result (no
 * canon); an 8-word result (to_fp*, canon of lz29.hpp, to_wire) in words 0..7 with word 8 = 0.  field: 0 = Fq, 1 = Fr.  op:
 * 0 mul(a, b), 1 sqr(a), 2 mul2(a, b, c, d) (generated assembly); 3..5 the same three in C++ (mul_cpp, sqr_cpp, mul2_cpp);
 * 6 mulc(a, w = b, wq_of(w)) (b canonical), 7 mulcs with ONE wave-uniform w = record 0's b; 8 add(a, b), 9 norm(a), 10 norm1(a),
 * 11 reduce(a), 12 reduce3(a), 13 canon(a), 14 to_fp(a), 15 to_fp_div<5>(a), 16 to_fp_div<10>(a), 17..19 sub<4 | 8 | 12>(a, b),
 * 20 sub_off(a, b, OFF) with param 0..5 = OFF4, OFF8, OFF12, OFF4T3, OFF2T1, OFF8T1; 21 the typed operation of signature `param`
 * of uzkge_amd/csrc/lz29_sigs.inc (its sub, to_wire or canon entries of this field); 22 reduce(from_fp_x32(words a.l[0..7]))
 * (what the MSM accumulator does to a loaded coordinate). */
int uzk_test_l29_kat(int field, int op, uint32_t param, const uint32_t* in, uint32_t* out, size_t n);
/* The lazy XYZZ additions of ec29l.hpp on raw coordinate limbs: record i of in is two points a, b (x, y, zz, zzz; 9 limbs each, 72
 * words), out[i] the raw result (36 words).  op: 0 a + b (p29_add), 1 2a (p29_dbl), 2 / 3 the same by the four lanes of a quad. */
int uzk_test_p29_kat(int op, const uint32_t* in, uint32_t* out, size_t n);
/* The G2 group law of g2_29.hpp on raw limbs.  A point is 73 words: x, y, zz, zzz, each c0 then c1 of 9 limbs, taken EXACTLY as given
 * (nothing re-limbed or reduced), then an infinity flag.  Record i of in is two points a, b and a flag word (147 words); out[i] is one
 * point, raw.  op: 0 g2p_add(a, b) on two G2P (every coordinate in 2^261-form, value < 16 M); 1 g2p_dbl(a); 2 g2acc_madd(a, p, flag)
 * with a an accumulator (x, y in 2^261-form < 16 M, zz, zzz in 2^266-form < 2 M) and p the wire affine point in b (x, y: eight
 * canonical words in the first eight limbs of each component; all zero = infinity), flag = negate; 3 the wire words of a, through
 * g2p_store (flag 0) or g2acc_store (flag 1): eight words per component, the ninth 0, out's flag = a's; 4 q2::is_zero of a's x
 * taken as E2<1, 32> (normalized or carry-step limbs, value < 32 M): the answer in out's flag, the coordinates zero. */
int uzk_test_g2_raw_kat(int op, const uint32_t* in, uint32_t* out, size_t n);
/* The prover's lane kernels (rounds.hip) on device polynomials: polynomial k of lane b holds its coefficients (wire elements) at
 * d_polys[k] + b * lane_strides[k] elements.  op 0, linear combination: lens[lanes][count] lengths, args[lanes][count] scalars,
 * out[lanes][len] = sum_k args[b][k] p_k,b (len = out_len).  op 1, evaluation: lens[count] lengths (every lane's), pts[count]
 * in {0, 1}, args[lanes][2] points, out[lanes][count] = p_k,b(args[b][pts[k]]) (len = max_len, 1 .. 2^18).  *kernel: bit 0 set
 * when the lazy 29-bit kernel ran, bit 1 when the wide one did (GS = 4 lanes per coefficient / PER = 16 per lane). */
int uzk_test_lanes(int op, const void* const* d_polys, const uint64_t* lane_strides, uint32_t count, const uint32_t* lens, const uint32_t* pts,
                   const uint64_t* args, uint32_t lanes, uint64_t len, uint64_t* out, int* kernel);

/* ntt_run exactly as uzk_ntt_fr_batch_strided_device calls it (forward only), with the caller's statement that every input vector
 * is zero from index in_len on (0 = no statement).  Synchronous.  Only the prover makes that statement (derive_cosets: in_len = n on
 * 6n-point slots; round 3: n + 8): with 3 * 2^k points, fused sub-transforms (n / 3 >= 4096) and 0 < in_len <= n / 3 the first
 * Stockham pass neither reads nor combines the two upper thirds and takes every element from in_len on as zero WITHOUT reading it --
 * whatever lies there.  Any other n or in_len runs the full transform.  Arguments and error codes as the public entry point's. */
int uzk_test_ntt_in_len(const void* d_in, uint64_t in_stride, void* d_out, uint64_t out_stride, uint64_t n, uint32_t batch,
                        const uint64_t* coset_shift_mont, uint64_t in_len);

/* Keccak-256 (padding byte 0x01) of `count` messages by the sponge of the verifier's transcript kernel (csrc/verify.hip), one lane
 * per message: message i is bytes [offsets[i], offsets[i + 1]) of msgs (count + 1 offsets), digests_out count x 32 bytes. */
int uzk_test_keccak256(const uint8_t* msgs, const uint64_t* offsets, uint32_t count, uint8_t* digests_out);

/* Weights 0 .. count - 1 of `seed` as the device kernel of uzk_srs_fold_powers writes them (csrc/srscheck.hip), copied back:
 * count x 4 limbs, Montgomery form.  uzk_srs_fold_weights is the host's run of the same code. */
int uzk_test_srs_weights_device(const uint8_t seed[32], uint64_t count, uint64_t* out_mont);

/* ---- the pairing (csrc/fq12_29.hpp, pairing.hip) ----
 * Fq12 on wire-form elements (uzk_gt's layout: 48 words each), one element per lane group.  op: 0 a b, 1 a^2, 2 a (b_0 + b_1 w + b_3 w^3)
 * (the product with a sparse line: b's other coefficients are ignored), 3 conj(a) (the p^6 map), 4 / 5 / 6 a^p, a^(p^2), a^(p^3),
 * 7 a^-1 by the norm chain (the inverse of 0 is 0), 8 the Granger-Scott square (defined on the cyclotomic subgroup only), 9 the easy part
 * a^((p^6 - 1)(p^2 + 1)), 10 the hard part a^((p^4 - p^2 + 1) / r) (for a in the cyclotomic subgroup).  Unary ops ignore b (it must still be
 * readable). */
int uzk_test_fq12_kat(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* The n Miller-loop values of the pairs, before the product and the final exponentiation (no point is checked). */
int uzk_test_miller(const uzk_g1_affine* p, const uzk_g2_affine* q, uint32_t n, uzk_gt* out);
/* Fq12 on RAW limbs, one element per lane group as above.  An element is 108 words: the coefficient of w^0 first, each c0 then c1 of 9
 * limbs, taken EXACTLY as given (nothing re-limbed or reduced) as members of q12::El = E2<1, 2> (2^261-form, low limbs below
 * 2^29 + 2^6, value < 2 M).  Record i of in is two elements a, b (216 words); out[i] is one element, raw (no to_wire, no canon).
 * op 0..10 as uzk_test_fq12_kat; 11 xi_mul of every coefficient of a; 12 q2::to_wire of every coefficient of a: eight canonical
 * words per component, the ninth 0. */
int uzk_test_fq12_raw_kat(int op, const uint32_t* in, uint32_t* out, size_t n);
/* One step of the Miller loop on RAW limbs, one record per lane group.  Record i of in (108 words): T = x, y, z and Q = qx, qy (each c0
 * then c1 of 9 limbs, members of E2<1, 2>), then xP and -yP (9 limbs each, members of Lz<Fq29, 1, 4>); 3 b' is the library's own
 * constant.  The hook fills the group's block of the LDS as the Miller kernel does (Q, 3 b', xP, -yP, then the barrier).  op 0
 * dbl_step, 1 add_step.  out[i] (126 words): x, y, z, l0, l1, l3 of the group's lane 0, raw, then 18 words holding the OR over the
 * other five coefficient lanes (and the six values) of their result XOR lane 0's: every lane computes the same step, so they are 0. */
int uzk_test_miller_step_raw(int op, const uint32_t* in, uint32_t* out, size_t n);
/* how the Miller kernel is laid out: pairs per wave = pairs per workgroup (a workgroup is one wave); the product tree's radix */
#define UZK_PAIRING_PAIRS_PER_WAVE 8
#define UZK_PAIRING_TREE_RADIX 8

/* ---- Baby Jubjub (csrc/ed29.hpp, edwards.hip) ----
 * The group law of ed29.hpp on RAW limbs, one record per lane.  A point is 36 words: x, y, z, t of 9 limbs each, taken EXACTLY as given
 * (nothing re-limbed or reduced) as members of ed::C = Lz<Fr29, 1, 2> (2^261-form, low limbs below 2^29 + 2^6, value < 2 M).  Record i of
 * in is two points a, b (72 words); out[i] is one point, raw, and a flag word (37 words).  op: 0 add(a, b); 1 neg(a); 2 is_identity(a),
 * 3 eq_affine(a, b.x, b.y), 4 on_curve(a.x, a.y): the answer in the flag, the point zero; 5 to_affine(a): the eight canonical wire words
 * of x and of y, the ninth 0, z and t zero; 6 inv(a.x), raw, in x. */
int uzk_test_ed_raw_kat(int op, const uint32_t* in, uint32_t* out, size_t n);

/* ---- synthetic circuits ----
 * TEST / TIMING ONLY -- changes results.  Marks the circuit as synthetic (random polynomials no witness satisfies, the frozen
 * parity vectors and the timing chains): round 3 then takes t as its first 5 n - 2 + sum(hiding) coefficients, as
 * tests/chain_oracle.py does, and the unsatisfied-witness check is off.  Never set it on a real circuit. */
int uzk_test_circuit_truncate_t(uint64_t circuit, int on);

/* The shuffle circuit as the library holds it: the wiring the witness kernel gathers by and the permutation round 2 walks (5 n
 * words each, downloaded from the device), and the 44 evaluation vectors the table kernels write, in slot order without l1 and
 * coset_quotient: q (9), s (5), qb, q_prk (4), q_shuffle_public_key (12), q_shuffle_generator (12), q_ecc -- 44 n elements.  The
 * public-key columns are laid out from `remark_key`'s T_pk, or from T_G when it is 0.  Every output optional (NULL). */
int uzk_test_shuffle_cs_tables(uint64_t circuit, uint64_t remark_key, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out);

/* The matchmaking circuit as the library holds it: the wiring and the permutation (5 n words each, downloaded from the device), and
 * the 19 evaluation vectors the table kernel writes, in slot order without l1 and coset_quotient: q (9), s (5), qb, q_prk (4) -- 19 n
 * elements.  Every output optional (NULL). */
int uzk_test_match_cs_tables(uint64_t circuit, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out);
/* The witness kernel's own division: `count` plain integers below r (4 words each, NOT Montgomery form) by m, 2 <= m <= 64.
 * quot_out: count x 4 words, plain; rem_out: count words. */
int uzk_test_match_divrem(const uint64_t* values, uint32_t m, uint32_t count, uint64_t* quot_out, uint32_t* rem_out);

/* The square roots of csrc/sqrt29.hpp, one lane per element.  field: 0 = Fq, 1 = Fq2 (8 words per element, c0 then c1), 2 = Fr.  a_mont:
 * n canonical Montgomery elements; root_out: n elements, a root where there is one (unspecified otherwise); is_square_out: n bytes,
 * 1 iff root^2 = a held on the device.  n outside 1 .. UZK_CODEC_MAX_BATCH or a word not below the modulus: UZK_ERR_PARAMETER. */
int uzk_test_sqrt_kat(int field, const uint64_t* a_mont, size_t n, uint64_t* root_out, uint8_t* is_square_out);

#ifdef __cplusplus
}
#endif
#endif
