/*
 * uzkge_gpu.h -- C ABI of the MI355X (gfx950) backend for uzkge's PlonK prover hot path.
 *
 * The reference (zypher-game/uzkge, /root/reference) has no FFI/plugin surface; the boundary is
 * the pair of Rust call sites that carry the heavy arithmetic:
 *
 *   G1Projective::msm(&points_raw, &coefs)   uzkge/src/poly_commit/kzg_poly_commitment.rs:287-290
 *   domain.fft(&self.coefs)                   uzkge/src/poly_commit/field_polynomial.rs:585
 *   domain.ifft(&values)                      uzkge/src/poly_commit/field_polynomial.rs:595
 *
 * A Rust `uzkge-gpu-sys` shim binds exactly these symbols (INTEGRATION.md shows the binding).
 *
 * Data layout (bit-identical to ark-ff `Fp<MontBackend<_,4>,4>`'s inner `BigInt<4>`):
 *   field element  = 4 x uint64 little-endian limbs, Montgomery form, R = 2^256
 *   uzk_g1_affine  = x || y (64 B); the point at infinity is encoded as x = y = 0
 *   uzk_g1_jac     = x || y || z (96 B), Jacobian (x/z^2, y/z^3); infinity <=> z == 0
 * The Jacobian representative of a result is not unique; compare after affine normalisation.
 *
 * Ownership: every pointer is caller-owned for the duration of the call; the library keeps no
 * reference except data explicitly copied (or adopted) by uzk_srs_register*.  Outputs go to
 * caller memory.  All functions are thread-safe (one lock per context, see uzk_ctx_create); none panics or aborts.
 *
 * Error codes map onto `UzkgeError` (uzkge/src/errors.rs:5-44):
 *   UZK_ERR_DEGREE     -> UzkgeError::DegreeError      (commit: len > SRS len, kzg_poly_commitment.rs:283-285)
 *   UZK_ERR_FFT        -> UzkgeError::FFTError         (no evaluation domain of that size)
 *   UZK_ERR_COMMITMENT -> UzkgeError::CommitmentError  (length mismatch: ark `msm` Err(min_len))
 *   UZK_ERR_PARAMETER  -> UzkgeError::ParameterError   (bad handle / null pointer)
 *   UZK_ERR_DEVICE     -> (new) no gfx950 device, HIP runtime failure, out of device memory; also out of HOST memory inside the
 *                         library (no C++ exception leaves an entry point: each is a function-try-block)
 * There is NO CPU fallback: without a usable GPU every compute entry point returns UZK_ERR_DEVICE.
 */
#ifndef UZKGE_GPU_H
#define UZKGE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UZK_OK 0
#define UZK_ERR_PARAMETER 1
#define UZK_ERR_DEGREE 2
#define UZK_ERR_FFT 3
#define UZK_ERR_COMMITMENT 4
#define UZK_ERR_DEVICE 5

typedef struct { uint64_t x[4], y[4]; } uzk_g1_affine;
typedef struct { uint64_t x[4], y[4], z[4]; } uzk_g1_jac;

/* ---- lifecycle ------------------------------------------------------------------------ */
/* Bind the calling process to HIP device `device` (one process per GPU); idempotent for the
 * same ordinal.  Creates the library stream and workspaces.  The library never edits the process environment: a host
 * that runs more than four prover threads (one context each) should export GPU_MAX_HW_QUEUES=16 before the process
 * makes its first HIP call -- the HIP runtime multiplexes streams onto four hardware queues by default. */
int uzk_init(int device);
int uzk_shutdown(void);
/* Number of visible HIP devices (0 when none / no driver); never fails. */
int uzk_device_count(void);
/* Thread-local description of the last non-OK return on this thread. */
const char* uzk_last_error(void);
const char* uzk_version(void);

/* ---- contexts (optional) ---------------------------------------------------------------- */
/* A context = one stream, one set of workspaces, one lock.  Every entry point works on the calling thread's current
 * context; threads that never set one share the default context (and serialise on its lock).  Giving each prover
 * thread its own context lets independent proofs overlap on the GPU -- at the real circuit size (n = 2^14) a single
 * proof leaves most of the chip idle.  SRS handles are process-wide and may be used from every context; register and
 * precompute them before the contexts start sharing them. */
/* The new context starts with the creator's current tuning (uzk_tune, uzk_msm_set_window_bits). */
int uzk_ctx_create(uint64_t* ctx_out);
/* A context on a named device ("uzk_init(n_devices)"): one process can then drive several GPUs -- prover threads
 * with a context, circuits and provers each on their own device, or the point chunks of one MSM (uzk_msm_g1_sharded).
 * uzk_init keeps its meaning: the device of the default context and of uzk_ctx_create.  SRS handles, circuits and provers
 * live on the device of the context that made them; using one from a context on another device is UZK_ERR_PARAMETER. */
int uzk_ctx_create_on(int device, uint64_t* ctx_out);
/* the device context `ctx` (0: the default context) lives on */
int uzk_ctx_device(uint64_t ctx, int* device_out);
/* Makes `ctx` (0 = the default context) the calling thread's current context. */
int uzk_ctx_set_current(uint64_t ctx);
/* Frees the context's stream, plans and workspaces; no thread may be inside a call on it.  A thread whose current
 * context has been destroyed (here or by uzk_shutdown) works on the default context from its next call on. */
int uzk_ctx_destroy(uint64_t ctx);
/* The calling thread's current context waits -- on the device, the host does not block -- for everything queued so far on
 * context `other` (0 = the default context).  A prover thread that owns TWO contexts has two lanes, each with its own stream
 * and workspaces: steps of a proof that do not depend on each other run side by side (the coset FFTs of the wire polynomials
 * under the commit of the same round, uzkge/src/plonk/prover.rs:160-192 / helpers.rs:256-266; the two batch_prove openings,
 * prover.rs:349-372), and this call is the dependency edge between the lanes. */
int uzk_ctx_wait(uint64_t other);
/* The calling thread's current context (0 = the default one). */
int uzk_ctx_current(uint64_t* ctx_out);

/* ---- device memory ------------------------------------------------------------------------ */
/* Everything a host language needs to keep data resident between the *_device entry points: with these it links
 * libuzkge_gpu.so and nothing else (no HIP runtime, no hip headers).  The reference keeps every polynomial of a proof in
 * Vec<Fr> between its steps (uzkge/src/plonk/prover.rs:151-372); these are the device-side Vecs.
 * Copies and fills are ordered on the calling context's stream, i.e. with that context's kernels:
 *   UZK_COPY_D2H  the data is in `dst` when the call returns;
 *   UZK_COPY_H2D  `src` may be reused when the call returns -- except for memory of uzk_host_alloc (pinned), whose
 *                 uploads are asynchronous: keep it unchanged until the next synchronising call (uzk_sync, a D2H copy, a
 *                 commit);
 *   UZK_COPY_D2D  asynchronous.
 * uzk_dev_free / uzk_host_free wait for the calling context's stream first.  Allocations belong to the caller and
 * survive uzk_shutdown. */
#define UZK_COPY_H2D 0
#define UZK_COPY_D2H 1
#define UZK_COPY_D2D 2
int uzk_dev_alloc(size_t bytes, void** d_out);
int uzk_dev_free(void* d_ptr);
int uzk_host_alloc(size_t bytes, void** h_out);
int uzk_host_free(void* h_ptr);
int uzk_dev_copy(void* dst, const void* src, size_t bytes, int kind);
/* `rows` rows of `width` bytes; consecutive rows are dst_pitch / src_pitch bytes apart. */
int uzk_dev_copy2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows, int kind);
int uzk_dev_memset(void* d_dst, int byte, size_t bytes);
int uzk_dev_memset2d(void* d_dst, size_t pitch, int byte, size_t width, size_t rows);

/* ---- SRS (the static bases of KZG commit) --------------------------------------------- */
/* Copy `n` affine points to HBM once; replaces the per-commit `normalize_batch` of
 * kzg_poly_commitment.rs:287-288.  Returns an opaque handle (never 0). */
int uzk_srs_register(const uzk_g1_affine* points, size_t n, uint64_t* handle_out);
/* Adopt points that already live in device memory (no copy; caller keeps them alive). */
int uzk_srs_register_device(const void* d_points, size_t n, uint64_t* handle_out);
int uzk_srs_release(uint64_t handle);
/* Optional, for a static SRS (KZG): build the window table T[j][i] = 2^(c*j) * SRS[i] in HBM
 * (W * n * 64 bytes, W = ceil(254 / c); c = window_bits or automatic when 0).  Later MSMs on this
 * handle then use one shared bucket set (larger windows, no per-window reduction, no host
 * combination).  Results are identical; only speed and memory change. */
int uzk_srs_precompute(uint64_t handle, int window_bits);
int uzk_srs_len(uint64_t handle, size_t* n_out);

/* ---- sharded SRS: one MSM over several GPUs from one process ------------------------------------------------------------------
 * north_star / SURVEY.md 8e: "MSM shards by point-chunk across the 8 GPUs of one node".  The bases are cut into n_devices
 * contiguous chunks (chunk i = [i n / N, (i + 1) n / N)), chunk i is copied to the HBM of devices[i] once and stays there; an MSM
 * call runs the chunks side by side (one host thread each, each uploading only its part of the scalars) and folds the N 96-byte
 * partial sums on the host (uzk_g1_fold).  Bases and scalars never move between devices.  devices[] may name an ordinal more
 * than once (several chunks on one GPU: what the single-GPU tests do).  window_bits: -1 no window table, 0 automatic, 4 .. 24.
 * (One process per GPU with the partial sums exchanged by RCCL is the other form of the same split: uzkge_amd/sharded.py,
 * bench.py --gpus N.) */
int uzk_srs_register_sharded(const uzk_g1_affine* points, size_t n, const int* devices, uint32_t n_devices, int window_bits, uint64_t* handle_out);
int uzk_srs_release_sharded(uint64_t handle);
/* sum_i scalars[i] * SRS[i], i < n <= the SRS length (a short vector touches the first chunks only).  partials_out (optional):
 * the n_devices partial sums in chunk order. */
int uzk_msm_g1_sharded(uint64_t handle, const uint64_t* scalars_mont, size_t n, uzk_g1_jac* partials_out, uzk_g1_jac* out);
/* length, number of chunks, their devices (n_chunks entries) and bounds (2 n_chunks entries: lo, hi); every output optional */
int uzk_srs_sharded_info(uint64_t handle, size_t* n_out, uint32_t* n_chunks_out, int* devices_out, size_t* bounds_out);

/* ---- MSM: replaces G1Projective::msm (kzg_poly_commitment.rs:290) ---------------------- */
/* out = sum_{i<n} scalars[i] * SRS[offset + i].  n == 0 -> infinity.  offset + n > len ->
 * UZK_ERR_DEGREE.  Zero scalars and infinity bases contribute the identity. */
int uzk_msm_g1(uint64_t srs_handle, size_t offset, const uint64_t* scalars_mont, size_t n,
               uzk_g1_jac* out);
/* Same with the scalars already resident in device memory (the bench / pipelined path). */
int uzk_msm_g1_device(uint64_t srs_handle, size_t offset, const void* d_scalars_mont, size_t n,
                      uzk_g1_jac* out);
/* `batch` scalar vectors of n elements each (scalars[b*n + i]) against the SAME bases
 * SRS[offset .. offset+n): out[b] = sum_i scalars[b][i] * SRS[offset+i].  One launch sequence for
 * the prover's independent commits (5 wires + 3 selectors, prover.rs:160-192; the 5 chunks of t,
 * helpers.rs:1390); shorter polynomials are zero-padded by the caller. */
int uzk_msm_g1_batch(uint64_t srs_handle, size_t offset, const uint64_t* scalars_mont, size_t n, uint32_t batch,
                     uzk_g1_jac* out);
int uzk_msm_g1_batch_device(uint64_t srs_handle, size_t offset, const void* d_scalars_mont, size_t n,
                            uint32_t batch, uzk_g1_jac* out);
/* The prover's commit closure on its Lagrange branch (uzkge/src/plonk/prover.rs:132-142) in ONE batched MSM: vector b has
 * n scalars at d_scalars + b * stride (device) followed by tail_n "tail" scalars (tail + b * tail_n; host memory unless
 * tail_on_device):
 *   out[b] = sum_{i<n} scalars_b[i] * SRS[offset + i]  +  sum_{j<tail_n} tail_b[j] * SRS[offset + n + j].
 * With the bases registered as  lagrange[0..n) || pcs[0..K) || pcs[zd..zd+K)  and the tail  blinds || -blinds  this is
 * lagrange_pcs.commit(evals) followed by pcs.apply_blind_factors(cm, blinds, zd) (kzg_poly_commitment.rs:299-313): the blind
 * terms ride in the commit's own MSM.  The stride lets the evaluation vectors stay where they are (no gather into a staging
 * array); a device tail is what uzk_fold_blinds_batch_device leaves behind.  n + tail_n <= 2^26. */
int uzk_msm_g1_batch_tail_device(uint64_t srs_handle, size_t offset, const void* d_scalars_mont, size_t stride, size_t n,
                                 uint32_t batch, const void* tail_scalars_mont, uint32_t tail_n, int tail_on_device, uzk_g1_jac* out);
/* One-shot, nothing cached: points and scalars are host arrays of the same length. */
int uzk_msm_g1_raw(const uzk_g1_affine* points, const uint64_t* scalars_mont, size_t n,
                   uzk_g1_jac* out);
/* Host-side fold of partial sums (point-chunk sharded MSM: ranks all-gather their 96-byte
 * partials over RCCL, then every rank folds; EC addition is not an RCCL reduce op). */
int uzk_g1_fold(const uzk_g1_jac* partials, size_t count, uzk_g1_jac* out);
/* Host-side Jacobian -> affine (for comparing results). */
int uzk_g1_to_affine(const uzk_g1_jac* p, uzk_g1_affine* out);

/* ---- G2: the MSM over b_g2_query of a Groth16 prover (ark-groth16's B in G2) ------------------------- */
/* BN254 G2 points over Fq2 = Fq[u] / (u^2 + 1): every coordinate is c0 then c1, each 4 x u64 LE Montgomery words (ark-bn254's
 * Fq2 as it lies in memory).  Affine infinity is all zeros, Jacobian infinity has z = 0. */
typedef struct { uint64_t x[2][4], y[2][4]; } uzk_g2_affine;
typedef struct { uint64_t x[2][4], y[2][4], z[2][4]; } uzk_g2_jac;
/* One call handles up to 2^UZK_MSM_G2_MAX_LOG2 points (point chunks of 2^15 folded inside); beyond: UZK_ERR_DEGREE. */
#define UZK_MSM_G2_MAX_LOG2 20
/* Uploads n affine points to the calling context's device; the handle is process-wide (like an SRS handle) and is used by
 * contexts on that device.  uzk_shutdown releases what is left. */
int uzk_g2_register(const uzk_g2_affine* points, size_t n, uint64_t* handle_out);
int uzk_g2_release(uint64_t handle);
int uzk_g2_len(uint64_t handle, size_t* n_out);
/* out = sum_{i<n} scalars[i] * bases[offset + i].  n == 0 -> infinity.  offset + n > len -> UZK_ERR_DEGREE.  Zero scalars and
 * infinity bases contribute the identity; equal and opposite bases are handled (the reference's b_g2_query has all three). */
int uzk_msm_g2(uint64_t handle, size_t offset, const uint64_t* scalars_mont, size_t n, uzk_g2_jac* out);
/* `batch` scalar vectors (scalars[b*n + i]) against the same bases in one launch sequence: the reveal proofs of one deck. */
int uzk_msm_g2_batch(uint64_t handle, size_t offset, const uint64_t* scalars_mont, size_t n, uint32_t batch, uzk_g2_jac* out);
int uzk_msm_g2_batch_device(uint64_t handle, size_t offset, const void* d_scalars_mont, size_t n, uint32_t batch, uzk_g2_jac* out);
/* The same sums finished on the device: handle, offset, n, batch, UZK_ERR_DEGREE and infinities as uzk_msm_g2_batch_device, but the
 * window sums never come back -- their chunk sums (n > 2^15), the Horner chain over the 32 windows and the affine map are kernels.
 * The results are canonical affine points (fully reduced Montgomery words; infinity all zeros), written to out (host, batch points),
 * to d_out (device, batch points), or to both; both NULL is UZK_ERR_PARAMETER.  Complete when the call returns. */
int uzk_msm_g2_batch_finish(uint64_t handle, size_t offset, const void* d_scalars_mont, size_t n, uint32_t batch, uzk_g2_affine* out, void* d_out);
/* Host-side fold of partial sums and Jacobian -> affine (canonical words), as for G1. */
int uzk_g2_fold(const uzk_g2_jac* partials, size_t count, uzk_g2_jac* out);
int uzk_g2_to_affine(const uzk_g2_jac* p, uzk_g2_affine* out);

/* ---- Groth16: the prover of a reveal proof on a resident key, batched over the proofs of a deck --------------------------------
 * Groth16::<Bn254>::prove (shuffle/src/sdk.rs:288-303) behind one call: the witness map (ark-groth16's
 * LibsnarkReduction::witness_map_from_matrices), the three G1 MSMs, the G2 MSM and the assembly of (A, B, C).  Everything a proof
 * needs is uploaded once by uzk_g16_key_create; per proof the caller passes the full assignment z (z[0] = 1, then the public
 * inputs, then the private witness: n_vars elements) and the two blinding scalars r, s it has drawn.
 *
 * The R1CS matrices A, B, C arrive in CSR: row_ptr[k] has n_constraints + 1 entries (row_ptr[k][0] = 0, non-decreasing), col[k] and
 * val[k] have row_ptr[k][n_constraints] entries (col < n_vars; val: Fr, 4 Montgomery words each); k = 0, 1, 2 for A, B, C.
 * The domain has n = the smallest power of two >= n_constraints + n_inputs points.  The witness map, with g = 5 (Fr::GENERATOR):
 *   a[i] = <A_i, z>, b[i] = <B_i, z>, c[i] = <C_i, z> for i < n_constraints;  a[n_constraints + j] = z[j] for j < n_inputs; zero up to n
 *   a, b, c: inverse transform over the domain, forward transform over the coset g H
 *   t = (a o b - c) / (g^n - 1);  h = the inverse coset transform of t  (n coefficients; h[n - 1] = 0 for a satisfying assignment)
 * An assignment that does not satisfy the constraints is not detected (as in the reference): its proof does not verify.
 *
 * The proof, with the key's fixed terms riding in the MSMs as extra bases:
 *   A  = MSM(a_query || alpha_g1 || delta_g1;      z || 1 || r)
 *   B1 = MSM(b_g1_query || beta_g1 || delta_g1;    z || 1 || s)
 *   B  = MSM(b_g2_query || beta_g2 || delta_g2;    z || 1 || s)          (G2)
 *   K  = MSM(l_query || h_query || delta_g1;       z[n_inputs ..] || h[0 .. n - 1) || -r s)
 *   C  = s A + r B1 + K
 * The host does the two scalar multiplications and the two additions of C and the affine maps; z, a, b, c, h and the scalar rows stay
 * on the device. */
typedef struct {
    uint32_t n_vars;            /* m: variables including the constant one; 1 <= n_inputs <= n_vars, n_vars + 2 <= 2^UZK_MSM_G2_MAX_LOG2 */
    uint32_t n_inputs;          /* l: instance variables including the constant one */
    uint32_t n_constraints;     /* rows of A, B, C; >= 1 */
    uint32_t reserved;
    uint64_t l_query_len;       /* must be n_vars - n_inputs */
    uint64_t h_query_len;       /* must be n - 1 */
    uzk_g1_affine alpha_g1, beta_g1, delta_g1;
    uzk_g2_affine beta_g2, delta_g2;
    const uzk_g1_affine* a_query;       /* n_vars points; infinity is all zeros (the reference's columns hold hundreds) */
    const uzk_g1_affine* b_g1_query;    /* n_vars */
    const uzk_g1_affine* l_query;       /* n_vars - n_inputs */
    const uzk_g1_affine* h_query;       /* n - 1 */
    const uzk_g2_affine* b_g2_query;    /* n_vars */
    const uint64_t* row_ptr[3];
    const uint32_t* col[3];
    const uint64_t* val[3];
} uzk_g16_key_desc;
typedef struct { uzk_g1_affine a; uzk_g2_affine b; uzk_g1_affine c; } uzk_g16_proof;
/* Proofs of one launch sequence at most; a larger batch runs as groups (the rule is below). */
#define UZK_G16_GROUP 128
/* Checks the descriptor on the host (null pointers, 1 <= n_inputs <= n_vars, the two lengths, row pointers, col < n_vars:
 * UZK_ERR_PARAMETER; uzk_domain_supported(n) == 0 or n_vars + 2 > 2^UZK_MSM_G2_MAX_LOG2: UZK_ERR_DEGREE) before the device is touched,
 * then uploads everything to the calling context's device.  The handle is process-wide (like an SRS or G2 handle) and is used by
 * contexts on that device; uzk_shutdown releases what is left.
 * Groups: a batch runs as groups of min(UZK_G16_GROUP, 2^21 / max(n_vars + 2, (n_vars - n_inputs) + n)) proofs, at least one -- the
 * divisor is the longest row a proof has (the scalars of B, of K; the domain is never longer than K's row), so the buffers of a
 * group hold at most 2^21 elements per row kind and each of the three G1 MSMs of a group is one the MSM code admits in one call.
 * The reveal key (n = 8192, n_vars = 4869) runs groups of 128.
 * What is tested how: proofs are compared with a reference at domains up to 2^16 and n_vars up to 2^15 + 3 (groups of 128, 63 and
 * 31; two G2 point chunks).  Every larger shape accepted here (domains up to 2^25, n_vars + 2 up to 2^20) is only PLANNED: its group
 * size and the admission of its MSMs are checked without running a proof (tests/test_gpu_g16_large.py). */
int uzk_g16_key_create(const uzk_g16_key_desc* desc, uint64_t* key_out);
/* The caller makes sure no context still proves with this key. */
int uzk_g16_key_release(uint64_t key);
/* n_vars, n_inputs, n_constraints, the domain size n and the device the key lives on; every output optional (NULL). */
int uzk_g16_key_info(uint64_t key, uint32_t* n_vars_out, uint32_t* n_inputs_out, uint32_t* n_constraints_out, uint64_t* domain_out,
                     int* device_out);
/* The witness map alone: d_z = batch assignments of n_vars elements each (device), d_h = batch x n coefficients of h (device).
 * The result is complete when the call returns. */
int uzk_g16_h_device(uint64_t key, const void* d_z, uint32_t batch, void* d_h);
/* batch proofs: z = batch x n_vars elements, r and s = batch elements each (host), out = batch proofs as affine points in the wire
 * format (Montgomery words, fully reduced; infinity all zeros).  batch == 0 and an assignment with z[0] != 1 are UZK_ERR_PARAMETER. */
int uzk_g16_prove_batch(uint64_t key, const uint64_t* z_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t batch,
                        uzk_g16_proof* out);
/* The same with the assignments already in device memory (a witness produced there); z[0] is not read back. */
int uzk_g16_prove_batch_device(uint64_t key, const void* d_z_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t batch,
                               uzk_g16_proof* out);
/* The same proofs finished on the device: B comes from uzk_msm_g2_batch_finish's kernels, the three G1 sums are uploaded again
 * (288 bytes per proof) and s A, r B1, their sum with K, the affine maps of A and C and the encoding are kernels -- no curve arithmetic
 * on the host.  z_mont is a host array (z_on_device == 0; z[0] must be 1) or a device array (z_on_device != 0), r and s as above.
 *   proofs_out   host, batch proofs in the struct layout: bit for bit what uzk_g16_prove_batch writes
 *   blobs_out    host, batch x UZK_G16_PROOF_BYTES: what uzk_g16_verify_batch reads -- the words a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0,
 *                c.x, c.y, each the canonical integer in 32 big-endian bytes; infinity is all-zero coordinates
 *   d_blobs_out  device, the same bytes, left there
 * Any of the three may be NULL, not all of them (UZK_ERR_PARAMETER).  Complete when the call returns. */
int uzk_g16_prove_batch_finish(uint64_t key, const void* z_mont, int z_on_device, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t batch,
                               uzk_g16_proof* proofs_out, uint8_t* blobs_out, void* d_blobs_out);

/* ---- NTT: replaces EvaluationDomain::{fft, ifft} (field_polynomial.rs:585,595) --------- */
/* The largest transforms this library runs: n = 2^k with k <= UZK_NTT_MAX_LOG2, n = 3 * 2^k with k <= UZK_NTT_MAX_LOG2_MIXED.
 * These are exactly the largest sizes the parity suite compares with the CPU oracle on the whole vector
 * (tests/test_gpu_ntt_large.py: 2^25 is the first four-pass plan); a size is accepted only if its result is checked.
 * (Fr has domains up to 2^28 / 3 * 2^28; the prover of the reference uses n = 2^14 and 6n = 3 * 2^15.) */
#define UZK_NTT_MAX_LOG2 25
#define UZK_NTT_MAX_LOG2_MIXED 22
/* 1 if this library transforms over the size-n domain (n = 2^k, k <= UZK_NTT_MAX_LOG2, or n = 3 * 2^k,
 * k <= UZK_NTT_MAX_LOG2_MIXED), else 0: the shim's FpPolynomial::{evaluation_domain, quotient_evaluation_domain}
 * (field_polynomial.rs:554-567) returns None on 0, which its callers turn into UzkgeError::FFTError. */
int uzk_domain_supported(uint64_t n);
/* group_gen of the size-n domain (5^((r-1)/n)), Montgomery form; answers for every domain Fr has (2^k, 3 * 2^k, k <= 28). */
int uzk_domain_group_gen(uint64_t n, uint64_t out_mont[4]);
/* In-place transform of `n` elements in natural order over <group_gen(n)>.
 * inverse != 0: includes the 1/n scaling.  coset_shift (4 limbs, Montgomery) or NULL:
 * forward: c_j *= shift^j before the transform (coset_fft_with_domain, :589-591);
 * inverse: c_j *= shift^j after the transform -- pass k^-1 (coset_ifft_with_domain, :601-607).
 * The caller zero-pads short inputs (it owns the Vec). */
int uzk_ntt_fr(uint64_t* data, uint64_t n, int inverse, const uint64_t* coset_shift_mont);
/* Device-resident variant: d_in -> d_out (may alias), asynchronous on the library stream
 * unless `sync` != 0. */
int uzk_ntt_fr_device(const void* d_in, void* d_out, uint64_t n, int inverse,
                      const uint64_t* coset_shift_mont, int sync);

/* `batch` independent transforms of the same size over contiguous vectors (the prover's 5 wire +
 * 3 selector iFFTs, prover.rs:160-192, or the ten coset FFTs of t_poly, helpers.rs:256-266, in one
 * launch sequence instead of 8-10). */
int uzk_ntt_fr_batch(uint64_t* data, uint64_t n, uint32_t batch, int inverse, const uint64_t* coset_shift_mont);
int uzk_ntt_fr_batch_device(const void* d_in, void* d_out, uint64_t n, uint32_t batch, int inverse,
                            const uint64_t* coset_shift_mont, int sync);

/* The same with consecutive vectors in_stride / out_stride elements apart (>= n; d_in == d_out needs equal strides): a batch
 * that reads or writes slots of a wider array -- the prover's iFFT results go straight into the 6n-element slots its coset
 * FFTs read (uzkge/src/plonk/prover.rs:160-175 -> helpers.rs:256-266), no copy in between. */
int uzk_ntt_fr_batch_strided_device(const void* d_in, uint64_t in_stride, void* d_out, uint64_t out_stride, uint64_t n,
                                    uint32_t batch, int inverse, const uint64_t* coset_shift_mont, int sync);

/* ---- NTT over G1: EvaluationDomain::{fft, ifft} over Vec<G1Projective> ------------------------------------------------------
 * The elements are curve points (64 B affine, (0,0) = infinity, in and out), the twiddles the powers of uzk_domain_group_gen(n);
 * natural order in and out:
 *   forward  out[k] = sum_i w^(ik) in[i]              inverse  out[i] = (1/n) sum_k w^(-ik) in[k]
 * With M[k] = [tau^k] G (a monomial SRS) and L[i] = [L_i(tau)] G (the Lagrange bases every commit of the round API takes):
 * L = inverse(M), M = forward(L).  The reference ships L for n = 4096, 8192, 16384 only (gen_params/mod.rs:175-177) and cannot
 * derive it; uzk_srs_to_lagrange does, for every n = 2^k up to the bound.  Complete: any input may be infinity, any output too.
 * The largest size is the largest one the parity suite checks on the whole vector (tests/test_gpu_g1_ntt.py), as for the Fr
 * transforms above: that case (two transforms of each direction, 0.36 / 0.40 s each, and four MSMs of 2^20 points by the CPU oracle) takes 4 s of
 * the suite. */
#define UZK_NTT_G1_MAX_LOG2 20
/* 1 if n = 2^k with k <= UZK_NTT_G1_MAX_LOG2, else 0 (3 * 2^k domains are not transformed over G1). */
int uzk_ntt_g1_supported(uint64_t n);
/* Host arrays of n points; `points` and `out` may be the same array.  n = 1 is the identity map. */
int uzk_ntt_g1(const uzk_g1_affine* points, uzk_g1_affine* out, uint64_t n, int inverse);
/* Device arrays (may alias), asynchronous on the calling context's stream unless `sync` != 0. */
int uzk_ntt_g1_device(const void* d_in, void* d_out, uint64_t n, int inverse, int sync);
/* The Lagrange bases of size n from the first n points of a registered (monomial) SRS: inverse transform into memory the new
 * handle owns (released with uzk_srs_release).  n > uzk_srs_len -> UZK_ERR_DEGREE; unsupported n -> UZK_ERR_FFT. */
int uzk_srs_to_lagrange(uint64_t monomial_handle, uint64_t n, uint64_t* lagrange_handle_out);
/* Reads n points of a handle back from `offset` on (what a caller needs to save a derived basis): offset + n > len ->
 * UZK_ERR_DEGREE. */
int uzk_srs_download(uint64_t handle, size_t offset, size_t n, uzk_g1_affine* out);
/* Group operations one transform of size n runs (doublings, additions), counted from its plan: tools/g1_ntt_shape.py. */
int uzk_ntt_g1_plan_info(uint64_t n, int inverse, uint64_t* doublings_out, uint64_t* additions_out);

/* ---- SRS validation: curve check and powers-of-tau fold ----------------------------------------------------------------------
 * uzk_srs_register* copies 64-byte words and trusts them, as the reference does (from_unchecked_bytes, Validate::No,
 * kzg_poly_commitment.rs:228-256).  An off-curve base does not fail an MSM: it runs through the addition formulas of another curve
 * and gives a commitment that looks like any other; a base set that is not [tau^i] G makes commitments that bind to nothing.  These
 * entry points are the check, on the device.  A handle of uzk_srs_register_sharded is not accepted (UZK_ERR_PARAMETER).
 *
 * uzk_srs_check_curve classifies the points P[offset .. offset + count) of a handle; every point falls into exactly one class,
 * checked = infinity + non_canonical + off_curve + good ones.  BN254 G1 has cofactor 1: a point on the curve is in the group, no
 * subgroup check is needed.  count = 0 is an empty report.
 *
 * uzk_srs_fold_powers folds the count - 1 equations P[i + 1] = tau P[i] of a run under random 128-bit weights into two points:
 *   left = sum_{i < count-1} rho_i P[offset+i]      right = sum_{i < count-1} rho_i P[offset+i+1]
 * and the run is a power sequence of tau  <=>  e(right, H) = e(left, [tau] H), except with probability 2^-128 over the seed.
 * Draw the seed AFTER the points are fixed.  The library computes no pairing: the pairing check, whether H and [tau] H are good G2 points,
 * and whether P[0] is the generator the caller expects stay with the caller.  Points at infinity inside a run contribute the
 * identity, as in every MSM here (the curve report is where the caller sees them); run the curve check first -- the fold of a run
 * with off-curve points means nothing.
 *
 * Weights: block j = Keccak-256 (padding byte 0x01, the transcript's sponge) of the 48-byte message seed || "uzksrsv1" || le64(j);
 * rho_2j = digest bytes 0..15, rho_2j+1 = bytes 16..31, little-endian integers < 2^128.  The device expands the seed itself.
 *
 * Errors: unknown handle or one of another device, null pointer, count < 2 for a fold -> UZK_ERR_PARAMETER;
 * offset + count > uzk_srs_len -> UZK_ERR_DEGREE; n not a size of uzk_ntt_g1_supported -> UZK_ERR_FFT. */
typedef struct {
    uint64_t checked;        /* points looked at (= count) */
    uint64_t infinity;       /* encoded (0,0) */
    uint64_t non_canonical;  /* a coordinate, read as a 256-bit integer, >= p */
    uint64_t off_curve;      /* canonical, not (0,0), y^2 != x^3 + 3 */
    uint64_t first_bad;      /* smallest index (relative to the handle, i.e. offset included) of a non-canonical
                                or off-curve point; UINT64_MAX if there is none */
} uzk_srs_curve_report;
int uzk_srs_check_curve(uint64_t handle, size_t offset, size_t count, uzk_srs_curve_report* out);
/* Host only, no device needed: weights first .. first + count - 1 of `seed`, Montgomery form, 4 limbs each (what the device
 * derives for a fold; first + count must not exceed 2^64 - 1). */
int uzk_srs_fold_weights(const uint8_t seed[32], uint64_t first, uint64_t count, uint64_t* out_mont);
/* The run P[offset .. offset + count), count >= 2; left_out / right_out as above. */
int uzk_srs_fold_powers(uint64_t handle, size_t offset, size_t count, const uint8_t seed[32], uzk_g1_jac* left_out,
                        uzk_g1_jac* right_out);
/* The same over M = the forward G1 transform of the first n points of a Lagrange handle (n: uzk_ntt_g1_supported, n >= 2), which
 * must be a power sequence if the handle holds [L_i(tau)] G.  first_out = M[0] = sum_i L_i, which the caller compares with G.
 * n > uzk_srs_len -> UZK_ERR_DEGREE. */
int uzk_srs_fold_powers_lagrange(uint64_t lagrange_handle, uint64_t n, const uint8_t seed[32], uzk_g1_affine* first_out,
                                 uzk_g1_jac* left_out, uzk_g1_jac* right_out);

/* ---- polynomial helpers next to the hot path ------------------------ */
/* out[b] = sum_j coefs[b*n + j] * x^j : FpPolynomial::eval (field_polynomial.rs:198-209) for a batch of
 * polynomials at one point (the prover's 19 + 20 openings at zeta / zeta*omega, prover.rs:246-273). */
int uzk_poly_eval_batch(const uint64_t* coefs, uint64_t n, uint32_t batch, const uint64_t* x_mont, uint64_t* out);
int uzk_poly_eval_batch_device(const void* d_coefs, uint64_t n, uint32_t batch, const uint64_t* x_mont, uint64_t* out);
/* The permutation grand product z_poly (uzkge/src/plonk/helpers.rs:160-220), evaluations only:
 * z[0] = 1, z[i+1] = z[i] * prod_j (w[j*n+i] + beta*k[j]*group[i] + gamma)
 *                         / (w[j*n+i] + beta*k[perm/n]*group[perm%n] + gamma),  perm = perm[j*n+i].
 * w: n_wires*n elements, perm: n_wires*n indices < n_wires*n, group: n elements (omega^i), k: n_wires.
 * A perm value >= n_wires*n is refused (UZK_ERR_PARAMETER, the message names its index) before anything is launched; a zero
 * denominator product is refused too ("a permutation denominator is zero"): the reference's batch_inversion has no value for it. */
int uzk_z_poly(const uint64_t* w, const uint32_t* perm, const uint64_t* group, const uint64_t* k,
               const uint64_t* beta_mont, const uint64_t* gamma_mont, uint32_t n, uint32_t n_wires, uint64_t* z_out);

/* The same on device-resident inputs (w, group: device Fr vectors; perm: device u32; k and the challenges on the
 * host), z written to d_z (n elements, device).  This entry point TRUSTS its caller: d_perm is not read back, and a value
 * >= n_wires*n makes the kernel index past k and group. */
int uzk_z_poly_device(const void* d_w, const uint32_t* d_perm, const void* d_group, const uint64_t* k,
                      const uint64_t* beta_mont, const uint64_t* gamma_mont, uint32_t n, uint32_t n_wires, void* d_z);

/* batch_prove's polynomial work (uzkge/src/poly_commit/pcs.rs:119-135 with div_rem,
 * field_polynomial.rs:519-550): evals_out[k] = p_k(z);  h = sum_k alpha^k (p_k - p_k(z));
 * q = h / (X - z)  (the remainder is zero by construction).
 * d_polys: batch polynomials of n coefficients each (device, zero-padded to the common n);
 * d_q: n elements on the device, q's n - 1 coefficients followed by a zero; evals_out: batch x 4 words
 * (host).  n <= 2^20, batch <= 4096.  The caller commits q (or folds it for the Lagrange path,
 * pcs.rs:137-166) exactly as the reference does. */
int uzk_open_quotient_device(const void* d_polys, uint64_t n, uint32_t batch, const uint64_t* z_mont,
                             const uint64_t* alpha_mont, void* d_q, uint64_t* evals_out);

/* The same on host arrays (polys: batch * n elements; q_out: n elements; evals_out: batch elements). */
int uzk_open_quotient(const uint64_t* polys, uint64_t n, uint32_t batch, const uint64_t* z_mont, const uint64_t* alpha_mont,
                      uint64_t* q_out, uint64_t* evals_out);

/* The fold modulo X^N - 1 in front of every Lagrange-basis commit of a polynomial with len > N coefficients
 * (batch_prove, uzkge/src/poly_commit/pcs.rs:137-156; split_t_and_commit, uzkge/src/plonk/helpers.rs:1366-1383):
 *   blinds_out[i] = -coefs[N + i]  (i < len - N, host memory),
 *   d_out[i] = coefs[i] + coefs[N + i] for i < len - N, coefs[i] for len - N <= i < min(len, N), 0 beyond  (N elements, device).
 * len <= 2N.  The caller continues exactly as the reference: fft(N) of d_out, commit over the Lagrange SRS,
 * apply_blind_factors(blinds, N).  d_out may alias d_coefs. */
int uzk_fold_blinds_device(const void* d_coefs, uint64_t len, uint64_t n_fold, void* d_out, uint64_t* blinds_out);

/* d_out[j] = sum_k scalars[k] * d_polys[k][j] for j < out_len (a polynomial contributes zero beyond lens[k]): the shape of
 * r_poly (uzkge/src/plonk/helpers.rs:681-999, 1030-1090) -- about 43 device-resident polynomials times scalars that the
 * caller builds from the evaluations and challenges exactly as the reference does.  count <= 64; d_out aliases no input.
 * Asynchronous on the library stream (the scalars are copied before the call returns). */
int uzk_poly_lincomb_device(const void* const* d_polys, const uint64_t* lens, const uint64_t* scalars_mont, uint32_t count,
                            void* d_out, uint64_t out_len);
/* hide_polynomial (uzkge/src/plonk/helpers.rs:139-158) on device-resident coefficients (len >= zeroing_degree +
 * hiding_degree, zero-padded by the caller): coefs[i] += blinds[i], coefs[zeroing_degree + i] -= blinds[i].
 * hiding_degree <= 16.  Asynchronous on the library stream. */
int uzk_hide_polynomial_device(void* d_coefs, uint64_t len, const uint64_t* blinds_mont, uint32_t hiding_degree, uint64_t zeroing_degree);

/* ---- batched / pointer-list forms: one launch per prover step instead of one per polynomial ---------------------------- */
/* hide_polynomial (helpers.rs:139-158) for `count` polynomials `stride` elements apart holding len_in coefficients each:
 * as the reference's `resize`, slots [len_in, zeroing_degree + hiding_degree) are written (zeros, then minus the blinds),
 * not read.  blinds: count * hiding_degree elements (host), count * hiding_degree <= 64.  Asynchronous. */
int uzk_hide_polynomial_batch_device(void* d_coefs, uint64_t stride, uint64_t len_in, uint32_t count, const uint64_t* blinds_mont,
                                     uint32_t hiding_degree, uint64_t zeroing_degree);
/* uzk_fold_blinds_device for `batch` <= 16 polynomials (lens[b] coefficients, in_stride apart), results out_stride apart, and
 * the scalars of apply_blind_factors left on the device as the tail of the following commit:
 *   d_tail[b * tail_n + i] = blind_i = -coefs_b[N + i],  d_tail[b * tail_n + tail_n / 2 + i] = -blind_i   (zero padded),
 * so fold -> uzk_ntt_fr_batch_strided_device -> uzk_msm_g1_batch_tail_device(.., d_tail, tail_n, 1, ..) is the tail of
 * batch_prove (pcs.rs:137-166) / split_t_and_commit (helpers.rs:1366-1394) without a host round trip.  blinds_out (optional,
 * host, batch * tail_n / 2 elements): the blinds as the reference's Vec; asking for them synchronises. */
int uzk_fold_blinds_batch_device(const void* d_polys, uint64_t in_stride, const uint64_t* lens, uint64_t n_fold, uint32_t batch,
                                 void* d_out, uint64_t out_stride, void* d_tail, uint32_t tail_n, uint64_t* blinds_out);
/* FpPolynomial::from_coefs trims trailing zeros (field_polynomial.rs:86-90) and the prover branches on the result: t's
 * coefs.len() (helpers.rs:1333), q.degree() (pcs.rs:138).  out_lens[b] = 1 + the highest index < lens[b] with a non-zero
 * coefficient of polynomial b (d_polys + b * stride), 0 for the zero polynomial.  batch <= 16.
 * sync != 0: the values are in out_lens on return.  sync == 0: out_lens must be uzk_host_alloc memory; the stream fills it in
 * order and the caller reads it after its next synchronising call -- a prover that KNOWS the lengths a well-formed proof has
 * (t: 5n + 11 coefficients, q: n + 2) goes on with them and checks at the round's commit that the device agrees, instead of
 * paying a synchronisation for an answer it already has. */
int uzk_poly_trimmed_len_device(const void* d_polys, uint64_t stride, const uint64_t* lens, uint32_t batch, uint64_t* out_lens, int sync);
/* The split of t in split_t_and_commit (helpers.rs:1335-1363); `chunk` is the reference's `n` argument (n_constraints + 2):
 * chunk i < last = t[i chunk .. (i+1) chunk) resized to chunk + 1 with coefs[chunk] += rands[i], coefs[0] -= rands[i-1];
 * the last chunk = t[last chunk .. t_len) (or [-rands[last-1]] if empty) with coefs[0] -= rands[last-1].  Written to
 * d_chunks + i * chunk_stride, zero padded to chunk_stride; lens_out[i] (optional, host) = the reference's coefs.len().
 * n_chunks <= 8.  Asynchronous. */
int uzk_split_t_device(const void* d_t, uint64_t t_len, uint64_t chunk, uint32_t n_chunks, const uint64_t* rands_mont,
                       void* d_chunks, uint64_t chunk_stride, uint64_t* lens_out);
/* out[k] = p_k(points[point_idx[k]]) for `count` device-resident polynomials of lens[k] coefficients: the prover's round 4
 * (prover.rs:246-273: 15 polynomials at zeta, 4 at zeta * omega) in one launch (count <= 64, n_points <= 4, lens <= 2^18;
 * beyond that one call per polynomial). */
int uzk_poly_eval_ptrs_device(const void* const* d_polys, const uint64_t* lens, const uint32_t* point_idx, uint32_t count,
                              const uint64_t* points_mont, uint32_t n_points, uint64_t* out);
/* uzk_open_quotient_device over a pointer list (polynomials of different lengths, wherever they live):
 * q = (sum_k alpha^k p_k) div (X - z) -> d_q: hlen - 1 coefficients (hlen = max lens[k]), zeros up to q_cap >= hlen.
 * evals_out (optional, host, count elements) = p_k(z); without it nothing is evaluated -- the constant batch_prove subtracts
 * (pcs.rs:124-130) only changes the remainder.  The division is queued on the context's stream and the call returns: d_q is
 * complete after the next synchronising call (uzk_sync, a commit, a D2H copy). */
int uzk_open_quotient_ptrs_device(const void* const* d_polys, const uint64_t* lens, uint32_t count, const uint64_t* z_mont,
                                  const uint64_t* alpha_mont, void* d_q, uint64_t q_cap, uint64_t* evals_out);

/* The quotient evaluations of t_poly on the coset k[1]*<g_m> (uzkge/src/plonk/helpers.rs:284-656 with
 * the "shuffle" feature; gate function turbo/mod.rs:193-222): for every point of the m = factor*n
 * domain, the 18 terms (gate, permutation, L1, booleanity, Anemoi round, shuffle/ECC selectors) are
 * combined with the powers of alpha and multiplied by z_h_inv[point % factor] -- the body of the
 * reference's cfg_into_iter!(0..m) loop, one lane per point.  The caller produces the inputs with the
 * coset transforms above (uzk_ntt_fr_batch_device with coset_shift = k[1]) and finishes with the
 * inverse coset transform, exactly as the reference does around that loop.
 * vec[slot]: DEVICE pointers to vectors of m elements (Montgomery form); "next" values (z, w0..w2 at
 * (point + factor) % m) are read from the same vectors. */
enum {
    UZK_TQ_W = 0,               /* 5: wire polynomials w[0..4] */
    UZK_TQ_WSEL = 5,            /* 3: wire selectors w_sel[0..2] */
    UZK_TQ_PI = 8,              /* public-input polynomial */
    UZK_TQ_Z = 9,               /* permutation grand product */
    UZK_TQ_Q = 10,              /* 9: selectors q_coset_evals (turbo/mod.rs:197-210 order) */
    UZK_TQ_S = 19,              /* 5: s_coset_evals */
    UZK_TQ_L1 = 24,
    UZK_TQ_QB = 25,
    UZK_TQ_QPRK = 26,           /* 4: q_prk1..4 */
    UZK_TQ_COSET_QUOTIENT = 30, /* prover_params.coset_quotient */
    UZK_TQ_QPK = 31,            /* 12: q_shuffle_public_key: x_00,x_01,x_10,x_11, y_.., dxy_.. */
    UZK_TQ_QG = 43,             /* 12: q_shuffle_generator, same order */
    UZK_TQ_QECC = 55,
    UZK_TQ_NVEC = 56
};
typedef struct {
    uint32_t n, factor;                 /* constraint-system size, m / n (6, or 16 for n <= 8); factor <= 16 */
    const void* vec[UZK_TQ_NVEC];
    uint64_t alpha[4], beta[4], gamma[4], k[5][4], anemoi_g[4], anemoi_g_inv[4], edwards_a[4];
    uint64_t z_h_inv[16][4];            /* 1 / (k[1]^n * g_m^(n*i) - 1), i < factor (helpers.rs:242-252) */
} uzk_quotient_args;
/* d_out: m elements on the device (must not alias an input).  A circuit built without the "shuffle" feature (zmatchmaking)
 * passes NULL in all 28 slots of UZK_TQ_WSEL, UZK_TQ_QPK, UZK_TQ_QG and UZK_TQ_QECC: terms 12..18 (helpers.rs:437-655,
 * #[cfg(feature = "shuffle")]) are then not evaluated. */
int uzk_t_quotient_device(const uzk_quotient_args* args, void* d_out, int sync);

/* ---- circuits and the five prover rounds ------------------------------------------------------------------------------------
 * prover_with_lagrange (uzkge/src/plonk/prover.rs:88-394) behind the C ABI: the per-circuit data of PlonkProverParams
 * (uzkge/src/plonk/indexer.rs:76-138) lives in HBM as a CIRCUIT, one proof's polynomials in a PROVER (a workspace), and one call
 * per Fiat-Shamir round does everything the reference does between two transcript draws.  The host keeps what is O(1) or
 * protocol: the transcript, the prng (blinds), r_poly's scalars.  Every host language -- the C++ driver tests/cpp/prover_rounds.cpp,
 * the Python driver tools/prover_chain.py, rust/uzkge-glue/gpu_prover.rs -- runs the same tested implementation.
 *
 * Slots of a circuit's polynomials = the quotient kernel's order (UZK_TQ_Q .. UZK_TQ_QECC) minus UZK_TQ_Q.
 * Coset evaluations over the quotient domain (indexer.rs:316-470: q_coset_evals, s_coset_evals, ...) are never uploaded: the
 * library derives them from the coefficient forms with one batched coset FFT (k[1], the 6n domain) -- exact arithmetic, so the
 * bytes are the indexer's, and the ordering of the 6n domain becomes internal to the library (every vector over that domain is
 * produced and consumed here: the proof does not depend on which primitive 6n-th root enumerates it). */
#define UZK_CIRCUIT_SLOTS 46
enum {
    UZK_CS_Q = 0,               /* 9: q_polys */
    UZK_CS_S = 9,               /* 5: s_polys */
    UZK_CS_L1 = 14,             /* l1_coefs */
    UZK_CS_QB = 15,             /* qb_poly */
    UZK_CS_QPRK = 16,           /* 4: q_prk_polys */
    UZK_CS_COSET_QUOTIENT = 20, /* prover_params.coset_quotient = k[1] * g_m^i: pass NULL, the library builds it (= the polynomial X) */
    UZK_CS_QPK = 21,            /* 12: q_shuffle_public_key_polys */
    UZK_CS_QG = 33,             /* 12: q_shuffle_generator_polys */
    UZK_CS_QECC = 45            /* q_ecc_poly */
};
typedef struct {
    uint32_t n;                 /* cs.size(): a power of two, 16 <= n <= 2^UZK_PROVER_MAX_LOG2 */
    uint32_t shuffle;           /* != 0: built with the "shuffle" feature -- all 46 slots; 0: slots 0..20 only (zmatchmaking) */
    uint32_t precompute;        /* window tables over the commit bases (uzk_srs_precompute): 0 none; 1 automatic -- two tables, 8-bit
                                   windows for provers of one proof (shortest chain of dependent additions) and 15-bit windows for
                                   lockstep batches (17 instead of 32 additions per scalar), 50 MiB at n = 2^14; 4 .. 24: one table
                                   of that window width for every prover */
    uint32_t reserved;
    const uzk_g1_affine* lagrange_bases;  /* n points: lagrange_pcs.public_parameter_group_1 (prover.rs:125-130) */
    const uzk_g1_affine* blind_bases;     /* 6 points: pcs.public_parameter_group_1[0..3) || [n..n+3) (apply_blind_factors) */
    const uint32_t* permutation;          /* 5 n entries < 5 n: prover_params.permutation */
    uint64_t k[5][4];                     /* verifier_params.k */
    uint64_t anemoi_g[4], anemoi_g_inv[4], edwards_a[4];
    uint64_t group_gen[4];                /* domain.group_gen of the size-n domain: must equal uzk_domain_group_gen(n), else UZK_ERR_FFT */
    const uint64_t* polys[UZK_CIRCUIT_SLOTS];   /* coefficient forms (host); slots >= 21 are ignored without shuffle; slot 20: NULL
                                                   (a polynomial given there replaces X: the frozen test vectors use a random one) */
    uint64_t poly_lens[UZK_CIRCUIT_SLOTS];      /* coefs.len() <= n (FpPolynomial::from_coefs has trimmed them); 0 = the zero polynomial */
} uzk_circuit_desc;
/* Uploads the circuit, derives the 46 (21) coset tables, registers the commit bases.  The handle is process-wide: provers of
 * every context may use it at the same time. */
int uzk_circuit_create(const uzk_circuit_desc* desc, uint64_t* circuit_out);
/* Replaces `count` polynomials from `first_slot` on (coefficient forms, host; lens[i] <= n) and re-derives their coset tables:
 * what refresh_prover_params_public_key (shuffle/src/gen_params/params.rs:57-129) does to q_shuffle_public_key_polys /
 * _coset_evals once per game -- first_slot = UZK_CS_QPK, count = 12.  Copy on write: a proof in flight (between its round 1 and
 * its round 5) keeps the tables it started with, the next round 1 sees the new ones; nothing is freed under a running kernel. */
int uzk_circuit_update_tables(uint64_t circuit, uint32_t first_slot, uint32_t count, const uint64_t* const* polys, const uint64_t* lens);
/* The per-table loop of refresh_prover_params_public_key (params.rs:88-121) and indexer_with_lagrange (indexer.rs:316-470) as
 * one device call: `count` evaluation vectors over the size-n domain (host, n elements each, evals + i * n)
 *   -> batched iFFT(n) -> batched coset FFT(6n, k[1]) -> batched Lagrange commit of the evaluations,
 * the results installed in slots first_slot .. first_slot + count (as uzk_circuit_update_tables would).  Outputs, each optional
 * (NULL): polys_out = count x n coefficients (zero padded; lens_out[i] = coefs.len() after from_coefs' trimming), coset_out =
 * count x 6n coset evaluations in the library's enumeration of the 6n domain (uzk_domain_group_gen(6 n)), commitments_out =
 * count commitments (lagrange_pcs.commit(evals), no blinds). */
int uzk_circuit_refresh_tables(uint64_t circuit, uint32_t first_slot, uint32_t count, const uint64_t* evals, uint64_t* polys_out,
                               uint64_t* lens_out, uint64_t* coset_out, uzk_g1_jac* commitments_out);
/* The same loop without a circuit -- what indexer_with_lagrange (indexer.rs:316-470) runs once per deck size for its 34 (9)
 * selector / permutation vectors: `count` evaluation vectors (host, n each) -> batched iFFT(n) -> polys_out (count x n, zero padded;
 * lens_out = coefs.len()), [coset_out: batched coset FFT over the 6n domain with shift k1: count x 6n], [commitments_out: one batched
 * MSM of the evaluations over the first n bases of `lagrange_srs` (uzk_srs_register)].  Every output is optional. */
int uzk_preprocess_tables(uint64_t lagrange_srs, uint32_t n, uint32_t count, const uint64_t* evals, const uint64_t* k1_mont, uint64_t* polys_out,
                          uint64_t* lens_out, uint64_t* coset_out, uzk_g1_jac* commitments_out);
/* Device address and coefficient count of a slot's polynomial (which = 0; n elements allocated) or coset table (which = 1; 6n
 * elements) as of now -- tests and diagnostics. */
int uzk_circuit_table(uint64_t circuit, uint32_t slot, int which, const void** d_out, uint64_t* len_out);
/* Forgets the handle.  Tables, commit bases and window tables are freed with the last proof that still holds them: a proof in
 * flight (between its round 1 and its round 5) finishes with what it started with. */
int uzk_circuit_release(uint64_t circuit);
/* n, the evaluations round 4 writes per proof (15, or 19 for a shuffle circuit), the r_poly scalars round 5 reads per proof
 * (19 or 43) and the device the circuit lives on; every output optional (NULL). */
int uzk_circuit_info(uint64_t circuit, uint32_t* n_out, uint32_t* evals_per_proof_out, uint32_t* r_scalars_per_proof_out, int* device_out);

/* A prover = the device buffers of `batch` proofs over circuits of size n that advance in lockstep (a server with several
 * witnesses of one circuit waiting runs them as ONE sequence of wider launches -- commits of 8 x batch vectors, transforms of
 * 10 x batch).  Use a prover from one thread at a time.  It lives on the calling context's device; all five rounds of a proof
 * must come from the context that ran its round 1 (else UZK_ERR_PARAMETER: they are ordered on that context's stream).
 *
 * batch = 1 is the reference's shape -- prover_with_lagrange proves one proof per call from whatever thread the application
 * runs (prover.rs:88-100; shuffle/src/sdk.rs:196-214) -- and at n = 2^14 one proof leaves most of the chip idle.  Provers of
 * one proof are therefore SHARED by default: when several threads stand at the same round of proofs over the same circuit, the
 * library runs their calls as one lockstep launch sequence on a pooled workspace with its own stream and hands each caller its
 * own outputs -- bit for bit what the call alone would have returned (tests/test_gpu_coalesce.py).  No new API: each thread
 * keeps calling uzk_prove_round1..5 on its own prover, from any context.  A thread whose prover is the only idle one never
 * waits; see uzk_coalesce_config.
 *
 * Device memory: a lane (the buffers of one proof) takes about 150 x n x 32 bytes -- 79 MB at n = 2^14, 315 MB at 2^16, 5 GB at
 * 2^20.  A prover of `batch` proofs holds `batch` lanes.  A shared prover holds one lane of its own (made on first need); the
 * pooled workspaces hold max_lanes lanes each and at most `groups` of them exist per (n, device): 8 x 4 x 79 MB = 2.5 GB at
 * n = 2^14 with the defaults.  Sharing only pays where one proof leaves the chip idle, so provers of n > UZK_SHARED_MAX_N
 * (2^16) are never shared: they own their single lane as before -- the pool cannot grow past 8 x 4 x 315 MB = 10 GB. */
#define UZK_SHARED_MAX_N (1u << 16)
/* The largest circuit uzk_circuit_create and uzk_prover_create[_private] accept: n = 2^k, 4 <= k <= UZK_PROVER_MAX_LOG2.  The bound
 * is the largest size at which the suite makes a whole proof and holds it to the oracle (tests/test_gpu_rounds_large.py); a
 * larger n is refused at creation, never in a later round. */
#define UZK_PROVER_MAX_LOG2 20
int uzk_prover_create(uint32_t n, uint32_t batch, uint64_t* prover_out);
/* The same, but the prover owns its lanes whatever `batch` and the sharing configuration are: its proofs run on the calling
 * context's stream, alone, and uzk_prover_buffer can show its buffers (tests, diagnostics, latency measurements). */
int uzk_prover_create_private(uint32_t n, uint32_t batch, uint64_t* prover_out);
int uzk_prover_destroy(uint64_t prover);
/* How provers of one proof made FROM NOW ON are shared (process-wide; existing provers keep their kind):
 *   max_lanes          most proofs per lockstep launch (default 8; <= 64).  0 or 1: off -- such provers own their lane, as
 *                      provers with batch >= 2 and those of uzk_prover_create_private always do
 *   gather_wait_us     how long the first caller of a round 1 waits for company (0 = the default, 2000); it does not wait at all
 *                      unless another shared prover of its size and device is about to start a proof too (one that finished a
 *                      proof within the last 5 ms, or stands in the last round of one)
 *   straggler_wait_us  how long the callers of rounds 2..5 wait for a member of their group before its proof is moved to a
 *                      workspace of its own and the rest go on (0 = the default, 20000)
 *   groups             the provers at work are spread over this many launch sequences side by side (0 = the default, 4: measured
 *                      best at n = 2^14 -- four streams of B proofs each beat one of 4 B): a group takes at most
 *                      ceil(provers at work / groups) proofs; up to three provers keep a stream each and are never merged,
 *                      from four on nobody is left alone (four provers run as 2 + 2, five as 3 + 2, seven as 3 + 2 + 2).
 *                      At most four of the library's own streams are busy on a device whatever `groups` is: the compute front
 *                      end has four pipes (a fifth busy queue shares one: profiles/r05_gaps_lockstep_5x8.txt) */
int uzk_coalesce_config(uint32_t max_lanes, uint32_t gather_wait_us, uint32_t straggler_wait_us, uint32_t groups);
/* What sharing has done since the last uzk_coalesce_config or the last reset (out == NULL resets the counters): out[0] shared rounds run, out[1] round calls they served (out[1] /
 * out[0] = proofs per launch sequence), out[2] the most calls one round served, out[3] proofs moved to a workspace of their own
 * because their caller stayed away, out[4] groups formed at a round 1, out[5] / out[6] the average host time in microseconds
 * between the end of a group's round and the start of its next (its callers wake, take their results and come back with the next
 * challenges: the price of keeping the one-proof API), out[7] / out[4] the average time in microseconds a group stayed open before
 * its first round, out[8 + i] how many groups started with i + 1 callers (the last entry: 8 or more). */
int uzk_coalesce_stats(uint64_t out[16]);
/* Per-proof arrays below are [batch][...]: element b of every input / output belongs to proof b.
 *
 * Round 1 (prover.rs:151-192): PI polynomial, wire and wire-selector polynomials: iFFT(n), hide_polynomial, commit with blinds.
 *   witness   batch x 5 n: cs.extend_witness(w) (wire-major).          wsel  batch x 3 n: cs.compute_witness_selectors(), or NULL
 *   inputs_on_device != 0: witness / wsel are device addresses (a witness produced on the device); host memory of
 *     uzk_host_alloc is uploaded asynchronously, other host memory synchronously
 *   pi_index  pi_count constraint indices (verifier_params.public_vars_constraint_indices), shared by the batch;
 *   pi_value  batch x pi_count online values (helpers.rs:111-131; a repeated index takes its first value, as find_position does)
 *   hiding    5 (+3 with wsel) hiding degrees <= 3: cs.get_hiding_degree(i), then 2 per wire selector (prover.rs:186)
 *   blinds    batch x (5 or 8) x 3 elements: the draws of hide_polynomial in the reference's order, unused third slots zero
 *   cm_out    batch x (5 or 8) commitments: cm_w_vec, then cm_w_sel_vec
 * Takes the circuit's CURRENT tables for the whole proof. */
int uzk_prove_round1(uint64_t prover, uint64_t circuit, const void* witness, const void* wsel, int inputs_on_device,
                     const uint32_t* pi_index, const uint64_t* pi_value, uint32_t pi_count, const uint32_t* hiding,
                     const uint64_t* blinds, uzk_g1_jac* cm_out);
/* Round 2 (prover.rs:194-209): z_poly, iFFT, hide with 3 blinds, commit.  beta, gamma: batch x 4 limbs; blinds_z: batch x 3. */
int uzk_prove_round2(uint64_t prover, const uint64_t* beta, const uint64_t* gamma, const uint64_t* blinds_z, uzk_g1_jac* cm_z_out);
/* Round 3 (prover.rs:211-239): t_poly (helpers.rs:223-678) and split_t_and_commit with n_constraints + 2 (helpers.rs:1323-1408).
 * alpha: batch x 4 limbs; t_rands: batch x 5 (one draw per chunk, chunk order); cm_t_out: batch x 5.
 * from_coefs trims t and the trimmed length drives the split: the library goes on with the length a satisfied circuit gives
 * (5 n - 2 + the wires' hiding degrees), measures the real one on the device meanwhile and redoes the split if they differ.
 * UZK_ERR_COMMITMENT: t is longer than 5 (n + 2) + 1 coefficients (the witness does not satisfy the circuit; the reference
 * indexes past its n + 3 SRS powers in apply_blind_factors and aborts there) or a chunk is shorter than n. */
int uzk_prove_round3(uint64_t prover, const uint64_t* alpha, const uint64_t* t_rands, uzk_g1_jac* cm_t_out);
/* Round 4 (prover.rs:241-273): the opening evaluations, in the reference's order of computation:
 *   w_polys_eval_zeta (5), s_polys_eval_zeta (4), prk_3, prk_4, z_eval_zeta_omega, w_polys_eval_zeta_omega (3)
 *   and, for a shuffle circuit, q_ecc_poly_eval_zeta, w_sel_polys_eval_zeta (3):  15 or 19 elements per proof.
 * zeta: batch x 4 limbs; zeta * omega is formed here.  evals_cap: the elements evals_out can hold (>= batch x 15 or 19:
 * uzk_circuit_info; less is UZK_ERR_PARAMETER, nothing is written past it). */
int uzk_prove_round4(uint64_t prover, const uint64_t* zeta, uint64_t* evals_out, size_t evals_cap);
/* Round 5 (prover.rs:296-372): r(X) = sum_k r_scalars[k] * p_k over (in this order) q_polys (9), z, s_polys[4], qb, q_prk1,
 * q_prk2, [q_shuffle_public_key (12), q_shuffle_generator (12)], t chunks (5): 19 or 43 scalars per proof, which the caller gets
 * from the reference's r_poly_or_comm (helpers.rs:681-1002); then both batch_prove calls (pcs.rs:107-168) with their transcript
 * challenges alpha_zeta / alpha_zeta_omega: quotient, fold, FFT(n), Lagrange commit, blind factors.
 * r_count: the elements r_scalars holds -- exactly batch x 19 or 43 (uzk_circuit_info), else UZK_ERR_PARAMETER.
 * openings_out: batch x 2 (opening_witness_zeta, opening_witness_zeta_omega).  Ends the proof: the circuit tables are released. */
int uzk_prove_round5(uint64_t prover, const uint64_t* r_scalars, size_t r_count, const uint64_t* alpha_zeta, const uint64_t* alpha_zeta_omega,
                     uzk_g1_jac* openings_out);
/* Device address and element count (per proof: proof b's part starts b * elems_out elements in) of a prover buffer -- tests
 * (provers that own their lanes only: batch >= 2, or uzk_prover_create_private):
 *   0 evals (10 n: w0..4, w_sel0..2, pi, z)  1 coefs (10 x 6n slots, same order)  2 coset evaluations (10 x 6n)
 *   3 quotient evaluations (6n)  4 t (6n)  5 t chunks (5 x (n + 8))  6 folded (5 n)  7 tails (5 x 6)
 *   8 opening quotients (2 x (n + 8))  9 r (n + 8).
 * Without wire selectors the slot order of 0..2 is w0..4, pi, z (7 slots used). */
int uzk_prover_buffer(uint64_t prover, int which, void** d_out, uint64_t* elems_out);

/* ---- batch verification: M proofs folded into one pairing check ------------------------------------------------------------------
 * The reference's verifier (uzkge/src/plonk/verifier.rs:17-164) ends in  e(left, [tau] G2) = e(right, G2)  with left and right
 * sums of (commitment, scalar) products (batch_verify_diff_points, kzg_poly_commitment.rs:373-422).  With one weight rho_i per
 * proof, M such equations collapse into ONE:
 *     e(L, [tau] G2) = e(R, G2),      L = sum_i rho_i left_i,      R = sum_i rho_i right_i,
 * which holds for weights nobody could predict only if every proof's own equation does.  Everything in front of the two pairings
 * is data-parallel over proofs and runs on the device: decoding and checking the proof bytes, the M Keccak transcripts, the
 * verifier scalars, and two MSMs (R over 16 M + 45 points, L over 2 M).  The commitments of the key are shared by the batch:
 * their scalars are summed in Fr and each enters the MSM once.  The pairing stays with the caller (arkworks'
 * Bn254::multi_pairing): the library computes no pairing. */
#define UZK_VERIFY_MAX_BATCH 4096
#define UZK_VERIFY_MAX_PI 1024
/* What PlonkVerifierParams (indexer.rs) carries, in the wire forms above: points in Montgomery form with (0,0) as infinity,
 * scalars as 4 Montgomery words. */
typedef struct {
    uint32_t cs_size;                     /* verifier_params.cs_size: a power of two */
    uint32_t n_pi;                        /* public inputs per proof (public_vars_constraint_indices.len()), <= UZK_VERIFY_MAX_PI */
    uint32_t shuffle;                     /* as in uzk_circuit_desc.  0: cm_q_ecc, cm_shuffle_public_key and cm_shuffle_generator are
                                             ignored, a proof has 1312 bytes and r(X) 19 scalars; else 1632 bytes and 43 */
    uint32_t transcript_prefix_len;       /* <= 256, a multiple of 8 (the transcript of utils/transcript.rs holds 32-byte slots) */
    const uint8_t* transcript_prefix;     /* the caller's transcript bytes in front of transcript_init_plonk; zshuffle: the label
                                             "Plonk shuffle Proof" left-padded to 32 bytes, then n_cards as a 32-byte big-endian word */
    const uint64_t* pi_root_powers;       /* n_pi elements: verifier_params.public_vars_constraint_indices as powers of the root */
    const uint64_t* pi_lagrange;          /* n_pi elements: verifier_params.lagrange_constants */
    uzk_g1_affine cm_q[9], cm_s[5], cm_qb, cm_prk[4], cm_q_ecc, cm_shuffle_public_key[12], cm_shuffle_generator[12];
    uzk_g1_affine g1_0;                   /* the SRS's first point: the base of the value term */
    uint64_t k[5][4], anemoi_g[4], anemoi_g_inv[4], edwards_a[4], root[4];
} uzk_vk_desc;
/* Makes the key resident on the calling context's device and absorbs the prefix and the key's part of transcript_init_plonk
 * ("PLONK", cs_size, r, cm_q, cm_s, root, k: plonk/transcript.rs:9-31) into a cached Keccak sponge state -- the same for every
 * proof under this key.  The handle is process-wide. */
int uzk_vk_create(const uzk_vk_desc* desc, uint64_t* vk_out);
/* No fold over the key may still be running. */
int uzk_vk_release(uint64_t vk);
/* cs_size, public inputs per proof, bytes per proof (1632 or 1312) and the device the key lives on; every output optional. */
int uzk_vk_info(uint64_t vk, uint32_t* cs_size_out, uint32_t* n_pi_out, uint32_t* proof_bytes_out, int* device_out);
/* Replaces cm_shuffle_public_key once per game (the counterpart of uzk_circuit_refresh_tables).  These commitments are not part
 * of the transcript: the cached sponge state stays valid.  No fold over the key may still be running (on any context): a fold reads
 * the commitments this call overwrites.  UZK_ERR_PARAMETER for a key made with shuffle == 0. */
int uzk_vk_set_public_key(uint64_t vk, const uzk_g1_affine pk[12]);
/* proofs       m blobs in PlonkProof::to_bytes_be's layout (indexer.rs:539-590): 1632 (1312) bytes of big-endian canonical words
 * pi_mont      m x n_pi public inputs
 * weights_mont m elements of Fr drawn by the CALLER after it has seen the proofs (128 random bits suffice; any element is
 *              accepted).  NULL only with m == 1: weight 1.  NULL with m > 1 is UZK_ERR_PARAMETER -- unweighted sums let errors cancel
 * status_out   m bytes: 0 = decoded and folded; 1 = a word is not canonical (a coordinate >= p, a scalar >= r); 2 = a point is
 *              not on y^2 = x^3 + 3.  A proof with a nonzero status contributes NOTHING to either sum; the call still returns UZK_OK
 *              and the caller decides what a bad proof means.  Zeros are the point at infinity, as in to_transcript_bytes
 * challenges_out  optional, m x 7 elements: beta, gamma, alpha, zeta, u, and the challenges of PolyComScheme::batch at zeta
 *              and at zeta omega (undefined for a proof with a nonzero status)
 * m == 0: two points at infinity.  m > UZK_VERIFY_MAX_BATCH: UZK_ERR_PARAMETER.
 * With m == 1 and weight 1, left_out and right_out are left_first and right_first of batch_verify_diff_points as group elements. */
int uzk_verify_fold(uint64_t vk, const uint8_t* proofs, const uint64_t* pi_mont, uint32_t m, const uint64_t* weights_mont,
                    uzk_g1_jac* left_out, uzk_g1_jac* right_out, uint8_t* status_out, uint64_t* challenges_out);

/* ---- batch Groth16 verification: M reveal proofs folded into one pairing check -----------------------------------------------------
 * A Groth16 proof (A, B, C) with public inputs x_1 .. x_(l-1) (x_0 = 1) is valid iff
 *     e(A, B) = e(alpha, beta) e(X, gamma) e(C, delta),      X = sum_j x_j IC_j      (Groth16Verifier.sol verifyProof)
 * With one weight rho_i per proof, M such equations collapse into ONE product of M + 3 Miller loops and one final exponentiation:
 *     prod_i e(rho_i A_i, B_i) . e(-(sum rho) alpha, beta) . e(-sum rho_i X_i, gamma) . e(-sum rho_i C_i, delta) = 1,
 *     sum rho_i X_i = (sum rho) IC_0 + sum_j (sum_i rho_i x_ij) IC_j.
 * Everything in front of the pairings runs on the device: decoding and checking the proof bytes, the subgroup check of B, the M
 * scalar multiplications rho_i A_i (normalised to affine), the l dot products in Fr and two MSMs (X over the key's l points, C over
 * the M fresh ones).  uzk_g16_verify_fold stops there and hands the G1 arguments to the caller; uzk_g16_verify_batch (below) goes on
 * to the pairing product on the device and returns the verdict. */
#define UZK_G16_VERIFY_MAX_BATCH 4096
#define UZK_G16_VERIFY_MAX_INPUTS 1024
#define UZK_G16_PROOF_BYTES 256
typedef struct {
    uint32_t n_inputs;                 /* l, the constant one included; 1 <= l <= UZK_G16_VERIFY_MAX_INPUTS */
    uint32_t reserved;
    uzk_g1_affine alpha_g1;
    uzk_g2_affine beta_g2, gamma_g2, delta_g2;   /* the caller's side of the pairing; not used on the device */
    const uzk_g1_affine* gamma_abc_g1; /* l points; infinity = all zeros */
} uzk_g16_vk_desc;
/* Checks the descriptor on the host (null pointers, n_inputs: UZK_ERR_PARAMETER) before the device is touched, then makes alpha_g1 and
 * gamma_abc_g1 resident on the calling context's device.  The handle is process-wide; uzk_shutdown releases what is left. */
int uzk_g16_vk_create(const uzk_g16_vk_desc* desc, uint64_t* vk_out);
/* No fold over the key may still be running. */
int uzk_g16_vk_release(uint64_t vk);
/* l and the device the key lives on; every output optional. */
int uzk_g16_vk_info(uint64_t vk, uint32_t* n_inputs_out, int* device_out);
/* proofs       m blobs of UZK_G16_PROOF_BYTES: eight 32-byte big-endian words in the EVM order a.x, a.y, b.x.c1, b.x.c0, b.y.c1,
 *              b.y.c0, c.x, c.y (shuffle/src/sdk.rs:306-319); all-zero coordinates are the point at infinity
 * public_mont  m x (l - 1) elements of Fr; the leading one is implied
 * weights_mont m elements of Fr drawn by the CALLER after it has seen the proofs (128 random bits suffice; any element is
 *              accepted).  NULL only with m == 1: weight 1.  NULL with m > 1 is UZK_ERR_PARAMETER -- unweighted sums let errors cancel
 * status_out   m bytes, the first check that fails: 0 = decoded and folded; 1 = a coordinate word is >= p; 2 = A or C is not on
 *              y^2 = x^3 + 3, or B is not on the twist; 3 = B is on the twist but [r] B != O (the subgroup check of EIP-197's
 *              precompile and of ark's Validate::Yes).  A proof with a nonzero status contributes NOTHING to any sum, its a_out and
 *              b_out are zeros; the call still returns UZK_OK and the caller decides what a bad proof means
 * a_out        m points: rho_i A_i, canonical affine words
 * b_out        m points: B_i in the wire form of uzk_g2_affine
 * alpha_out = (sum rho) alpha, x_out = sum rho_i X_i, c_out = sum rho_i C_i, the sums over the proofs with status 0.
 * m == 0: three points at infinity.  m > UZK_G16_VERIFY_MAX_BATCH: UZK_ERR_PARAMETER.
 * With m == 1 and weight 1 the three sums are alpha, X and C themselves. */
int uzk_g16_verify_fold(uint64_t vk, const uint8_t* proofs, const uint64_t* public_mont, uint32_t m, const uint64_t* weights_mont,
                        uzk_g1_affine* a_out, uzk_g2_affine* b_out, uzk_g1_jac* alpha_out, uzk_g1_jac* x_out, uzk_g1_jac* c_out,
                        uint8_t* status_out);

/* ---- the pairing product: prod_i e(P_i, Q_i) on the device --------------------------------------------------------------------------
 * The optimal ate pairing of BN254: one Miller loop per pair (independent chains, one pair per group of eight lanes), the values
 * multiplied down a tree, one final exponentiation by (p^12 - 1) / r EXACTLY -- gt_out is the element arkworks' Bn254::multi_pairing
 * and the test oracle return, bit for bit, not a power of it.
 * uzk_gt       sum_k (c[k][0] + c[k][1] u) w^k with u^2 = -1, w^6 = 9 + u; Montgomery words, fully reduced
 * p, q         n points each, canonical Montgomery words; all zeros is the point at infinity, and a pair with either point at infinity
 *              contributes 1.  Every coordinate is checked against p, every P against y^2 = x^3 + 3, every Q against the twist
 *              y^2 = x^3 + 3 / (9 + u): a failure is UZK_ERR_PARAMETER and uzk_last_error names the first bad pair.  Membership of Q in
 *              the subgroup of order r is NOT checked here: it is the caller's business (uzk_g16_verify_batch has it from the fold's
 *              status 3; key material is checked when the key is made).
 * gt_out       optional;  is_one_out  1 iff the product is 1.
 * n == 0: the empty product, 1.  n > UZK_PAIRING_MAX_PAIRS or a null pointer: UZK_ERR_PARAMETER, before the device is touched. */
#define UZK_PAIRING_MAX_PAIRS 4099            /* UZK_G16_VERIFY_MAX_BATCH + 3 */
typedef struct { uint64_t c[6][2][4]; } uzk_gt;
int uzk_pairing_product(const uzk_g1_affine* p, const uzk_g2_affine* q, uint32_t n, uzk_gt* gt_out, int* is_one_out);
/* uzk_g16_verify_fold to the end: the fold's kernels, the three sums brought to affine and negated on the device, then the product
 *     prod_i e(rho_i A_i, B_i) . e(-(sum rho) alpha, g2[0]) . e(-sum rho_i X_i, g2[1]) . e(-sum rho_i C_i, g2[2])
 * with rho_i A_i and B_i taken from the fold's workspace -- they never visit the host.  Arguments and status rules are those of
 * uzk_g16_verify_fold; g2 = beta, gamma, delta of the verifying key (a call argument, so that uzk_g16_vk_desc stays what it is; a point
 * of g2 that is not a canonical point of the twist is UZK_ERR_PARAMETER).
 * accepted_out  1 iff every status is 0 and the product is 1.  A proof with a nonzero status makes the verdict 0; its status byte says
 *               why.  m == 0 is accepted (the empty product), status_out may then be NULL. */
int uzk_g16_verify_batch(uint64_t vk, const uint8_t* proofs, const uint64_t* public_mont, uint32_t m, const uint64_t* weights_mont,
                         const uzk_g2_affine g2[3], uint8_t* status_out, int* accepted_out);

/* ---- Baby Jubjub: the curve the cards live on, and the Chaum-Pedersen reveal proofs over it ------------------------------------------
 * zshuffle's cards and keys are points of the twisted Edwards curve x^2 + y^2 = 1 + d x^2 y^2 over BN254's scalar field
 * (ark_ed_on_bn254: a = 1, d = 168696 / 168700, identity (0, 1), cofactor 8, prime subgroup of order
 * L = 2736030358979909402780800718157159386076813972158567259200215660948447373041, generator as in EdOnBN254.sol).  The six public
 * signals of a Groth16 reveal proof are three of its points -- masked.e1, reveal = sk e1, pk = sk G -- and the plain reveal path
 * (shuffle/src/reveal.rs over uzkge/src/chaum_pedersen/dl.rs; ChaumPedersenDLVerifier.sol) proves the same statement with a
 * Chaum-Pedersen DL proof, 52 per player per deck.  Batches run one lane per item (per equation for the verifier).
 *   point      two elements of Fr, x then y, in EXACTLY the element encoding uzk_g16_verify_fold takes for its public signals
 *              (4 Montgomery words each).  Affine; the identity is (0, 1) as in arkworks (the contract's (0, 0) is not a point here)
 *   scalar     a 256-bit integer, 4 little-endian 64-bit words, NOT in Montgomery form and not reduced: an integer multiple is
 *              defined on the whole curve
 *   statement  six elements e1.x, e1.y, reveal.x, reveal.y, pk.x, pk.y: ONE buffer of m x 6 elements serves both
 *              uzk_g16_verify_fold / uzk_g16_verify_batch (as public_mont, l = 7) and uzk_cp_reveal_verify_batch
 *   proof      ChaumPedersenDLProof::to_uncompress: UZK_CP_PROOF_BYTES, the 32-byte big-endian words a.x a.y b.x b.y r
 * Calls that compute with their points (mul, sum, unmask, prove) refuse a coordinate that is not below q with UZK_ERR_PARAMETER
 * before the device is touched; the two checking calls report it as status 1.  A batch of 0 is UZK_ERR_PARAMETER. */
#define UZK_ED_MAX_BATCH 1048576
#define UZK_ED_MAX_ROWS 1024
#define UZK_CP_MAX_BATCH 65536
#define UZK_CP_PROOF_BYTES 160
/* status_out: n bytes, the first that applies: 1 a coordinate word >= q; 2 off the curve; 3 [L] P != identity; 0 otherwise. */
int uzk_ed_check_points(const uint64_t* points_mont, size_t n, uint8_t* status_out);
/* out_i = s_i P_i, canonical affine words.  point_stride 1: n points; 0: points_mont holds one base shared by every item. */
int uzk_ed_mul_batch(const uint64_t* points_mont, size_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_mont);
/* out_j = sum_k rows[k n + j] over k rows of n points (aggregateKeys: n = 1, one key per row). */
int uzk_ed_sum_batch(const uint64_t* rows_mont, uint32_t k, uint32_t n, uint64_t* out_mont);
/* out_j = e2_j - sum_k reveals[k n + j]: the cards of n masked cards from the reveals of k players (shuffle/src/reveal.rs unmask). */
int uzk_ed_unmask_batch(const uint64_t* e2_mont, const uint64_t* reveals_mont, uint32_t k, uint32_t n, uint64_t* out_mont);
/* One player's reveals of m masked cards: reveal_i = sk e1_i, pk = sk G and the proof (a_i = omega_i e1_i, b_i = omega_i G,
 * c_i = Keccak-256(pad32("Revealing") | pad32("DL") | e1_i, G, reveal_i, pk, a_i, b_i as big-endian words) mod L,
 * r_i = omega_i + c_i sk mod L).  sk: one scalar below L; omegas: m scalars drawn by the CALLER (the library has no random number
 * generator); e1: m points of the prime subgroup (uzk_ed_check_points says whether they are).
 * reveal_out: m points; pk_out: one point; proofs_out: m blobs. */
int uzk_cp_reveal_prove_batch(const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* omegas, uint32_t m, uint64_t* reveal_out, uint64_t* pk_out,
                              uint8_t* proofs_out);
/* verdict_out     m bytes, the first that applies: 1 a statement or proof coordinate >= q; 2 a point off the curve; 3 a point outside
 *                 the prime subgroup; 4 r e1 != a + c reveal; 5 r G != b + c pk; 0 accepted.  r is taken as any 256-bit integer (the
 *                 reference reduces it mod L; on subgroup points the results agree).  The call returns UZK_OK unless it is itself
 *                 malformed: the caller reads the verdicts
 * challenges_out  optional, m x 4 words: c_i as plain integers below L (undefined for a verdict of 1) */
int uzk_cp_reveal_verify_batch(const uint64_t* statements_mont, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, uint64_t* challenges_out);

/* -- masking a card and the remask of a shuffle (shuffle/src/mask.rs; uzkge/src/shuffle/remark.rs) --
 * A masked card is e1 = r G, e2 = card + r pk under the joint key pk, with a Chaum-Pedersen DL proof over the parameters g = G, h = pk
 * and the statement (e1, e2 - card): a_i = omega_i G, b_i = omega_i pk,
 * c_i = Keccak-256(pad32("Masking") | pad32("DL") | G, pk, e1_i, e2_i - card_i, a_i, b_i as big-endian words) mod L,
 * r'_i = omega_i + c_i r_i mod L; the blob is the same UZK_CP_PROOF_BYTES layout.  A shuffle re-randomises every card by
 * UZK_REMARK_ITERATIONS signed additions from two tables  T_P[i][j] = (j + 1) 16^i P  (i < 84, j < 4; P = G for e1, P = pk for e2):
 *   digit     one byte per (card, iteration): bits 0 and 1 give j = bit0 + 2 bit1, bit 2 set adds T[i][j], clear subtracts it; bits
 *             3 .. 7 must be 0.  Equivalent scalar: rho = sum_i +-(j_i + 1) 16^i, and the remasked card is (e1 + rho G, e2 + rho pk)
 *   trace     the affine (c2.x, c2.y, c1.x, c1.y) after every step, c1 from e1 and c2 from e2 (RemarkTrace::intermediate_values: the
 *             witness of the shuffle circuit's remark gates); entry 83 is the remasked card; the identity is (0, 1)
 *   tables    x, y, d x y of every entry, [84][4][3] elements: what compute_shuffle_public_key_selectors /
 *             load_shuffle_remark_parameters put into the circuit; uzk_shuffle_circuit_create / _set_key (below) lay them out over
 *             the size-n domain
 * The computing calls (key_create, remark_batch, mask_prove) refuse a coordinate that is not below q, a batch of 0 or above the
 * maximum, a perm that is no permutation, a digit above 7 and an unknown key with UZK_ERR_PARAMETER before the device is touched;
 * they check neither the curve nor the subgroup (uzk_ed_check_points does; off the curve the outputs are unspecified).  The library
 * draws no randomness: digits, rs, omegas and perm come from the caller. */
#define UZK_REMARK_ITERATIONS 84
/* Builds T_pk on the current context's device and keeps it until the key is released (once per game). */
int uzk_remark_key_create(const uint64_t* pk_mont, uint64_t* key_out);
int uzk_remark_key_release(uint64_t key);
/* Either output optional: [84][4][3] elements (x, y, d x y) of T_pk / T_G. */
int uzk_remark_key_tables(uint64_t key, uint64_t* pk_tables_out, uint64_t* gen_tables_out);
/* digits: n x 84 bytes; perm: n entries, a permutation of 0 .. n-1 (out[i] = remasked[perm[i]], the row convention of Permutation),
 * or NULL for the identity; trace_out optional: n x 84 x 4 elements in INPUT card order; e1_out / e2_out: n points in OUTPUT order. */
int uzk_remark_batch(uint64_t key, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* digits, const uint32_t* perm, uint32_t n,
                     uint64_t* e1_out, uint64_t* e2_out, uint64_t* trace_out);
/* pk: one point; cards: m points; rs, omegas: m scalars each, drawn by the CALLER.  e1_out, e2_out: m points; proofs_out: m blobs. */
int uzk_cp_mask_prove_batch(const uint64_t* pk_mont, const uint64_t* cards_mont, const uint64_t* rs, const uint64_t* omegas, uint32_t m,
                            uint64_t* e1_out, uint64_t* e2_out, uint8_t* proofs_out);
/* verdict_out     m bytes, the first that applies over the six points pk, card, e1, e2, a, b: 1 a coordinate or proof word >= q; 2 a
 *                 point off the curve; 3 a point outside the prime subgroup; 4 r G != a + c e1; 5 r pk != b + c (e2 - card); 0 accepted
 * challenges_out  optional, m x 4 words: c_i as plain integers below L (undefined for a verdict of 1) */
int uzk_cp_mask_verify_batch(const uint64_t* pk_mont, const uint64_t* cards_mont, const uint64_t* e1_mont, const uint64_t* e2_mont,
                             const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, uint64_t* challenges_out);

/* ---- the shuffle circuit: zshuffle's constraint system and its witness on the device ------------------------------------------------
 * build_cs (shuffle/src/build_cs.rs:26-55) drives a TurboCS through new(), per card new_card_variable / prepare_pi_card_variable /
 * eval_card_remark, then shuffle_card, the new deck's prepare_pi_card_variable and pad.  For a deck of N cards the resulting circuit is
 * a pure function of N:
 *   size      2 + 89 N + 2 N (ceil(N/3) + 1) + 4 N (ceil(N/2) + ceil(ceil(N/2)/3)) + 4 N gates, padded to n = the next power of two
 *             (N = 52: 14 094 -> 16 384; N = 20: 3 302 -> 4 096; N = UZK_SHUFFLE_CS_MAX_CARDS = 64: 20 322 -> 32 768)
 *   tables    the indexer's evaluation vectors (indexer.rs:301-478): nine selectors, s = k[perm / n] omega^(perm mod n) over
 *             compute_permutation, qb on the row-sum gates, q_prk zero, q_ecc = the marker of the 84 constrained rows of every card's
 *             remark block (NOT selector 7, which is zero), and x, y, d x y of the remask tables T_G / T_pk on those rows
 *   witness   every variable's value follows from the deck, its remark trace and the permutation; extend_witness gathers them by the
 *             wiring, compute_witness_selectors lays the digits' bits (bit 0, bit 1, +-1 by bit 2) over the remark blocks
 * The 32 key commitments come in the order of the reference's verifier key: cm_q (9), cm_s (5), cm_qb, cm_prk (4, the point at
 * infinity), cm_q_ecc, cm_shuffle_generator (12).  tests/test_shuffle_cs_ref_host.py and tests/test_gpu_shuffle_cs.py hold the layout
 * to the keys the reference generated for 52 and 20 cards, bit for bit. */
#define UZK_SHUFFLE_CS_MAX_CARDS 64
#define UZK_SHUFFLE_CS_MAX_BATCH 64
#define UZK_SHUFFLE_CS_KEY_COMMITMENTS 32
/* Host only.  Every output optional (NULL); pi_rows_out: 8 cards rows (verifier_params.public_vars_constraint_indices: the deck's
 * cards as e2.x, e2.y, e1.x, e1.y, then the new deck's).  cards outside 1 .. UZK_SHUFFLE_CS_MAX_CARDS: UZK_ERR_PARAMETER. */
int uzk_shuffle_cs_info(uint32_t cards, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out);
typedef struct {
    uint32_t cards;                       /* 1 .. UZK_SHUFFLE_CS_MAX_CARDS */
    uint32_t precompute;                  /* as uzk_circuit_desc.precompute */
    const uzk_g1_affine* lagrange_bases;  /* n points, n = the padded size (uzk_shuffle_cs_info) */
    const uzk_g1_affine* blind_bases;     /* 6 points, as uzk_circuit_desc.blind_bases */
    uint64_t k[5][4];                     /* verifier_params.k */
    uint64_t group_gen[4];                /* must equal uzk_domain_group_gen(n), else UZK_ERR_FFT */
} uzk_shuffle_circuit_desc;
/* Builds the layout, writes the evaluation vectors with one kernel pass and runs them through the path of uzk_circuit_refresh_tables
 * (iFFT -> coset FFT -> Lagrange commit).  The handle is an ordinary circuit with shuffle = 1: uzk_prove_round1..5, uzk_circuit_info,
 * uzk_circuit_table and uzk_circuit_release take it unchanged.  Until the first uzk_shuffle_circuit_set_key the public-key tables hold
 * the generator's (indexer.rs:472-478 does the same).  commitments_out: optional, UZK_SHUFFLE_CS_KEY_COMMITMENTS points. */
int uzk_shuffle_circuit_create(const uzk_shuffle_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out);
/* refresh_prover_params_public_key (shuffle/src/gen_params/params.rs:57-129) from a remask key's resident T_pk: slots UZK_CS_QPK .. + 12,
 * copy on write as uzk_circuit_update_tables.  commitments_out: optional, the 12 cm_shuffle_public_key of the game. */
int uzk_shuffle_circuit_set_key(uint64_t circuit, uint64_t remark_key, uzk_g1_jac* commitments_out);
/* Remasks and permutes `batch` decks of the circuit's size and leaves their witnesses on the device, ready for uzk_prove_round1 with
 * inputs_on_device = 1.  The remark trace never leaves the device.
 *   e1_mont, e2_mont  batch x cards points;  digits  batch x cards x 84 bytes;  perms  batch x cards, each a permutation (as
 *                     uzk_remark_batch: out[i] = remasked[perm[i]]), or NULL for identities
 *   d_witness         device, batch x 5 n elements: extend_witness;  d_wsel  device, batch x 3 n: compute_witness_selectors
 *   pi_values_out     host, batch x 8 cards elements in the order of the PI rows: verify_shuffle's online inputs
 *   e1_out, e2_out    host, batch x cards points: the new decks
 * UZK_ERR_PARAMETER before the device is touched: a circuit not made by uzk_shuffle_circuit_create, `cards` (the size of the decks the
 * caller's arrays hold) other than the circuit's, batch outside 1 .. UZK_SHUFFLE_CS_MAX_BATCH, an unknown key, a coordinate not below q, a digit above 7, a perm that is no permutation. */
int uzk_shuffle_witness_batch(uint64_t circuit, uint64_t remark_key, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* digits,
                              const uint32_t* perms, uint32_t cards, uint32_t batch, void* d_witness, void* d_wsel, uint64_t* pi_values_out,
                              uint64_t* e1_out, uint64_t* e2_out);

/* ---- the matchmaking circuit: zmatchmaking's constraint system and its witness on the device ------------------------------------------
 * build_cs (matchmaking/src/build_cs.rs:27-66) drives a TurboCS through new(), the variables of a match (N inputs, the random number,
 * the committed seed and its Anemoi hash), Matchmaking::generate_constraints (matchmaking.rs:42-229: the constants 2 .. N - 1, the hash
 * of the seed, the stream cipher over (seed, random number) with N - 1 outputs, then for i = 1 .. N - 1 the division of output i - 1 by
 * i + 1, the one-hot bits of the remainder and the exchange of positions i and remainder of the running output vector), the 2 N + 2
 * public inputs and pad.  For N players the resulting circuit is a pure function of N:
 *   size      N + 15 + (14 P + N - 1 + [P > 1]) + sum_{i=1}^{N-1} (3 i + 4 + 2 ceil((i + 1) / 3)) + 2 N + 2 gates with P = 1 for
 *             N <= 4 and ceil((N - 1) / 3) otherwise, padded to n = the next power of two (N = 50: 5 208 -> 8 192, 6 027 variables;
 *             N = UZK_MATCH_CS_MAX_PLAYERS = 64: 8 295 -> 16 384)
 *   tables    the indexer's evaluation vectors (indexer.rs:301-478) of a circuit without the "shuffle" feature: nine selectors (the
 *             ninth, q_ecc, all zero), s = k[perm / n] omega^(perm mod n), qb on the running sums of the bits, q_prk = the round keys
 *             after the linear layer on the 14 rows of each of the 1 + P permutation blocks
 *   witness   every variable's value follows from the match, the traces of the two sponges and the remainders; extend_witness gathers
 *             them by the wiring.  There are no wire selectors.
 * The 19 key commitments come in the order of the reference's verifier key: cm_q (9, the eighth the point at infinity), cm_s (5), cm_qb,
 * cm_prk (4).  tests/test_match_cs_ref_host.py and tests/test_gpu_match_cs.py hold the layout to the key the reference ships for 50
 * players, bit for bit. */
#define UZK_MATCH_CS_MIN_PLAYERS 3
#define UZK_MATCH_CS_MAX_PLAYERS 64
#define UZK_MATCH_CS_MAX_BATCH 1024
#define UZK_MATCH_CS_KEY_COMMITMENTS 19
/* Host only.  Every output optional (NULL); pi_rows_out: 2 players + 2 rows (verifier_params.public_vars_constraint_indices: the inputs,
 * the outputs, the random number, the commitment).  players outside 3 .. UZK_MATCH_CS_MAX_PLAYERS: UZK_ERR_PARAMETER. */
int uzk_match_cs_info(uint32_t players, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out);
typedef struct {
    uint32_t players;                     /* UZK_MATCH_CS_MIN_PLAYERS .. UZK_MATCH_CS_MAX_PLAYERS */
    uint32_t precompute;                  /* as uzk_circuit_desc.precompute */
    const uzk_g1_affine* lagrange_bases;  /* n points, n = the padded size (uzk_match_cs_info) */
    const uzk_g1_affine* blind_bases;     /* 6 points, as uzk_circuit_desc.blind_bases */
    uint64_t k[5][4];                     /* verifier_params.k */
    uint64_t group_gen[4];                /* must equal uzk_domain_group_gen(n), else UZK_ERR_FFT */
} uzk_match_circuit_desc;
/* Builds the layout, writes the evaluation vectors with one kernel and runs them through the path of uzk_circuit_refresh_tables
 * (iFFT -> coset FFT -> Lagrange commit).  The handle is an ordinary circuit with shuffle = 0 and the Anemoi generator 5:
 * uzk_prove_round1..5 (no wire selectors, 15 evaluations, 19 r_poly scalars), uzk_circuit_info, uzk_circuit_table and uzk_circuit_release
 * take it unchanged.  commitments_out: optional, UZK_MATCH_CS_KEY_COMMITMENTS points. */
int uzk_match_circuit_create(const uzk_match_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out);
/* Hashes the seeds, runs the stream ciphers and leaves the witnesses of `batch` matches on the device, ready for uzk_prove_round1 with
 * inputs_on_device = 1 and no wire selectors.  The Anemoi traces never leave the device.
 *   inputs_mont       batch x players elements;  seeds_mont, randoms_mont  batch elements each
 *   d_witness         device, batch x 5 n elements: extend_witness (the rows behind the pad hold variable 0's value, zero)
 *   pi_values_out     host, batch x (2 players + 2) elements in the order of the PI rows: verify_matchmaking's online inputs (inputs,
 *                     outputs, random number, commitment)
 *   outputs_out       host, batch x players elements: the matched order
 *   commitments_out   host, batch elements: the Anemoi hash of every seed
 * UZK_ERR_PARAMETER before the device is touched: a circuit not made by uzk_match_circuit_create, `players` (the size of the matches the
 * caller's arrays hold) other than the circuit's, batch outside 1 .. UZK_MATCH_CS_MAX_BATCH, a null pointer, an element not below r. */
int uzk_match_witness_batch(uint64_t circuit, const uint64_t* inputs_mont, const uint64_t* seeds_mont, const uint64_t* randoms_mont, uint32_t players,
                            uint32_t batch, void* d_witness, uint64_t* pi_values_out, uint64_t* outputs_out, uint64_t* commitments_out);

/* ---- the reveal circuit: the R1CS of a Groth16 reveal proof and its witness, on the device ----------------------------------------------
 * RevealCircuit (shuffle/src/reveal_with_snark.rs) over ark-r1cs-std 0.4's twisted Edwards gadget: g.scalar_mul_le(sk) == pk and
 * h.scalar_mul_le(sk) == reveal for the constant generator g, the inputs h = masked.e1, reveal, pk and the 256 little-endian Boolean
 * witnesses of sk -- the circuit behind reveal_card_with_snark (shuffle/src/sdk.rs:288-303) and RevealVerifier.sol.
 *   variables    4869: the one; h.x h.y reveal.x reveal.y pk.x pk.y (l = 7, the statement of uzk_g16_verify_batch and
 *                uzk_cp_reveal_verify_batch); x^2, y^2 of the three points; the 256 bits; 255 x 5 witnesses of the fixed-base chain
 *                (v0 v1, tmp.x, tmp.y, res.x, res.y; its iteration 0 is linear); 10 + 255 x 13 of the variable-base chain (u, v0, v1, v0 v1,
 *                tmp, res, then the doubling's xy, x^2, y^2, x3, y3)
 *   constraints  4869 (9 curve checks, 256 bit rows, 255 x 5 + 2, 10 + 255 x 13 + 2); the domain has 8192 points
 * tests/test_reveal_cs_ref_host.py holds the layout to the proving key the reference ships: a proof made over these matrices is
 * accepted under that key's verifying key.
 *   sk           ONE 256-bit integer for the call (four little-endian words, NOT Montgomery; the reference's secrets are below the
 *                subgroup order): all 256 bits enter the circuit as they are
 *   e1_mont      m points, x then y, canonical Montgomery words: any point of the curve (the subgroup is the caller's business, as in
 *                the reference)
 * UZK_ERR_PARAMETER before any launch: a handle not of uzk_reveal_circuit_create, m outside 1 .. UZK_REVEAL_CS_MAX_BATCH, a null pointer,
 * a coordinate not below q, an e1 off the curve. */
#define UZK_REVEAL_CS_VARS 4869
#define UZK_REVEAL_CS_INPUTS 7
#define UZK_REVEAL_CS_MAX_BATCH 1024
/* Host only.  Every output optional (NULL); nnz_out: the non-zero counts of A, B, C. */
int uzk_reveal_cs_info(uint32_t* n_vars_out, uint32_t* n_inputs_out, uint32_t* n_constraints_out, uint64_t* domain_out, uint64_t nnz_out[3]);
/* Host only.  Fills the caller's CSR buffers (sizes from uzk_reveal_cs_info: row_ptr[k] n_constraints + 1 entries, col[k] and val[k]
 * nnz[k]; val: 4 Montgomery words per entry; columns ascend within a row). */
int uzk_reveal_cs_matrices(uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]);
/* desc: a uzk_g16_key_desc whose row_ptr, col and val are NULL (n_constraints 0 or the circuit's).  A key whose n_vars, n_inputs,
 * l_query_len or h_query_len are not the layout's is UZK_ERR_PARAMETER before the device is touched.  Creates the resident Groth16 key
 * from the key's points and the circuit's own matrices, and uploads the 256 constant multiples 2^i G. */
int uzk_reveal_circuit_create(const uzk_g16_key_desc* desc, uint64_t* circuit_out);
/* Releases the circuit and the key it holds.  The caller makes sure no context still works with either. */
int uzk_reveal_circuit_release(uint64_t circuit);
/* The inner key handle, for uzk_g16_key_info, uzk_g16_h_device and uzk_g16_prove_batch[_device]; it lives as long as the circuit. */
int uzk_reveal_circuit_key(uint64_t circuit, uint64_t* key_out);
/* d_z (device): m full assignments of UZK_REVEAL_CS_VARS elements, the layout uzk_g16_prove_batch_device reads; statements_out (host):
 * m x 6 elements e1.x e1.y reveal.x reveal.y pk.x pk.y.  Complete when the call returns. */
int uzk_reveal_witness_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, uint32_t m, void* d_z, uint64_t* statements_out);
/* uzk_reveal_witness_batch into a buffer of the context's, then uzk_g16_prove_batch_device over it: nothing leaves the device in
 * between.  r_mont, s_mont: m blinding scalars each; proofs_out: m proofs as uzk_g16_prove_batch writes them. */
int uzk_reveal_prove_snark_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                                 uint64_t* statements_out, uzk_g16_proof* proofs_out);
/* uzk_reveal_witness_batch into the same buffer, then uzk_g16_prove_batch_finish over it: the proofs leave the call as the blobs
 * uzk_g16_verify_batch reads.  proofs_out, blobs_out (host) and d_blobs_out (device) as there: any may be NULL, not all. */
int uzk_reveal_prove_snark_batch_finish(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont,
                                        uint32_t m, uint64_t* statements_out, uzk_g16_proof* proofs_out, uint8_t* blobs_out, void* d_blobs_out);

/* ---- Anemoi-Jive over BN254's scalar field: hashes, the stream cipher, their traces (uzkge/src/anemoi) -------------------------------
 * AnemoiJive254: 2 columns, 14 rounds, alpha = 5, g = 5, delta = 1 / g, the round keys of the Anemoi paper's pi rule; a sponge of rate
 * 3 (eval_variable_length_hash, eval_stream_cipher).  Batches run one lane per item, every item of a call with the same lengths.
 *   element   4 Montgomery words of Fr, as everywhere in this header; a word not below r is UZK_ERR_PARAMETER before the device is
 *             touched
 *   padding   a nonempty input whose length is a multiple of 3 is absorbed as it is and sigma = 1; any other (the empty one too) gets
 *             a 1 and then zeros up to a multiple of 3, and sigma = 0.  sigma is added to y1 after the last absorbing permutation
 *   outputs   x0, x1, y0 of the state after absorbing, then of every further permutation; a hash is the first of them
 *   trace     n x P x UZK_ANEMOI_TRACE_ELEMS elements, P = uzk_anemoi_permutations(len, out_len).  Per item its P permutations in
 *             the order they run, and per permutation 64 elements -- the fields of AnemoiVLHTrace / AnemoiStreamCipherTrace:
 *               [0, 4)    before_permutation                              x0 x1 y0 y1
 *               [4, 60)   intermediate_values_before_constant_additions   round 0 .. 13, each x0 x1 y0 y1 after that round's S-box
 *               [60, 64)  after_permutation                               x0 x1 y0 y1 (before sigma is added, as in the reference)
 * A batch of 0 or above UZK_ANEMOI_MAX_BATCH, len above UZK_ANEMOI_MAX_INPUT and out_len outside 1 .. UZK_ANEMOI_MAX_OUTPUT are
 * UZK_ERR_PARAMETER.  len == 0 is legal (inputs_mont may then be NULL): the single chunk (1, 0, 0). */
#define UZK_ANEMOI_MAX_BATCH 1048576
#define UZK_ANEMOI_MAX_INPUT 96
#define UZK_ANEMOI_MAX_OUTPUT 96
#define UZK_ANEMOI_TRACE_ELEMS 64
/* states_mont, out_mont: n x (x0 x1 y0 y1).  One permutation each. */
int uzk_anemoi_permute_batch(const uint64_t* states_mont, size_t n, uint64_t* out_mont);
/* inputs_mont: n x len elements; out_mont: n elements; trace_out optional (layout above). */
int uzk_anemoi_hash_batch(const uint64_t* inputs_mont, uint32_t len, size_t n, uint64_t* out_mont, uint64_t* trace_out);
/* out_mont: n x out_len elements; trace_out optional. */
int uzk_anemoi_stream_batch(const uint64_t* inputs_mont, uint32_t len, size_t n, uint32_t out_len, uint64_t* out_mont, uint64_t* trace_out);
/* P: how many permutations one item runs; out_len == 0: a hash.  Pure arithmetic, no device. */
uint32_t uzk_anemoi_permutations(uint32_t len, uint32_t out_len);
/* The zk-friendly reveals (shuffle/src/reveal.rs reveal0 / verify_reveal0 over chaum_pedersen/dl.rs prove0 / verify0): the arguments,
 * the blob and the verdict codes of uzk_cp_reveal_prove_batch / uzk_cp_reveal_verify_batch, with
 * c_i = uzk_anemoi_hash(e1.x e1.y G.x G.y reveal.x reveal.y pk.x pk.y a.x a.y b.x b.y) taken as an integer below r, mod L, in place of
 * the Keccak transcript.  A point enters the hash as into_affine().xy().unwrap_or_default() gives it: the identity (0, 1) as (0, 0) --
 * SUPPOSED from upstream arkworks (xy() of the identity is None), not verified against the reference's fork. */
int uzk_cp_reveal_prove0_batch(const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* omegas, uint32_t m, uint64_t* reveal_out, uint64_t* pk_out,
                               uint8_t* proofs_out);
int uzk_cp_reveal_verify0_batch(const uint64_t* statements_mont, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, uint64_t* challenges_out);

/* ---- the point codec: ark-serialize's compressed G1, G2 and Baby Jubjub points, and keys made of them -----------------------------
 * Everything the reference persists or sends as a point is in this form: groth16_pk.bin (load_groth16_pk), the SDK's key strings
 * (hex_to_point), the card points (index_to_point: a y coordinate alone).  Decoding is a square root per point, one lane each
 * (csrc/sqrt29.hpp); batches take host pointers like uzk_ed_*.
 *   G1    32 bytes: x little-endian; in byte 31 bit 6 = infinity, bit 7 = "y is the larger of y and p - y, as integers"
 *   G2    64 bytes: x.c0 then x.c1, little-endian; the flags in byte 63; "larger" orders Fq2 by c1 first, then c0
 *   Ed    32 bytes: y little-endian; bit 7 of byte 31 = "x is the larger of x and q - x"; no infinity flag, the identity is (0, 1);
 *         x^2 = (1 - y^2) / (1 - d y^2)  (get_point_from_y_unchecked(y, true) is this rule with the bit set)
 * The library is strict: an encoding that ark never writes is status 1.
 *   - G1, G2: infinity is bit 6 set, bit 7 clear and every other bit of the encoding zero; anything else with bit 6 set is status 1
 *   - a masked coordinate (for G2 either component of x) at or above the modulus is status 1
 *   - a sign bit on a coordinate that is its own negation (y = 0; x = 0 on the Edwards curve) is status 1
 * status_out: n bytes in the numbering of uzk_ed_check_points, the first that applies: 1 not a canonical encoding; 2 no point (the
 * right-hand side is not a square); 3 on the curve but [r] P != O (G2) or [L] P != identity (Ed), reported only with check_subgroup
 * != 0 and never for G1 (cofactor 1); 0 accepted.  Outputs are wire form (uzk_g1_affine, uzk_g2_affine, Edwards x then y; canonical
 * Montgomery words); an accepted infinity, and every point whose status is not 0, comes back as all-zero words.  A call returns
 * UZK_OK when it ran, whatever the statuses say.  n == 0, n > UZK_CODEC_MAX_BATCH (larger inputs are the caller's loop) or a null
 * pointer: UZK_ERR_PARAMETER before the device is touched.
 * Encoding checks only that the coordinates are below the modulus (status 1: 32 or 64 zero bytes come back); it does not check the
 * curve.  All-zero G1 / G2 words are infinity. */
#define UZK_CODEC_MAX_BATCH 1048576
int uzk_g1_decompress_batch(const uint8_t* enc, size_t n, uzk_g1_affine* out, uint8_t* status_out);
int uzk_g2_decompress_batch(const uint8_t* enc, size_t n, int check_subgroup, uzk_g2_affine* out, uint8_t* status_out);
int uzk_ed_decompress_batch(const uint8_t* enc, size_t n, int check_subgroup, uint64_t* points_mont_out, uint8_t* status_out);
int uzk_g1_compress_batch(const uzk_g1_affine* points, size_t n, uint8_t* out, uint8_t* status_out);
int uzk_g2_compress_batch(const uzk_g2_affine* points, size_t n, uint8_t* out, uint8_t* status_out);
int uzk_ed_compress_batch(const uint64_t* points_mont, size_t n, uint8_t* out, uint8_t* status_out);
/* n compressed points decoded straight into device memory the new handle owns (an SRS handle as of uzk_srs_register, a G2 handle as of
 * uzk_g2_register; any n >= 1, decoded UZK_CODEC_MAX_BATCH at a time).  Any non-zero status refuses the call with UZK_ERR_PARAMETER,
 * uzk_last_error names the first bad index, and no handle is made. */
int uzk_srs_register_compressed(const uint8_t* enc, size_t n, uint64_t* handle_out);
int uzk_g2_register_compressed(const uint8_t* enc, size_t n, int check_subgroup, uint64_t* handle_out);
/* The sections of a compressed Groth16 ProvingKey<Bn254> (groth16_pk.bin): vk = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | Vec
 * gamma_abc_g1, then beta_g1 | delta_g1 | Vec a_query | Vec b_g1_query | Vec b_g2_query | Vec h_query | Vec l_query (a Vec: u64
 * little-endian length, then the elements).  Arrays are indexed by UZK_PK_* (the struct cannot share the function's name in C: uzk_g16_pk_sections). */
#define UZK_G16_PK_SECTIONS 12
#define UZK_PK_ALPHA_G1 0
#define UZK_PK_BETA_G2 1
#define UZK_PK_GAMMA_G2 2
#define UZK_PK_DELTA_G2 3
#define UZK_PK_GAMMA_ABC_G1 4
#define UZK_PK_BETA_G1 5
#define UZK_PK_DELTA_G1 6
#define UZK_PK_A_QUERY 7
#define UZK_PK_B_G1_QUERY 8
#define UZK_PK_B_G2_QUERY 9
#define UZK_PK_H_QUERY 10
#define UZK_PK_L_QUERY 11
typedef struct {
    uint64_t offset[UZK_G16_PK_SECTIONS];       /* of the section's first encoding, in bytes */
    uint64_t count[UZK_G16_PK_SECTIONS];        /* encodings in the section */
    uint64_t infinities[UZK_G16_PK_SECTIONS];   /* of them, how many have the infinity bit set */
    uint64_t bytes;                             /* the length of the key */
} uzk_g16_pk_sections;
/* Host only, no device.  A key that ends inside a section, a length that does not fit the bytes left, or bytes behind the key:
 * UZK_ERR_PARAMETER, and uzk_last_error names the section. */
int uzk_g16_pk_layout(const uint8_t* pk, size_t len, uzk_g16_pk_sections* out);
/* A key from its bytes: ALL G1 encodings are decoded in one launch and all G2 encodings in one (with validate != 0 also the G2
 * subgroup check, one more launch), then the points go to uzk_g16_vk_create / uzk_reveal_circuit_create through host memory.  Any
 * non-zero status refuses the key with UZK_ERR_PARAMETER; uzk_last_error names the section and the index in it.  Without validate the
 * points are still decoded strictly and are on their curves (a decoded point always is); only the subgroup of the G2 points is taken on
 * trust, as the reference does (deserialize_compressed_unchecked).
 * uzk_g16_vk_create_compressed reads the first 232 + 32 l bytes of key (a verifying key, or a proving key's head) and ignores what lies
 * behind them; uzk_reveal_circuit_create_compressed takes the whole proving key. */
int uzk_g16_vk_create_compressed(const uint8_t* key, size_t len, int validate, uint64_t* vk_out);
int uzk_reveal_circuit_create_compressed(const uint8_t* pk, size_t len, int validate, uint64_t* circuit_out);

/* ---- synthetic workloads (bench / tests; generated on device, nothing uploaded) -------- */
/* d_points[i] = (i + 1) * Q with Q = seed_scalar * G: n distinct valid G1 points whose discrete
 * logs relative to Q are known, so MSM(points, s) == (sum_i s_i (i+1)) * Q for any size. */
int uzk_synth_points_arith(void* d_points, size_t n, const uint64_t* seed_scalar_mont);
/* d_points[i] = hash-to-curve of a SplitMix64 counter stream (try-and-increment on x):
 * pseudo-random G1 points with unknown discrete logs. */
int uzk_synth_points_random(void* d_points, size_t n, uint64_t seed);
/* Uniform Fr elements (Montgomery form) from a SplitMix64 counter stream. */
int uzk_synth_scalars(void* d_scalars, size_t n, uint64_t seed);
/* The illustrative prover-like mix (SURVEY.md 8d set B): by a hash of the index 50 % zero, 20 % one,
 * 10 % r - 1, 10 % below 2^16, 10 % uniform. */
int uzk_synth_scalars_mix(void* d_scalars, size_t n, uint64_t seed);

/* ---- element-wise field arithmetic on host arrays (the host mirrors' helper) --------------- */
/* The device's field primitives applied element-wise to host arrays: what the host-side mirrors use for format conversion and the
 * few O(n) field operations they own (include/uzkge_poly_commit.hpp: the SRS blob's canonical coordinates -> Montgomery form,
 * apply_blind_factors' negations).  field: 0 = Fq, 1 = Fr.  op: 0 mul, 1 add, 2 sub, 4 sqr, 5 neg, 6 from_mont, 7 to_mont
 * (unary ops ignore b).  Any other op: UZK_ERR_PARAMETER -- the known-answer opcodes of the arithmetic cores live in
 * include/uzkge_gpu_test.h (uzk_test_field_kat), outside the drop-in ABI. */
int uzk_field_op_device(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);

/* ---- measurement ---------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by hipEvents on the library stream. */
int uzk_profile_enable(int on);
int uzk_profile_reset(void);
/* Total elapsed ms and launch count of kernel `name` since the last reset. */
int uzk_profile_get(const char* name, double* total_ms, uint64_t* launches);
/* Newline-separated "name launches total_ms" table into buf. */
int uzk_profile_dump(char* buf, size_t cap);
/* Block until the library stream is idle. */
int uzk_sync(void);
/* The library's hipStream_t (so callers can order their own work against it). */
void* uzk_stream(void);
/* Tuning knobs (0 = automatic): MSM window bits.  Like uzk_tune, this sets the calling thread's CURRENT CONTEXT only;
 * a context created afterwards inherits its creator's settings. */
int uzk_msm_set_window_bits(int c);
/* What a general-mode MSM over n points will use: signed window width and window count (every
 * point is added into one bucket per window: n * windows mixed additions). */
int uzk_msm_plan_info(size_t n, int* window_bits, int* windows);
/* The switches of the calling thread's current context (a context made afterwards inherits them).  None changes a result.
 *   "msm_no_precompute"   1: ignore window tables (uzk_srs_precompute): the general pipeline over the plain bases -- what a host
 *                         sets when HBM is short; the A/B of table against no table
 *   "msm_stream_log"      log2 of the point chunk in which the host scalars of a large MSM are uploaded while the previous chunk
 *                         is accumulated (0 = 21); -1: never stream -- upload, then one MSM
 *   "msm_stream_min_log"  host-scalar MSMs of at least 2^this points are streamed (default 22)
 *   "msm_chunk_log"       points per sort pass of one MSM (default 26, the index space of the sort; lower = less workspace)
 *   "msm_small"           0: n <= 2^15 takes the general pipeline too (default 1: one workgroup per (vector, window))
 *   "msm_seg_sort"        0: the generic last sort pass instead of one workgroup per segment; 10 + k: segment kernel k at any size
 *   "ntt_tile"            1024 / 2048: elements per workgroup of an NTT pass at every size (default 0: by size)
 *   "ntt_two_pass"        0: transforms of 2^17 .. 2^21 elements in three passes of 5 .. 8 bits (default 1: two passes of 9 .. 11)
 *   "arith29"             bit mask, default 7: which of the prover's kernels run on the lazy 29-bit limbs (csrc/lz29.hpp) instead of
 *                         8 x 32-bit Montgomery words -- 1: the quotient kernel, 2: the lane evaluations and linear combinations,
 *                         4: the MSM's bucket-side additions (class sums, folds, the small pipeline's quads).  Same bytes either way
 *   "verify_transcript"   which transcript kernel uzk_verify_fold runs: 1 one proof per lane, 2 a proof's sponge state spread over the
 *                         lanes of a half wave (default 0: the same as 2)
 * The last six exist so that the tests reach every pipeline and instantiation at sizes the CPU oracle can check
 * (tests/test_gpu_variants.py, tests/test_gpu_arith29.py).  Unknown keys are UZK_ERR_PARAMETER. */
int uzk_tune(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* UZKGE_GPU_H */
