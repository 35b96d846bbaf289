// Process-wide backend context: one HIP device, one stream, grow-only HBM workspaces, per-kernel
// hipEvent profiling.  One process per GPU (the multi-GPU MSM runs one process per device and
// exchanges 96-byte partial sums through the host language's RCCL binding).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/uzkge_gpu.h"
#include "../../include/uzkge_gpu_test.h"
#include "ec.hpp"

namespace uzk {

void set_error(const char* fmt, ...);
int on_exception(const char* fn) noexcept;   // the catch (...) of every extern "C" entry point: message + UZK_ERR_DEVICE

#define UZK_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            (void)hipGetLastError(); /* the runtime keeps it as its sticky last error: clear it */ \
            ::uzk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return UZK_ERR_DEVICE;                                                         \
        }                                                                                  \
    } while (0)

#define UZK_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != UZK_OK) return _rc; \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes);   // grow-only; contents NOT preserved on growth
    void release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Small per-round arguments of the prover's lane kernels (challenges, blinds, lengths, pointer lists): the host writes them into
// pinned memory, ONE copy per round puts them into HBM, the kernels read them with scalar loads.  A round ends with a
// synchronisation (its commitments or evaluations are results), so the next round may overwrite the block.
struct ArgArena {
    char* h = nullptr;
    char* d = nullptr;
    size_t cap = 0, used = 0, uploaded = 0;
    int init(size_t bytes);
    void release();
    void reset() { used = 0; uploaded = 0; }
    // `count` objects of T: host pointer to fill, device pointer for the kernels (nullptr when the block is full: callers size it)
    template <class T> T* push(size_t count, const T** dev) {
        const size_t at = (used + 15) & ~(size_t)15, bytes = count * sizeof(T);
        if (at + bytes > cap) { *dev = nullptr; return nullptr; }
        used = at + bytes;
        *dev = reinterpret_cast<const T*>(d + at);
        return reinterpret_cast<T*>(h + at);
    }
    int upload(hipStream_t s);   // what was pushed since the last upload
};

struct ProfEntry {
    std::string name;
    hipEvent_t e0, e1;
};

struct NttPlan;   // ntt.hip
struct MsmWork;   // msm.hip

// One context = one stream, one set of grow-only workspaces, one lock.  The default context serves callers that
// never ask for another; uzk_ctx_create / uzk_ctx_set_current give every prover thread its own, so independent
// proofs overlap on the GPU (at n = 2^14 a single proof leaves most of the chip idle).  The device binding and the
// SRS registry are process-wide (Shared, api.cpp).
struct Ctx {
    std::mutex mu;
    bool ready = false;
    int want_device = -1;              // uzk_ctx_create_on: the device this context lives on; -1: the process's default device (uzk_init)
    int device = -1;                   // the device it was made ready on
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;     // second pipeline instance of large MSMs
    hipStream_t cur_stream = nullptr;  // stream the profiling events are recorded on
    int num_cus = 256;
    // profiling
    bool prof_on = false;
    std::vector<ProfEntry> prof_pending;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, std::pair<double, uint64_t>> prof_totals;
    // NTT plans keyed by (n << 1 | inverse)
    std::map<uint64_t, NttPlan*> ntt_plans;
    DevBuf ntt_scratch[2];
    DevBuf ntt_io;            // staging for the host-pointer API
    // MSM
    MsmWork* msm = nullptr;
    DevBuf msm_scalars;       // staging for host scalars
    Fp* msm_tail_host = nullptr;   // pinned: the tail scalars of the current call (uzk_msm_g1_batch_tail_device)
    size_t msm_tail_cap = 0;
    int msm_window_bits = 0;  // 0 = auto
    // uzk_tune: switches with a production use, and three that let the tests reach every pipeline at small sizes
    int tune_no_precompute = 0;    // 1: ignore window tables (uzk_srs_precompute) -- the general pipeline over the plain bases
    int tune_ntt_two_pass = 1;     // 2^17 .. 2^21 as two passes of 9 .. 11 bits (0: the three passes of 5 .. 8 bits -- tests reach both)
    int tune_ntt_tile = 0;         // elements per workgroup of an NTT pass: 2048 (512 threads), 1024 (256 threads), 0 = by size
    int tune_small = 1;            // 1: n <= 2^15 takes the one-workgroup-per-slot pipeline (msm_small_*); 0: the general pipeline at every size
    int tune_chunk_log = 26;       // point-chunk size of one sort pass (tests lower it to reach the chunk loop at small n)
    int tune_stream_log = 0;       // log2 of the point chunk of a streamed host-scalar MSM (0 = 21); -1: never stream (upload, then one MSM)
    int tune_stream_min_log = 22;  // host-scalar MSMs of at least 2^this points are streamed (tests lower it)
    // bit 0: the quotient kernel, bit 1: evaluations / linear combinations, bit 2: the bucket-side group additions of the MSM on the lazy
    // 29-bit arithmetic (lz29.hpp) instead of 8 x 32-bit Montgomery words; same bytes either way.  Default: all on (UZK_ARITH29 in the
    // environment changes the default of every context of the process: the A/B runs of tests/cpp/prover_rounds); uzk_tune("arith29", mask).
    int tune_arith29 = default_arith29();
    static int default_arith29() {
        static const int v = [] { const char* e = std::getenv("UZK_ARITH29"); return e ? std::atoi(e) : 7; }();
        return v;
    }
    int tune_seg_sort = 1;         // 1: last pass of a packed two-pass sort = one workgroup per segment (msm_radix_segment_kernel); 0: the generic kernels; 10 + k: instantiation k whatever the size (tests)
    int tune_msm_taper = 1;        // the end of the accumulator's task schedule is made of short tasks (msm_cut.hpp): 0 never, 1 where the task list is several times the resident lanes, 2 at any size (tests)
    // poly.hip workspaces (grow-only)
    DevBuf poly_tmp, poly_tmp2, poly_io, zpoly_tmp, open_tmp, poly_args;
    DevBuf poly_cnt;                 // per-polynomial arrival counters of poly_eval_small (zero between calls); trimmed-length results
    uint32_t trim_flip = 0;          // which of the two trimmed-length result sets the next call uses
    void* poly_host = nullptr;       // pinned, device-visible: small results written by the kernels themselves
    size_t poly_host_cap = 0;
    // ntt.hip: decimated sub-vectors of the small 3 * 2^k path; three-level power tables of arbitrary
    // elements (coset shifts, mixed-radix roots) cached by VALUE, least recently used entry replaced
    DevBuf ntt_sub;
    struct PowCache { Fp key; bool valid = false; uint64_t stamp = 0; DevBuf buf; };
    PowCache pow_cache[8];
    uint64_t pow_stamp = 0;
    std::vector<void*> ntt_fused;   // NttFused* (ntt.hip): tables of the fused coset / radix-3 transforms
    // g1ntt.hip: twiddle digits keyed by n (G1NttPlan*), the working array of extended points, the prefix products of the
    // conversion to affine, staging for the host-pointer API (grow-only)
    std::map<uint64_t, void*> g1ntt_plans;
    DevBuf g1ntt_work, g1ntt_prefix, g1ntt_io;
    // verify.hip: one block carved into the arrays of a fold (proofs, decoded words, challenges, coefficients, the MSMs' inputs)
    DevBuf verify_ws;
    // srscheck.hip: one record per workgroup of the curve kernel, the weights of a fold, the forward transform of a Lagrange
    // handle (grow-only)
    DevBuf srs_records, srs_weights, srs_points;
    // g2msm.hip: the workspaces of the G2 MSM (G2Work*, grow-only)
    void* g2 = nullptr;
    // groth16.hip: the workspaces of the Groth16 prover (G16Work*, grow-only)
    void* g16 = nullptr;
    // g16verify.hip: one block carved into the arrays of a Groth16 fold (proofs, public inputs, weights, decoded points, results)
    DevBuf g16v_ws;
    // pairing.hip: one block carved into the arrays of a pairing product (constants, points, statuses, the tree's two levels)
    DevBuf pairing_ws;
    std::vector<uint8_t> pairing_status;   // the statuses of a product's pairs on the host (grow-only)
    // edwards.hip: one block carved into the arrays of a Baby Jubjub call (points, scalars, proofs, statuses, results)
    DevBuf ed_ws;
    DevBuf ed_gen;                    // T_G, the generator's half of the remask tables: a constant, built once per context
    bool ed_gen_ready = false;
    // shufflecs.hip: one block carved into the arrays of a shuffle witness (decks, digits, the remark trace, variable values)
    DevBuf shuffle_ws;
    // matchcs.hip: one block carved into the arrays of a matchmaking witness (matches, the two Anemoi traces, steps, variable values)
    DevBuf match_ws;
    // revealcs.hip: one block carved into the arrays of a reveal witness (cards, the chains' workspace, affine points), and the
    // assignments of uzk_reveal_prove_snark_batch
    DevBuf reveal_ws;
    DevBuf reveal_z;
    // codec.hip: one block carved into the arrays of a decoding or encoding call (bytes, points, statuses)
    DevBuf codec_ws;
    int tune_verify_transcript = 0;   // which transcript kernel a fold runs: 1 one proof per lane; 0 / 2 a proof's state spread over a half wave (the default)
    // an entry of the process-wide SRS registry
    struct Srs {
        Affine* d_points = nullptr;
        size_t n = 0;
        bool owned = false;
        int device = 0;
        // optional window table (uzk_srs_precompute): table[j*n + i] = 2^(pre_c*j) * P_i
        Affine* d_table = nullptr;
        int pre_c = 0;
        uint32_t pre_W = 0;
    };

    hipEvent_t get_event();
    void prof_begin(const char* name);
    void prof_end();
    int prof_collect();   // sync + fold pending events into totals
};

// The scalars of an MSM call: vector b, element i is main[b * stride + i] for i < n_main and
// tail[b * tail_n + (i - n_main)] beyond (n = n_main + tail_n).  The tail carries the blind factors of a commit
// (apply_blind_factors, kzg_poly_commitment.rs:299-313) so that they ride in the commit's own MSM; it may live in
// pinned host memory (a few dozen elements, read once by the digit kernel).
struct ScalarView {
    const Fp* main = nullptr;
    uint64_t stride = 0;
    uint32_t n_main = 0;
    const Fp* tail = nullptr;
    uint32_t tail_n = 0;
    // Vectors in groups: vector b lives at main[(b / group) * group_stride + (b % group) * stride].  The prover's batched round 1
    // commits 8 of the 10 evaluation vectors of every proof of a lockstep batch (prover.cpp); one group = everything else.
    uint32_t group = 0xffffffffu;
    uint64_t group_stride = 0;
    static ScalarView dense(const Fp* p, size_t n) { ScalarView v; v.main = p; v.stride = n; v.n_main = (uint32_t)n; return v; }
    __host__ __device__ const Fp& at(uint32_t b, uint32_t i) const {
        return i < n_main ? main[(uint64_t)(b / group) * group_stride + (uint64_t)(b % group) * stride + i]
                          : tail[(uint64_t)b * tail_n + (i - n_main)];
    }
};

Ctx& ctx();
std::mutex& ctx_mutex();
int require_ready();
// While one lives, ctx() on this thread is `c`: a round that several callers share runs on a library-internal context
// (coalesce.cpp), whatever context the thread that happens to run it has made current.
struct CtxScope {
    Ctx* prev;
    explicit CtxScope(Ctx* c);
    ~CtxScope();
    CtxScope(const CtxScope&) = delete;
    CtxScope& operator=(const CtxScope&) = delete;
};
int ctx_init_internal(Ctx& c, int device);     // a context no handle names, ready on `device`, tuned like the default context
void ctx_release_internal(Ctx& c);
void devices_synchronize();                    // every device a context has been made ready on
void coalesce_release_all();                   // coalesce.cpp (uzk_shutdown)
void sharded_release_all();                    // sharded.cpp (uzk_shutdown)
// api.cpp: the process-wide SRS registry and the pinned-block table, for prover.cpp
uint64_t srs_insert(const Ctx::Srs& e);
bool srs_lookup(uint64_t handle, Ctx::Srs* out);
bool srs_erase(uint64_t handle, Ctx::Srs* out);
bool is_pinned_block(const void* p, size_t bytes);
int msm_dispatch_view(const Ctx::Srs& s, size_t offset, const ScalarView& sv, size_t n, uint32_t batch, Jac* out);
// prover.cpp: frees every circuit and prover (uzk_shutdown)
void prover_release_all();

// RAII kernel-launch bracket:  { KernelScope ks(c, "name"); kernel<<<...>>>(...); }
// host-side section timer feeding the same profile table (entries named host_*)
struct HostScope {
    Ctx& c;
    const char* name;
    std::chrono::steady_clock::time_point t0;
    HostScope(Ctx& c_, const char* n) : c(c_), name(n), t0(std::chrono::steady_clock::now()) {}
    ~HostScope() {
        if (!c.prof_on) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        auto& e = c.prof_totals[name];
        e.first += ms; e.second += 1;
    }
};

struct KernelScope {
    Ctx& c;
    KernelScope(Ctx& c_, const char* name) : c(c_) { if (c.prof_on) c.prof_begin(name); }
    ~KernelScope() { if (c.prof_on) c.prof_end(); }
};

// One launch under its own KernelScope, then the launch's error: returns UZK_ERR_DEVICE from the enclosing function like UZK_HIP.
// The stream is the caller's to name; c.cur_stream (where the profiling events go) is left alone.
//     UZK_LAUNCH(c, "name", kernel, grid, block, lds_bytes, stream, args...);
#define UZK_LAUNCH(c, name, kernel, grid, block, lds, stream, ...)                        \
    do {                                                                                   \
        {                                                                                  \
            ::uzk::KernelScope _ks((c), (name));                                           \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);             \
        }                                                                                  \
        UZK_HIP(hipGetLastError());                                                        \
    } while (0)

// While one lives, the calling thread's current device is `device`; then it is what it was.  Freeing a key's memory needs the
// key's device current, and must not leave the caller's thread on it.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// entry points implemented in the .hip files
int ntt_run(Ctx& c, const Fp* d_in, Fp* d_out, uint64_t n, bool inverse, const Fp* coset_shift_host, uint32_t batch,
            uint64_t in_stride = 0, uint64_t out_stride = 0, uint64_t in_len = 0);
void ntt_free_plans(Ctx& c);
int g1ntt_run(Ctx& c, const Affine* d_in, Affine* d_out, uint64_t n, bool inverse);
void g1ntt_op_count(uint64_t n, bool inverse, uint64_t* dbl_out, uint64_t* add_out);
void g1ntt_free(Ctx& c);
// verify.hip: verifier keys (process-wide handles) and the fold of a batch of proofs
int vf_key_check(const uzk_vk_desc* d);
int vf_key_create(Ctx& c, const uzk_vk_desc* d, uint64_t* out);
bool vf_key_known(uint64_t h, uint32_t* cs_size, uint32_t* n_pi, uint32_t* proof_bytes, int* device);
int vf_key_release(uint64_t h);
void vf_release_all();
int vf_key_set_public_key(Ctx& c, uint64_t h, const Affine* pk);
int vf_fold_run(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pi, uint32_t m, const Fp* weights, Jac* left_out, Jac* right_out,
                uint8_t* status_out, Fp* challenges_out);
int vf_keccak_test(Ctx& c, const uint8_t* msgs, const uint64_t* offsets, uint32_t count, uint8_t* out);
// srscheck.hip: the curve report of d_points[0 .. count) (first_bad relative to d_points), the fold weights of a seed on the
// device and on the host (the same code)
int srs_curve_run(Ctx& c, const Affine* d_points, uint64_t count, uzk_srs_curve_report* out);
int srs_weights_run(Ctx& c, const uint8_t seed[32], uint64_t first, uint64_t count, Fp* d_out);
void srs_weights_host(const uint8_t seed[32], uint64_t first, uint64_t count, Fp* out);
void srscheck_free(Ctx& c);
// g2msm.hip: the G2 base registry (process-wide handles, like the SRS registry), the MSM over device bases and device scalars, the
// host-side fold / affine map, the known-answer kernel
struct G2Affine;
struct G2Jac;
int g2_register(Ctx& c, const G2Affine* points, size_t n, uint64_t* handle_out);
bool g2_lookup(uint64_t handle, const G2Affine** d_points, size_t* n, int* device);
bool g2_release(uint64_t handle);
void g2_release_all();
void g2_free(Ctx& c);
int g2_msm_run(Ctx& c, const G2Affine* d_points, const Fp* d_scalars, size_t n, uint32_t batch, G2Jac* out_host);
// the same sums finished on the device: canonical affine points (infinity all zeros) to out_host, to d_out, or to both
int g2_msm_finish_run(Ctx& c, const G2Affine* d_points, const Fp* d_scalars, size_t n, uint32_t batch, G2Affine* out_host, G2Affine* d_out);
void g2_fold_host(const G2Jac* partials, size_t count, G2Jac* out);
void g2_to_affine_host(const G2Jac* p, G2Affine* out);
int g2_op_device(Ctx& c, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int g2_raw_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n);
// groth16.hip: Groth16 proving keys (process-wide handles), the witness map and the batched prover
int g16_key_check(const uzk_g16_key_desc* d, uint64_t* domain_out);
int g16_key_create(Ctx& c, const uzk_g16_key_desc* d, uint64_t* out);
bool g16_key_known(uint64_t h, uint32_t* n_vars, uint32_t* n_inputs, uint32_t* n_constraints, uint64_t* domain, int* device);
bool g16_key_release(uint64_t h);
void g16_release_all();
void g16_free(Ctx& c);
int g16_h_run(Ctx& c, uint64_t h, const Fp* d_z, uint32_t batch, Fp* d_h);
int g16_prove_run(Ctx& c, uint64_t h, const Fp* z, bool z_on_device, const Fp* r_host, const Fp* s_host, uint32_t batch, uzk_g16_proof* out);
// the same proofs with C, the affine maps and the verifier's blob computed on the device; any of the three outputs may be null but one
int g16_prove_finish_run(Ctx& c, uint64_t h, const Fp* z, bool z_on_device, const Fp* r_host, const Fp* s_host, uint32_t batch, uzk_g16_proof* proofs_out,
                         uint8_t* blobs_out, uint8_t* d_blobs_out);
int g16_finish_test_run(Ctx& c, const Jac* a, const Jac* b1, const Jac* k, const Fp* r_host, const Fp* s_host, uint32_t n, Affine* a_out, Affine* c_out);
int g16_plan_test(Ctx& c, uint32_t m, uint32_t l, uint32_t nc, uint32_t* group_out, uint64_t lens_out[3], int admitted_out[3]);
// g16verify.hip: Groth16 verifying keys (process-wide handles) and the fold of a batch of proofs
int g16v_key_check(const uzk_g16_vk_desc* d);
int g16v_key_create(Ctx& c, const uzk_g16_vk_desc* d, uint64_t* out);
bool g16v_key_known(uint64_t h, uint32_t* n_inputs, int* device);
int g16v_key_release(uint64_t h);
void g16v_release_all();
int g16v_fold_run(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pub, uint32_t m, const Fp* weights, Affine* a_out, G2Affine* b_out,
                  Jac* alpha_out, Jac* x_out, Jac* c_out, uint8_t* status_out);
// pairing.hip: the pairing product over host or device points (the first pair that failed its check in *bad_out, n if none), the
// constants the host computes at start-up, the known-answer kernels
struct Fq12w;
int pairing_product_run(Ctx& c, const Affine* p, const G2Affine* q, bool on_device, uint32_t n, Fq12w* gt_out, uint32_t* bad_out, uint8_t* bad_status);
bool gt_is_one(const Fq12w& a);
int pairing_kat_device(Ctx& c, int op, const Fq12w* a, const Fq12w* b, Fq12w* out, uint32_t n);
int pairing_miller_device(Ctx& c, const Affine* p, const G2Affine* q, uint32_t n, Fq12w* out);
int pairing_raw_kat_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, uint32_t n);
int pairing_raw_step_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, uint32_t n);
// g16verify.hip: the fold, then the product of its M + 3 pairs without leaving the device (g2: beta, gamma, delta on the host)
int g16v_verify_run(Ctx& c, uint64_t h, const uint8_t* proofs, const Fp* pub, uint32_t m, const Fp* weights, const G2Affine* g2, uint8_t* status_out,
                    Fq12w* gt_out, uint32_t* bad_g2_out);
// edwards.hip: Baby Jubjub -- point classification, scalar multiplications, sums, and the Chaum-Pedersen reveal proofs over it
struct EdAffine;
size_t ed_first_noncanonical(const Fp* words, size_t count);
int ed_check_run(Ctx& c, const EdAffine* pts, size_t n, uint8_t* status_out);
int ed_mul_run(Ctx& c, const EdAffine* pts, bool shared_base, const Fp* scalars, size_t n, EdAffine* out);
int ed_sum_run(Ctx& c, const EdAffine* e2, const EdAffine* rows, uint32_t k, uint32_t n, EdAffine* out);
int cp_verify_run(Ctx& c, const EdAffine* statements, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, Fp* challenges_out, bool anemoi);
int cp_prove_run(Ctx& c, const Fp* sk, const EdAffine* e1, const Fp* omegas, uint32_t m, EdAffine* reveal_out, EdAffine* pk_out, uint8_t* proofs_out,
                 bool anemoi);
int anemoi_permute_run(Ctx& c, const Fp* states, size_t n, Fp* out);                                          // anemoi.hip
int anemoi_sponge_run(Ctx& c, const Fp* inputs, uint32_t len, size_t n, uint32_t out_len, Fp* out, Fp* trace_out);
// the same sponge over inputs that are already on the device, with outputs and trace left there (matchcs.cpp): one launch, nothing is
// copied and nothing waited for.  d_trace: null or n x P x 64 elements
int anemoi_sponge_device(Ctx& c, const Fp* d_inputs, uint32_t len, uint32_t n, uint32_t out_len, Fp* d_out, Fp* d_trace);
int ed_raw_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n);
// codec.hip: compressed points.  group: 0 G1, 1 G2, 2 Baby Jubjub; in / out on the host unless named d_*.  d_out: null (the points
// come back to `out`) or the device array the points are decoded into and stay in.
int codec_decompress_run(Ctx& c, int group, const uint8_t* in, size_t n, bool check_subgroup, void* out, void* d_out, uint8_t* status_out);
int codec_compress_run(Ctx& c, int group, const void* points, size_t n, uint8_t* out, uint8_t* status_out);
int codec_sqrt_kat_run(Ctx& c, int field, const Fp* a, size_t n, Fp* root_out, uint8_t* is_square_out);
int g2_register_owned(G2Affine* d_points, size_t n, int device, uint64_t* handle_out);     // g2msm.hip: the handle takes the array over
// edwards.hip: the Chaum-Pedersen proofs of a mask; remask keys (process-wide handles: T_pk on the device), the tables and the remask
int cp_mask_prove_run(Ctx& c, const EdAffine* pk, const EdAffine* cards, const Fp* rs, const Fp* omegas, uint32_t m, EdAffine* e1_out, EdAffine* e2_out,
                      uint8_t* proofs_out);
int cp_mask_verify_run(Ctx& c, const EdAffine* pk, const EdAffine* cards, const EdAffine* e1, const EdAffine* e2, const uint8_t* proofs, uint32_t m,
                       uint8_t* verdict_out, Fp* challenges_out);
int remark_key_create(Ctx& c, const EdAffine* pk, uint64_t* out);
bool remark_key_known(uint64_t h, int* device);
int remark_key_release(uint64_t h);
void remark_release_all();
// revealcs.hip: the reveal circuit (they take the context lock themselves)
int rcs_info(uint32_t* n_vars, uint32_t* n_inputs, uint32_t* n_constraints, uint64_t* domain, uint64_t nnz_out[3]);
int rcs_matrices(uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]);
int rcs_circuit_create(const uzk_g16_key_desc* desc, uint64_t* circuit_out);
int rcs_circuit_release(uint64_t circuit);
void rcs_release_all();
int rcs_circuit_key(uint64_t circuit, uint64_t* key_out);
int rcs_witness_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, uint32_t m, void* d_z, uint64_t* statements_out);
int rcs_prove_snark_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                          uint64_t* statements_out, uzk_g16_proof* proofs_out);
int rcs_prove_snark_batch_finish(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                                 uint64_t* statements_out, uzk_g16_proof* proofs_out, uint8_t* blobs_out, void* d_blobs_out);
int remark_tables_run(Ctx& c, uint64_t h, Fp* pk_tables_out, Fp* gen_tables_out);
int remark_run(Ctx& c, uint64_t h, const EdAffine* e1, const EdAffine* e2, const uint8_t* digits, const uint32_t* slot, uint32_t n, EdAffine* e1_out,
               EdAffine* e2_out, Fp* trace_out);
// the same remask over arrays that are already on the device and stay there (shufflecs.cpp): n <= 4096 cards, one launch, nothing is
// copied and nothing waited for; the tables of a key as device addresses ([84][4][3] elements each; either output optional, and T_G
// alone needs no key)
int remark_device_run(Ctx& c, uint64_t h, const EdAffine* d_e1, const EdAffine* d_e2, const uint8_t* d_digits, const uint32_t* d_slot, uint32_t n,
                      EdAffine* d_e1_out, EdAffine* d_e2_out, Fp* d_trace);
int remark_device_tables(Ctx& c, uint64_t h, const Fp** d_pk_out, const Fp** d_gen_out);
void msm_plan_info(Ctx& c, size_t n, int* window_bits, int* windows);
// UZK_OK when msm_run takes `batch` vectors of n points (pre_c > 0: over a window table), its refusal otherwise; launches nothing
int msm_admit(Ctx& c, size_t n, uint32_t batch, int pre_c);
int msm_run(Ctx& c, const Affine* points, const ScalarView& scalars, size_t n, uint32_t batch, Jac* out_host, int pre_c,
            uint32_t pre_stride, uint32_t pre_off);
int msm_run_streamed(Ctx& c, const Affine* points, const Fp* scalars_host, size_t n, Jac* out_host);
int msm_run_chunked(Ctx& c, const Affine* points, const Fp* d_scalars, size_t n, Jac* out_host);
int msm_build_table(Ctx& c, const Affine* d_points, size_t n, int cb, Affine** table_out, uint32_t* W_out);
int msm_precompute_window_bits(size_t n, int forced);
void msm_free(Ctx& c);
int synth_points_arith(Ctx& c, Affine* d_points, size_t n, const Fp& seed_scalar_mont);
int synth_points_random(Ctx& c, Affine* d_points, size_t n, uint64_t seed);
int synth_scalars(Ctx& c, Fp* d_scalars, size_t n, uint64_t seed);
int synth_scalars_mix(Ctx& c, Fp* d_scalars, size_t n, uint64_t seed);
int poly_eval_batch(Ctx& c, const Fp* d_coefs, uint64_t n, uint32_t batch, const Fp& x, Fp* out_host);
int poly_eval_batch_host(Ctx& c, const Fp* coefs_host, uint64_t n, uint32_t batch, const Fp& x, Fp* out_host);
int open_quotient_run(Ctx& c, const Fp* d_polys, uint64_t n, uint32_t batch, const Fp& z, const Fp& alpha, Fp* d_q,
                      Fp* evals_host);
int poly_eval_ptrs(Ctx& c, const void* const* d_polys, const uint64_t* lens, const uint32_t* point_idx, uint32_t count,
                   const Fp* points_host, uint32_t n_points, Fp* out_host);
int open_quotient_ptrs(Ctx& c, const void* const* d_polys, const uint64_t* lens, uint32_t count, const Fp& z, const Fp& alpha, Fp* d_q,
                       uint64_t q_cap, Fp* evals_host);
int poly_hide_batch_run(Ctx& c, Fp* d_coefs, uint64_t stride, uint64_t len_in, uint32_t count, const Fp* blinds_host, uint32_t hd,
                        uint64_t zeroing_degree);
int fold_blinds_batch_run(Ctx& c, const Fp* d_polys, uint64_t in_stride, const uint64_t* lens_host, uint64_t N, uint32_t batch, Fp* d_out,
                          uint64_t out_stride, Fp* d_tail, uint32_t tail_n, Fp* blinds_host);
int split_t_run(Ctx& c, const Fp* d_t, uint64_t t_len, uint64_t chunk, uint32_t n_chunks, const Fp* rands_host, Fp* d_chunks,
                uint64_t chunk_stride, uint64_t* lens_out);
int poly_trimmed_len_run(Ctx& c, const Fp* d_polys, uint64_t stride, const uint64_t* lens_host, uint32_t batch, uint64_t* out_host, bool sync);
int fold_blinds_run(Ctx& c, const Fp* d_coefs, uint64_t len, uint64_t N, Fp* d_out, Fp* blinds_host);
int poly_lincomb_run(Ctx& c, const void* const* d_polys, const uint64_t* lens, const Fp* scalars_host, uint32_t count, Fp* d_out,
                     uint64_t out_len);
int poly_hide_run(Ctx& c, Fp* d_coefs, uint64_t len, const Fp* blinds_host, uint32_t hiding_degree, uint64_t zeroing_degree);
int poly_scatter_run(Ctx& c, Fp* d_dst, uint64_t dst_stride, const uint32_t* idx_pinned, const Fp* val_pinned, uint32_t count, uint32_t batch);
struct QuotientDev;
int t_quotient_run(Ctx& c, const void* args_c_abi, Fp* d_out);
int z_poly_device(Ctx& c, const Fp* d_w, const uint32_t* d_perm, const Fp* d_group, const Fp* k_host, const Fp& beta,
                  const Fp& gamma, uint32_t n, uint32_t n_wires, Fp* d_z, bool* zero_den = nullptr);
constexpr uint32_t kZPolyLanesMax = 1u << 16;       // the longest lane of z_poly_lanes
constexpr uint64_t kEvalLanesMax = 1ull << 18;      // the longest polynomial of poly_eval_lanes (its lazy-limb contract)
int z_poly_lanes(Ctx& c, ArgArena& args, const Fp* d_w, uint64_t w_lane_stride, const uint32_t* d_perm, const Fp* d_group, const Fp* k_host,
                 const Fp* d_bg, uint32_t n, uint32_t n_wires, uint32_t lanes, Fp* d_z, uint64_t z_lane_stride, uint8_t* lane_ok);
int t_quotient_lanes(Ctx& c, const void* args_c_abi, uint64_t own_stride, const void* d_lanes, uint32_t lanes, Fp* d_out, uint64_t out_stride);
void quotient_lane(const Fp& alpha, const Fp& beta, const Fp& gamma, const Fp* k, void* lane_out);
size_t quotient_lane_bytes();
// rounds.hip: the lane kernels of the prover's rounds (device-resident argument entries are filled through the *_fill helpers)
int hide_lanes(Ctx& c, Fp* d_coefs, uint64_t lane_stride, uint64_t slot_stride, uint32_t n, uint32_t slots, uint32_t lanes, const Fp* d_blinds);
int poly_eval_lanes(Ctx& c, const void* d_polys, uint32_t count, uint64_t max_len, const Fp* d_points, uint32_t lanes, uint32_t* d_counters, Fp* out_host_pinned);
void eval_poly_fill(void* host_entry, const void* p, uint64_t lane_stride, uint64_t len, uint32_t pt);
size_t eval_poly_bytes();
int poly_lincomb_lanes(Ctx& c, const void* d_polys, uint32_t count, const uint32_t* d_lens, const Fp* d_scalars, uint32_t lanes, Fp* d_out, uint64_t out_stride,
                       uint64_t out_len);
void lin_poly_fill(void* host_entry, const void* p, uint64_t lane_stride);
size_t lin_poly_bytes();
int open_div_lanes(Ctx& c, const Fp* d_h, uint64_t h_stride, uint64_t n, const void* d_pows, uint32_t count, Fp* d_q, uint64_t q_stride, uint64_t q_cap);
void div_pows_fill(void* host_entry, const Fp& z, int per);
size_t div_pows_bytes();
int open_div_per(uint64_t n);
int split_t_lanes(Ctx& c, const Fp* d_t, uint64_t t_stride, const uint32_t* d_t_lens, uint64_t chunk, uint32_t n_chunks, const Fp* d_rands, uint32_t lanes,
                  Fp* d_chunks, uint64_t chunk_stride);
int fold_blinds_lanes(Ctx& c, const Fp* d_polys, uint64_t in_stride, const uint32_t* d_lens, uint64_t N, uint32_t count, Fp* d_out, uint64_t out_stride, Fp* d_tail,
                      uint32_t tail_n);
int trimmed_len_lanes(Ctx& c, const Fp* d_polys, uint64_t stride, uint64_t cap, uint32_t count, uint64_t* d_sets, uint32_t count_max, uint32_t* flip,
                      uint64_t* out_host_pinned);
int z_poly_run(Ctx& c, const Fp* w_host, const uint32_t* perm_host, const Fp* group_host, const Fp* k_host,
               const Fp& beta, const Fp& gamma, uint32_t n, uint32_t n_wires, Fp* z_host);
void poly_free(Ctx& c);
int field_op_device(Ctx& c, int field, int op, const Fp* a, const Fp* b, Fp* out, size_t n);
int g1_op_device(Ctx& c, int op, const Affine* a, const Affine* b, Jac* out, size_t n);
// raw 9-limb known answers (fieldops.hip; include/uzkge_gpu_test.h uzk_test_l29_kat / uzk_test_p29_kat)
bool l29_sig_runnable(int field, uint32_t idx);
int l29_op_device(Ctx& c, int field, int op, uint32_t param, const uint32_t* in, uint32_t* out, size_t n);
bool const_operand_case_known(int op, int form_a, int form_b);
int const_operand_device(Ctx& c, int field, int op, int form_a, int form_b, bool portable, const Fp* a, const Fp* b, Fp* out, size_t n);
int p29_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n);
// which lane kernel runs (rounds.hip): the launchers and the test hook uzk_test_lanes share the choice
struct LaneKernel { bool a29, wide; };
LaneKernel poly_eval_lanes_kernel_of(const Ctx& c, uint32_t lanes, uint64_t max_len);
LaneKernel poly_lincomb_lanes_kernel_of(const Ctx& c, uint32_t count, uint64_t out_len);
int lanes_test(Ctx& c, int op, const void* const* d_polys, const uint64_t* lane_strides, uint32_t count, const uint32_t* lens, const uint32_t* pts,
               const Fp* args, uint32_t lanes, uint64_t len, Fp* out, int* kernel);

}  // namespace uzk
