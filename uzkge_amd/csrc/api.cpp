// extern "C" surface of libuzkge_gpu.so (declared in include/uzkge_gpu.h).
// Thin: argument checks, staging of host buffers, error mapping; all compute is in the .hip files.
// There is deliberately no CPU fallback: without a gfx950 device every compute call fails with
// UZK_ERR_DEVICE.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "anemoi29.hpp"
#include "ctx.hpp"
#include "lane_tools.hpp"
#include "fq12_29.hpp"
#include "g16_pk_layout.hpp"
#include "g2_29.hpp"
#include "host_ec64.hpp"
#include "host_math.hpp"
#include "shufflecs_dev.hpp"
#include "matchcs_dev.hpp"

namespace uzk {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// Every extern "C" entry point is a function-try-block that ends here: no C++ exception (std::bad_alloc from a host-side vector,
// map or shared_ptr; std::system_error from a mutex) crosses the C ABI into a caller that cannot unwind it (Rust with
// panic = "abort", ctypes).  Locks taken by the entry point are released by the unwinding; a prover that was mid-round must be
// destroyed by the caller.
int on_exception(const char* fn) noexcept {
    try { throw; }
    catch (const std::bad_alloc&) { set_error("%s: out of host memory", fn); }
    catch (const std::exception& e) { set_error("%s: %s", fn, e.what()); }
    catch (...) { set_error("%s: C++ exception of unknown type", fn); }
    return UZK_ERR_DEVICE;
}

// Process-wide state: the device this process is bound to, the SRS registry (bases are read-only and shared by
// every context), the contexts.  Lock order: a context's own mutex first, then Shared::mu (held briefly).
struct Shared {
    std::mutex mu;
    bool bound = false;
    int device = -1;                       // the process's default device (uzk_init); contexts of uzk_ctx_create_on name their own
    std::map<int, int> num_cus;            // per device that a context has been made ready on

    std::map<uint64_t, Ctx::Srs> srs;
    uint64_t next_handle = 1;
    std::map<uint64_t, Ctx*> contexts;
    uint64_t next_ctx = 1;                 // never reused: a stale handle cannot name a later context
    std::atomic<uint64_t> epoch{1};        // bumped whenever a context is destroyed (uzk_ctx_destroy, uzk_shutdown)
    std::map<const void*, size_t> pinned;  // uzk_host_alloc blocks (base -> bytes): uploads from them are asynchronous
};
static Shared& shared() {
    static Shared s;
    return s;
}
static Ctx& default_ctx() {
    static Ctx c;
    return c;
}
// The calling thread's context is remembered by HANDLE; the pointer is only a cache, valid while no context has been
// destroyed since it was looked up (Shared::epoch).  A worker thread that outlives uzk_shutdown / uzk_ctx_destroy of its
// context therefore falls back to the default context instead of dereferencing a freed Ctx.
static thread_local uint64_t t_handle = 0;          // 0: the default context
static thread_local Ctx* t_cached = nullptr;
static thread_local uint64_t t_epoch = 0;
static thread_local Ctx* t_scope = nullptr;         // CtxScope: a library-internal context while a shared round runs on this thread

CtxScope::CtxScope(Ctx* c) : prev(t_scope) { t_scope = c; }
CtxScope::~CtxScope() { t_scope = prev; }

Ctx& ctx() {
    if (t_scope) return *t_scope;
    if (t_handle == 0) return default_ctx();
    Shared& s = shared();
    if (t_cached && t_epoch == s.epoch.load(std::memory_order_acquire)) return *t_cached;
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.contexts.find(t_handle);
    if (it == s.contexts.end()) { t_handle = 0; t_cached = nullptr; return default_ctx(); }
    t_cached = it->second;
    t_epoch = s.epoch.load(std::memory_order_acquire);
    return *t_cached;
}
std::mutex& ctx_mutex() { return ctx().mu; }

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return UZK_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = bytes + (bytes >> 3);   // 12.5 % head-room against regrowth
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        want = bytes;
        e = hipMalloc(&p, want);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();        // clear the runtime's sticky last error
        p = nullptr;
        set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return UZK_ERR_DEVICE;
    }
    cap = want;
    return UZK_OK;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

hipEvent_t Ctx::get_event() {
    if (!event_pool.empty()) {
        hipEvent_t e = event_pool.back();
        event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
void Ctx::prof_begin(const char* name) {
    ProfEntry pe;
    pe.name = name;
    pe.e0 = get_event();
    pe.e1 = get_event();
    (void)hipEventRecord(pe.e0, cur_stream ? cur_stream : stream);
    prof_pending.push_back(pe);
}
void Ctx::prof_end() {
    if (!prof_pending.empty()) (void)hipEventRecord(prof_pending.back().e1, cur_stream ? cur_stream : stream);
}
int Ctx::prof_collect() {
    if (prof_pending.empty()) return UZK_OK;
    UZK_HIP(hipStreamSynchronize(stream));
    if (stream2) UZK_HIP(hipStreamSynchronize(stream2));
    for (auto& pe : prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.e0, pe.e1) == hipSuccess) {
            auto& t = prof_totals[pe.name];
            t.first += ms;
            t.second += 1;
        }
        event_pool.push_back(pe.e0);
        event_pool.push_back(pe.e1);
    }
    prof_pending.clear();
    return UZK_OK;
}

// The device this process was last bound to by uzk_init: a lazy re-initialisation after uzk_shutdown
// returns to it instead of silently moving to device 0.
static int g_last_device = 0;

// compute units of `device` (Shared::mu held by the caller); the device becomes one uzk_shutdown synchronises
static int device_cus_locked(Shared& s, int device, int* cus) {
    auto it = s.num_cus.find(device);
    if (it == s.num_cus.end()) {
        int v = 0;
        UZK_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device));
        it = s.num_cus.emplace(device, v > 0 ? v : 256).first;
    }
    *cus = it->second;
    return UZK_OK;
}
// binds the process's default device (Shared::mu held by the caller)
static int bind_device_locked(Shared& s, int device) {
    UZK_HIP(hipSetDevice(device));
    int cus = 0;
    UZK_TRY(device_cus_locked(s, device, &cus));
    s.device = device;
    s.bound = true;
    g_last_device = device;
    return UZK_OK;
}

// Makes the calling thread's context usable: process bound to a device, HIP's per-thread current device set to it,
// the context's stream created.  Called with the context's mutex held.
int require_ready() {
    Shared& s = shared();
    Ctx& c = ctx();
    int device;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (!s.bound) {
            // lazy init (device 0, or the one uzk_init bound before a shutdown) so a plain library user need not call uzk_init
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
                set_error("no HIP device visible: the MI355X backend has no CPU fallback");
                return UZK_ERR_DEVICE;
            }
            UZK_TRY(bind_device_locked(s, g_last_device < n ? g_last_device : 0));
        }
        device = c.want_device >= 0 ? c.want_device : s.device;
        UZK_TRY(device_cus_locked(s, device, &c.num_cus));
    }
    // HIP's current device is per thread: a prover thread that never called uzk_init would otherwise
    // allocate and launch on device 0 while the streams and the SRS live on the context's device
    UZK_HIP(hipSetDevice(device));
    if (!c.ready) {
        UZK_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        c.device = device;
        c.ready = true;
    }
    return UZK_OK;
}

void devices_synchronize() {
    Shared& s = shared();
    std::vector<int> devs;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        for (auto& kv : s.num_cus) devs.push_back(kv.first);
    }
    for (int d : devs) { (void)hipSetDevice(d); (void)hipDeviceSynchronize(); }
}

// frees everything a context owns (its mutex held, or no other user left)
static void ctx_release(Ctx& c) {
    if (!c.ready) return;
    (void)hipSetDevice(c.device);
    (void)hipStreamSynchronize(c.stream);
    ntt_free_plans(c);
    g1ntt_free(c);
    srscheck_free(c);
    g2_free(c);
    g16_free(c);
    c.verify_ws.release();
    c.g16v_ws.release();
    c.ed_ws.release();
    c.codec_ws.release();
    c.shuffle_ws.release();
    c.match_ws.release();
    c.reveal_ws.release();
    c.reveal_z.release();
    c.ed_gen.release();
    c.ed_gen_ready = false;
    c.pairing_ws.release();
    msm_free(c);
    poly_free(c);
    c.ntt_scratch[0].release(); c.ntt_scratch[1].release(); c.ntt_io.release(); c.msm_scalars.release();
    if (c.msm_tail_host) { (void)hipHostFree(c.msm_tail_host); c.msm_tail_host = nullptr; c.msm_tail_cap = 0; }
    for (auto& pe : c.prof_pending) { (void)hipEventDestroy(pe.e0); (void)hipEventDestroy(pe.e1); }
    c.prof_pending.clear();
    for (auto e : c.event_pool) (void)hipEventDestroy(e);
    c.event_pool.clear();
    (void)hipStreamDestroy(c.stream);
    c.stream = nullptr;
    c.cur_stream = nullptr;
    c.ready = false;
    c.device = -1;
}

static const Fp* as_fp(const uint64_t* p) { return reinterpret_cast<const Fp*>(p); }

static void copy_tuning(const Ctx& from, Ctx& to);
int ctx_init_internal(Ctx& c, int device) {
    c.want_device = device;
    {
        std::lock_guard<std::mutex> lk(default_ctx().mu);
        copy_tuning(default_ctx(), c);
    }
    CtxScope scope(&c);
    std::lock_guard<std::mutex> lk(c.mu);
    return require_ready();
}
void ctx_release_internal(Ctx& c) {
    std::lock_guard<std::mutex> lk(c.mu);
    ctx_release(c);
}

}  // namespace uzk

using namespace uzk;

#define API_LOCK std::lock_guard<std::mutex> _lk(ctx_mutex())

extern "C" {

#ifndef UZK_SRC_HASH
#define UZK_SRC_HASH "unstamped"
#endif
const char* uzk_version(void) { return "uzkge-amd 0.3 (gfx950) src:" UZK_SRC_HASH; }
const char* uzk_last_error(void) { return g_err; }

int uzk_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} catch (...) { return uzk::on_exception("uzk_device_count"); }

int uzk_init(int device) try {
    API_LOCK;
    Shared& s = shared();
    {
        std::lock_guard<std::mutex> lk(s.mu);
        if (s.bound && s.device != device) {
            set_error("uzk_init(%d): already bound to device %d (one process per GPU)", device, s.device);
            return UZK_ERR_PARAMETER;
        }
        if (!s.bound) {
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
                set_error("no HIP device visible: the MI355X backend has no CPU fallback");
                return UZK_ERR_DEVICE;
            }
            if (device < 0 || device >= n) {
                set_error("uzk_init(%d): %d device(s) visible", device, n);
                return UZK_ERR_PARAMETER;
            }
            UZK_TRY(bind_device_locked(s, device));
        }
    }
    return require_ready();
} catch (...) { return uzk::on_exception("uzk_init"); }

// Frees every context (the default one and those of uzk_ctx_create), every SRS and table, and unbinds the device.
// No other thread may be inside the library.  Threads that had made a destroyed context current fall back to the
// default context on their next call (the handle no longer resolves).  Memory from uzk_dev_alloc / uzk_host_alloc
// belongs to the caller and is not touched.
int uzk_shutdown(void) try {
    Shared& s = shared();
    coalesce_release_all();                // shared provers, their workspaces and internal contexts
    sharded_release_all();                 // sharded SRSs: their chunks' contexts and registry entries
    prover_release_all();                  // circuits and provers own device memory (takes Shared::mu itself)
    vf_release_all();                      // verifier keys
    g2_release_all();                      // G2 bases
    rcs_release_all();                     // reveal circuits, with the Groth16 keys they hold
    g16_release_all();                     // Groth16 proving keys
    g16v_release_all();                    // Groth16 verifying keys
    remark_release_all();                  // remask keys
    std::lock_guard<std::mutex> lk(s.mu);
    if (!s.bound) return UZK_OK;
    ctx_release(default_ctx());
    for (auto& kv : s.contexts) { ctx_release(*kv.second); delete kv.second; }
    s.contexts.clear();
    s.epoch.fetch_add(1, std::memory_order_acq_rel);
    t_handle = 0;
    t_cached = nullptr;
    for (auto& kv : s.srs) {
        (void)hipSetDevice(kv.second.device);
        if (kv.second.owned && kv.second.d_points) (void)hipFree(kv.second.d_points);
        if (kv.second.d_table) (void)hipFree(kv.second.d_table);
    }
    s.srs.clear();
    s.num_cus.clear();
    s.bound = false;
    s.device = -1;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_shutdown"); }

/* ---- contexts ------------------------------------------------------------------------------- */
// the experiment switches and the forced window width travel with the creator: a tool that tunes the default context
// and then starts prover threads measures what it configured
namespace uzk {
static void copy_tuning(const Ctx& from, Ctx& to) {
    to.msm_window_bits = from.msm_window_bits;
    to.tune_no_precompute = from.tune_no_precompute; to.tune_ntt_tile = from.tune_ntt_tile; to.tune_ntt_two_pass = from.tune_ntt_two_pass; to.tune_small = from.tune_small;
    to.tune_chunk_log = from.tune_chunk_log; to.tune_verify_transcript = from.tune_verify_transcript; to.tune_stream_log = from.tune_stream_log; to.tune_stream_min_log = from.tune_stream_min_log;
    to.tune_seg_sort = from.tune_seg_sort; to.tune_arith29 = from.tune_arith29;
    to.tune_msm_taper = from.tune_msm_taper;
}
}  // namespace uzk
int uzk_ctx_create(uint64_t* ctx_out) try {
    if (!ctx_out) { set_error("uzk_ctx_create: null pointer"); return UZK_ERR_PARAMETER; }
    Ctx* c = new Ctx();
    {
        API_LOCK;                                      // binds the device through the caller's current context
        int rc = require_ready();
        if (rc != UZK_OK) { delete c; return rc; }
        copy_tuning(ctx(), *c);
    }
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    const uint64_t h = s.next_ctx++;
    s.contexts[h] = c;
    *ctx_out = h;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_create"); }
// A context on a named device: one process can then drive several GPUs -- a pool of prover threads, each with a context (and its
// circuits and provers) on its own device, or the point chunks of one MSM (uzk_msm_g1_sharded).  uzk_init keeps its meaning: the
// device of the default context and of uzk_ctx_create.
int uzk_ctx_create_on(int device, uint64_t* ctx_out) try {
    if (!ctx_out) { set_error("uzk_ctx_create_on: null pointer"); return UZK_ERR_PARAMETER; }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device visible: the MI355X backend has no CPU fallback"); return UZK_ERR_DEVICE; }
    if (device < 0 || device >= n) { set_error("uzk_ctx_create_on(%d): %d device(s) visible", device, n); return UZK_ERR_PARAMETER; }
    Ctx* c = new Ctx();
    {
        API_LOCK;
        copy_tuning(ctx(), *c);
    }
    c->want_device = device;
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    const uint64_t h = s.next_ctx++;
    s.contexts[h] = c;
    *ctx_out = h;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_create_on"); }
int uzk_ctx_device(uint64_t handle, int* device_out) try {
    if (!device_out) { set_error("uzk_ctx_device: null pointer"); return UZK_ERR_PARAMETER; }
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    Ctx* c = nullptr;
    if (handle == 0) c = &default_ctx();
    else {
        auto it = s.contexts.find(handle);
        if (it == s.contexts.end()) { set_error("uzk_ctx_device: unknown context %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
        c = it->second;
    }
    *device_out = c->ready ? c->device : (c->want_device >= 0 ? c->want_device : (s.bound ? s.device : g_last_device));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_device"); }
int uzk_ctx_set_current(uint64_t handle) try {
    if (handle == 0) { t_handle = 0; t_cached = nullptr; return UZK_OK; }
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.contexts.find(handle);
    if (it == s.contexts.end()) { set_error("uzk_ctx_set_current: unknown context %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    t_handle = handle;
    t_cached = it->second;
    t_epoch = s.epoch.load(std::memory_order_acquire);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_set_current"); }
int uzk_ctx_destroy(uint64_t handle) try {
    Shared& s = shared();
    Ctx* c = nullptr;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        auto it = s.contexts.find(handle);
        if (it == s.contexts.end()) { set_error("uzk_ctx_destroy: unknown context %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
        c = it->second;
        s.contexts.erase(it);
        s.epoch.fetch_add(1, std::memory_order_acq_rel);   // every thread's cached pointer is looked up again
    }
    if (t_handle == handle) { t_handle = 0; t_cached = nullptr; }
    { std::lock_guard<std::mutex> lk(c->mu); ctx_release(*c); }
    delete c;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_destroy"); }

int uzk_ctx_current(uint64_t* ctx_out) try {
    if (!ctx_out) { set_error("uzk_ctx_current: null pointer"); return UZK_ERR_PARAMETER; }
    (void)ctx();                                         // a handle whose context is gone resolves to the default context here
    *ctx_out = t_handle;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_current"); }
// The calling thread's current context waits (on the device: no host synchronisation) for everything queued so far on
// `other`.  Two contexts in one prover thread are two lanes with their own stream and workspaces: independent steps of a
// proof -- the coset FFTs of the wire polynomials and the commit of the same round, the two openings -- run side by side,
// and this is the edge between them.
int uzk_ctx_wait(uint64_t other) try {
    Ctx* cur = &ctx();
    Ctx* oth = nullptr;
    if (other == 0) oth = &default_ctx();
    else {
        Shared& s = shared();
        std::lock_guard<std::mutex> lk(s.mu);
        auto it = s.contexts.find(other);
        if (it == s.contexts.end()) { set_error("uzk_ctx_wait: unknown context %llu", (unsigned long long)other); return UZK_ERR_PARAMETER; }
        oth = it->second;
    }
    if (oth == cur) return UZK_OK;
    std::unique_lock<std::mutex> l1(cur->mu, std::defer_lock), l2(oth->mu, std::defer_lock);
    std::lock(l1, l2);                                   // both locks, in whatever order avoids a deadlock with a thread waiting the other way
    UZK_TRY(require_ready());
    if (!oth->ready) return UZK_OK;                      // nothing was ever queued there
    hipEvent_t ev = oth->get_event();
    struct Return { Ctx* c; hipEvent_t e; ~Return() { c->event_pool.push_back(e); } } back{oth, ev};   // on every path, errors included
    UZK_HIP(hipEventRecord(ev, oth->stream));
    UZK_HIP(hipStreamWaitEvent(cur->stream, ev, 0));     // the wait has captured this recording; a later re-record does not move it
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ctx_wait"); }

/* ---- device memory ----------------------------------------------------------------------------
 * What a host language needs to keep data resident between the *_device entry points without linking the HIP runtime
 * itself.  Copies and fills are ordered on the calling context's stream, i.e. with that context's kernels. */
int uzk_dev_alloc(size_t bytes, void** d_out) try {
    API_LOCK;
    if (!d_out) { set_error("uzk_dev_alloc: null pointer"); return UZK_ERR_PARAMETER; }
    *d_out = nullptr;
    UZK_TRY(require_ready());
    if (bytes == 0) return UZK_OK;
    hipError_t e = hipMalloc(d_out, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();        // the runtime keeps a failed call as its sticky "last error": the next launch check must not see it
        *d_out = nullptr;
        set_error("uzk_dev_alloc(%zu): %s", bytes, hipGetErrorString(e));
        return UZK_ERR_DEVICE;
    }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_dev_alloc"); }
// Waits for the calling context's stream first: work queued on it may still use the block.
int uzk_dev_free(void* d_ptr) try {
    API_LOCK;
    if (!d_ptr) return UZK_OK;
    UZK_TRY(require_ready());
    UZK_HIP(hipStreamSynchronize(ctx().stream));
    UZK_HIP(hipFree(d_ptr));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_dev_free"); }
int uzk_host_alloc(size_t bytes, void** h_out) try {
    API_LOCK;
    if (!h_out) { set_error("uzk_host_alloc: null pointer"); return UZK_ERR_PARAMETER; }
    *h_out = nullptr;
    UZK_TRY(require_ready());
    if (bytes == 0) return UZK_OK;
    hipError_t e = hipHostMalloc(h_out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *h_out = nullptr; set_error("uzk_host_alloc(%zu): %s", bytes, hipGetErrorString(e)); return UZK_ERR_DEVICE; }
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    s.pinned[*h_out] = bytes;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_host_alloc"); }
int uzk_host_free(void* h_ptr) try {
    API_LOCK;
    if (!h_ptr) return UZK_OK;
    UZK_TRY(require_ready());
    Shared& s = shared();
    size_t bytes = 0;
    {
        // the entry goes BEFORE the memory does: once hipHostFree has run, another context's uzk_host_alloc may be handed the same
        // address and register it -- an erase after the free would then remove the new block's entry
        std::lock_guard<std::mutex> lk(s.mu);
        auto it = s.pinned.find(h_ptr);
        if (it == s.pinned.end()) { set_error("uzk_host_free: %p is not a block of uzk_host_alloc", h_ptr); return UZK_ERR_PARAMETER; }
        bytes = it->second;
        s.pinned.erase(it);
    }
    hipError_t e = hipStreamSynchronize(ctx().stream);
    if (e == hipSuccess) e = hipHostFree(h_ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(s.mu);
        s.pinned[h_ptr] = bytes;            // still allocated: still pinned, still freeable
        set_error("uzk_host_free: %s", hipGetErrorString(e));
        return UZK_ERR_DEVICE;
    }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_host_free"); }
}  // extern "C"
namespace uzk {
// true when [p, p + bytes) lies inside a block of uzk_host_alloc
bool is_pinned_block(const void* p, size_t bytes) {
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.pinned.upper_bound(p);
    if (it == s.pinned.begin()) return false;
    --it;
    const char* base = static_cast<const char*>(it->first);
    const char* q = static_cast<const char*>(p);
    return q >= base && q + bytes <= base + it->second;
}
}  // namespace uzk
extern "C" {
static int dev_copy_common(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, int kind, const char* who) {
    if (kind != UZK_COPY_H2D && kind != UZK_COPY_D2H && kind != UZK_COPY_D2D) { set_error("%s: kind must be UZK_COPY_H2D / D2H / D2D", who); return UZK_ERR_PARAMETER; }
    if (width == 0 || rows == 0) return UZK_OK;
    if (!dst || !src) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    if (rows > 1 && (dpitch < width || spitch < width)) { set_error("%s: a pitch is smaller than the row width", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    const hipMemcpyKind k = kind == UZK_COPY_H2D ? hipMemcpyHostToDevice : kind == UZK_COPY_D2H ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (rows == 1 || (dpitch == width && spitch == width)) UZK_HIP(hipMemcpyAsync(dst, src, width * rows, k, c.stream));
    else UZK_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, k, c.stream));
    // D2H: the data is in `dst` on return.  H2D: `src` may be reused on return -- unless it is pinned memory of
    // uzk_host_alloc, whose uploads stay asynchronous (the caller keeps it unchanged until the next synchronising call).
    const size_t span = rows > 1 ? (rows - 1) * spitch + width : width;
    if (kind == UZK_COPY_D2H || (kind == UZK_COPY_H2D && !is_pinned_block(src, span))) UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}
int uzk_dev_copy(void* dst, const void* src, size_t bytes, int kind) try {
    API_LOCK;
    return dev_copy_common(dst, bytes, src, bytes, bytes, 1, kind, "uzk_dev_copy");
} catch (...) { return uzk::on_exception("uzk_dev_copy"); }
int uzk_dev_copy2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows, int kind) try {
    API_LOCK;
    return dev_copy_common(dst, dst_pitch, src, src_pitch, width, rows, kind, "uzk_dev_copy2d");
} catch (...) { return uzk::on_exception("uzk_dev_copy2d"); }
int uzk_dev_memset(void* d_dst, int byte, size_t bytes) try {
    API_LOCK;
    if (bytes == 0) return UZK_OK;
    if (!d_dst) { set_error("uzk_dev_memset: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    UZK_HIP(hipMemsetAsync(d_dst, byte, bytes, ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_dev_memset"); }
int uzk_dev_memset2d(void* d_dst, size_t pitch, int byte, size_t width, size_t rows) try {
    API_LOCK;
    if (width == 0 || rows == 0) return UZK_OK;
    if (!d_dst) { set_error("uzk_dev_memset2d: null pointer"); return UZK_ERR_PARAMETER; }
    if (rows > 1 && pitch < width) { set_error("uzk_dev_memset2d: pitch smaller than the row width"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    UZK_HIP(hipMemset2DAsync(d_dst, pitch, byte, width, rows, ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_dev_memset2d"); }

/* ---- SRS (process-wide registry: the bases are read-only and shared by every context) ------------ */
}  // extern "C"
namespace uzk {
uint64_t srs_insert(const Ctx::Srs& e) {
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    const uint64_t h = s.next_handle++;
    s.srs[h] = e;
    return h;
}
// copy of the registry entry (the pointers stay valid until uzk_srs_release / uzk_srs_precompute on that handle)
bool srs_lookup(uint64_t handle, Ctx::Srs* out) {
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.srs.find(handle);
    if (it == s.srs.end()) return false;
    *out = it->second;
    return true;
}
// removes the entry and hands it to the caller, who frees what it owns
bool srs_erase(uint64_t handle, Ctx::Srs* out) {
    Shared& s = shared();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.srs.find(handle);
    if (it == s.srs.end()) return false;
    *out = it->second;
    s.srs.erase(it);
    return true;
}
}  // namespace uzk
extern "C" {

int uzk_srs_register(const uzk_g1_affine* points, size_t n, uint64_t* handle_out) try {
    API_LOCK;
    if (!handle_out || (n > 0 && !points)) { set_error("uzk_srs_register: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    Ctx::Srs s;
    s.n = n;
    s.owned = true;
    s.device = c.device;
    if (n > 0) {
        UZK_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_points), n * sizeof(Affine)));
        UZK_HIP(hipMemcpyAsync(s.d_points, points, n * sizeof(Affine), hipMemcpyHostToDevice, c.stream));
        UZK_HIP(hipStreamSynchronize(c.stream));
    }
    *handle_out = srs_insert(s);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_register"); }

int uzk_srs_register_device(const void* d_points, size_t n, uint64_t* handle_out) try {
    API_LOCK;
    if (!handle_out || (n > 0 && !d_points)) { set_error("uzk_srs_register_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx::Srs s;
    s.n = n;
    s.owned = false;
    s.device = ctx().device;
    s.d_points = const_cast<Affine*>(static_cast<const Affine*>(d_points));
    *handle_out = srs_insert(s);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_register_device"); }

// The caller makes sure no context still runs an MSM over this handle.
int uzk_srs_release(uint64_t handle) try {
    API_LOCK;
    Ctx& c = ctx();
    Shared& sh = shared();
    Ctx::Srs e;
    {
        std::lock_guard<std::mutex> lk(sh.mu);
        auto it = sh.srs.find(handle);
        if (it == sh.srs.end()) { set_error("uzk_srs_release: unknown handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
        e = it->second;
        sh.srs.erase(it);
    }
    if (c.ready) (void)hipStreamSynchronize(c.stream);
    (void)hipSetDevice(e.device);
    if (e.owned && e.d_points) (void)hipFree(e.d_points);
    if (e.d_table) (void)hipFree(e.d_table);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_release"); }

// Build the table before contexts start using the handle concurrently (the entry is replaced, not versioned).
int uzk_srs_precompute(uint64_t handle, int window_bits) try {
    API_LOCK;
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    Ctx::Srs s;
    if (!srs_lookup(handle, &s)) { set_error("uzk_srs_precompute: unknown handle"); return UZK_ERR_PARAMETER; }
    if (window_bits != 0 && (window_bits < 4 || window_bits > 24)) {
        set_error("uzk_srs_precompute: window bits must be 0 (auto) or 4..24");
        return UZK_ERR_PARAMETER;
    }
    if (s.n == 0) return UZK_OK;
    if (s.device != c.device) { set_error("uzk_srs_precompute: the SRS lives on device %d, the calling context on device %d", s.device, c.device); return UZK_ERR_PARAMETER; }
    const int cb = msm_precompute_window_bits(s.n, window_bits);
    if (s.d_table && s.pre_c == cb) return UZK_OK;
    Affine* old_table = s.d_table;
    Affine* table = nullptr;
    uint32_t W = 0;
    UZK_TRY(msm_build_table(c, s.d_points, s.n, cb, &table, &W));
    {
        Shared& sh = shared();
        std::lock_guard<std::mutex> lk(sh.mu);
        auto it = sh.srs.find(handle);
        if (it == sh.srs.end()) { (void)hipFree(table); set_error("uzk_srs_precompute: handle released meanwhile"); return UZK_ERR_PARAMETER; }
        it->second.d_table = table;
        it->second.pre_c = cb;
        it->second.pre_W = W;
    }
    if (old_table) { (void)hipStreamSynchronize(c.stream); (void)hipFree(old_table); }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_precompute"); }

int uzk_srs_len(uint64_t handle, size_t* n_out) try {
    Ctx::Srs s;
    if (!n_out || !srs_lookup(handle, &s)) { set_error("uzk_srs_len: unknown handle"); return UZK_ERR_PARAMETER; }
    *n_out = s.n;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_len"); }

/* ---- MSM ---------------------------------------------------------------------------------- */
static int msm_checked(uint64_t srs_handle, size_t offset, size_t n, Ctx::Srs* srs_out) {
    if (!srs_lookup(srs_handle, srs_out)) { set_error("msm: unknown SRS handle %llu", (unsigned long long)srs_handle); return UZK_ERR_PARAMETER; }
    if (offset > srs_out->n || n > srs_out->n - offset) {
        // KZG commit: degree + 1 > SRS length (kzg_poly_commitment.rs:283-285)
        set_error("msm: offset %zu + n %zu exceeds SRS length %zu", offset, n, srs_out->n);
        return UZK_ERR_DEGREE;
    }
    if (srs_out->device != ctx().device) { set_error("msm: the SRS lives on device %d, the calling context on device %d", srs_out->device, ctx().device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}
}  // extern "C"
namespace uzk {
// general mode unless the handle carries a window table
int msm_dispatch_view(const Ctx::Srs& s, size_t offset, const ScalarView& sv, size_t n, uint32_t batch, Jac* out) {
    Ctx& c = ctx();
    if (s.d_table && !c.tune_no_precompute)
        return msm_run(c, s.d_table, sv, n, batch, out, s.pre_c, (uint32_t)s.n, (uint32_t)offset);
    return msm_run(c, s.d_points + offset, sv, n, batch, out, 0, 0, 0);
}
}  // namespace uzk
extern "C" {
static int msm_dispatch_one(const Ctx::Srs& s, size_t offset, const Fp* d_scalars, size_t n, uint32_t batch, Jac* out) {
    Ctx& c = ctx();
    // one vector of more than 2^24 points over plain bases: chunks of 2^24 into one bucket set (msm_run_chunked)
    if (batch == 1 && n > ((size_t)1 << 24) && !(s.d_table && !c.tune_no_precompute) && c.tune_chunk_log >= 25)
        return msm_run_chunked(c, s.d_points + offset, d_scalars, n, out);
    return msm_dispatch_view(s, offset, ScalarView::dense(d_scalars, n), n, batch, out);
}
// The sort indexes (point, window) pairs with 31 bits, so one pass handles at most 2^26 points per
// scalar vector (2^26 * 16 windows); longer inputs are cut into point chunks whose partial sums are
// folded on the host -- the same decomposition the multi-GPU path uses across ranks.
static int msm_dispatch(const Ctx::Srs& s, size_t offset, const Fp* d_scalars, size_t n, uint32_t batch, Jac* out) {
    const size_t kChunk = (size_t)1 << ctx().tune_chunk_log;
    if (n <= kChunk || batch != 1) return msm_dispatch_one(s, offset, d_scalars, n, batch, out);
    XYZZ acc = xyzz_inf();
    for (size_t lo = 0; lo < n; lo += kChunk) {
        const size_t len = std::min(kChunk, n - lo);
        Jac part;
        UZK_TRY(msm_dispatch_one(s, offset + lo, d_scalars + lo, len, 1, &part));
        XYZZ q = xyzz_from_jac(part);
        xyzz_add(acc, q);
    }
    *out = xyzz_to_jac(acc);
    return UZK_OK;
}

int uzk_msm_g1_device(uint64_t srs_handle, size_t offset, const void* d_scalars_mont, size_t n, uzk_g1_jac* out) try {
    API_LOCK;
    if (!out || (n > 0 && !d_scalars_mont)) { set_error("uzk_msm_g1_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx::Srs srs;
    UZK_TRY(msm_checked(srs_handle, offset, n, &srs));
    Jac r;
    UZK_TRY(msm_dispatch(srs, offset, static_cast<const Fp*>(d_scalars_mont), n, 1, &r));
    std::memcpy(out, &r, sizeof r);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_g1_device"); }

int uzk_msm_g1(uint64_t srs_handle, size_t offset, const uint64_t* scalars_mont, size_t n, uzk_g1_jac* out) try {
    API_LOCK;
    if (!out || (n > 0 && !scalars_mont)) { set_error("uzk_msm_g1: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    Ctx::Srs srs;
    UZK_TRY(msm_checked(srs_handle, offset, n, &srs));
    Jac r = jac_inf();
    const bool table = srs.d_table && !c.tune_no_precompute;
    if (n >= ((size_t)1 << c.tune_stream_min_log) && n <= ((size_t)1 << c.tune_chunk_log) && !table && c.tune_stream_log >= 0) {
        // large general-mode MSM: the scalars arrive in point chunks under the previous chunk's accumulation (msm.hip)
        UZK_TRY(msm_run_streamed(c, srs.d_points + offset, as_fp(scalars_mont), n, &r));
    } else if (n > 0) {
        UZK_TRY(c.msm_scalars.reserve(n * sizeof(Fp)));
        UZK_HIP(hipMemcpyAsync(c.msm_scalars.p, scalars_mont, n * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
        UZK_TRY(msm_dispatch(srs, offset, c.msm_scalars.as<Fp>(), n, 1, &r));
    }
    std::memcpy(out, &r, sizeof r);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_g1"); }

int uzk_msm_g1_batch_device(uint64_t srs_handle, size_t offset, const void* d_scalars_mont, size_t n, uint32_t batch,
                            uzk_g1_jac* out) try {
    API_LOCK;
    if (batch > 0 && (!out || (n > 0 && !d_scalars_mont))) { set_error("uzk_msm_g1_batch_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx::Srs srs;
    UZK_TRY(msm_checked(srs_handle, offset, n, &srs));
    std::vector<Jac> r(batch);
    UZK_TRY(msm_dispatch(srs, offset, static_cast<const Fp*>(d_scalars_mont), n, batch, r.data()));
    if (batch) std::memcpy(out, r.data(), (size_t)batch * sizeof(Jac));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_g1_batch_device"); }

int uzk_msm_g1_batch(uint64_t srs_handle, size_t offset, const uint64_t* scalars_mont, size_t n, uint32_t batch,
                     uzk_g1_jac* out) try {
    API_LOCK;
    if (batch > 0 && (!out || (n > 0 && !scalars_mont))) { set_error("uzk_msm_g1_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    Ctx::Srs srs;
    UZK_TRY(msm_checked(srs_handle, offset, n, &srs));
    std::vector<Jac> r(batch, jac_inf());
    if (n > 0 && batch > 0) {
        const size_t bytes = (size_t)n * batch * sizeof(Fp);
        UZK_TRY(c.msm_scalars.reserve(bytes));
        UZK_HIP(hipMemcpyAsync(c.msm_scalars.p, scalars_mont, bytes, hipMemcpyHostToDevice, c.stream));
        UZK_TRY(msm_dispatch(srs, offset, c.msm_scalars.as<Fp>(), n, batch, r.data()));
    }
    if (batch) std::memcpy(out, r.data(), (size_t)batch * sizeof(Jac));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_g1_batch"); }

// out[b] = sum_{i<n} d_scalars[b*stride + i] * SRS[offset + i] + sum_{j<tail_n} tail[b*tail_n + j] * SRS[offset + n + j]
int uzk_msm_g1_batch_tail_device(uint64_t srs_handle, size_t offset, const void* d_scalars_mont, size_t stride, size_t n, uint32_t batch,
                                 const void* tail_scalars_mont, uint32_t tail_n, int tail_on_device, uzk_g1_jac* out) try {
    API_LOCK;
    if (batch > 0 && (!out || (n > 0 && !d_scalars_mont) || (tail_n > 0 && !tail_scalars_mont))) { set_error("uzk_msm_g1_batch_tail_device: null pointer"); return UZK_ERR_PARAMETER; }
    if (batch > 1 && stride < n) { set_error("uzk_msm_g1_batch_tail_device: stride %zu smaller than n %zu", stride, n); return UZK_ERR_PARAMETER; }
    if (tail_n > 4096) { set_error("uzk_msm_g1_batch_tail_device: tail_n %u exceeds 4096", tail_n); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    const size_t total = n + tail_n;
    Ctx::Srs srs;
    UZK_TRY(msm_checked(srs_handle, offset, total, &srs));
    if (total > ((size_t)1 << c.tune_chunk_log)) { set_error("uzk_msm_g1_batch_tail_device: n + tail_n = %zu exceeds one sort pass (2^%d points)", total, c.tune_chunk_log); return UZK_ERR_PARAMETER; }
    if (batch == 0) return UZK_OK;
    ScalarView sv;
    sv.main = static_cast<const Fp*>(d_scalars_mont);
    sv.stride = stride;
    sv.n_main = (uint32_t)n;
    sv.tail_n = tail_n;
    if (tail_n && tail_on_device) sv.tail = static_cast<const Fp*>(tail_scalars_mont);
    else if (tail_n) {
        // a few dozen elements: copied into pinned, device-visible memory the digit kernel reads directly; the call returns
        // after the window sums have arrived, so one slot per context is enough
        const size_t bytes = (size_t)batch * tail_n * sizeof(Fp);
        if (c.msm_tail_cap < bytes) {
            if (c.msm_tail_host) { UZK_HIP(hipStreamSynchronize(c.stream)); (void)hipHostFree(c.msm_tail_host); c.msm_tail_host = nullptr; c.msm_tail_cap = 0; }
            const size_t cap = std::max<size_t>(bytes, 1 << 14);
            UZK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.msm_tail_host), cap, hipHostMallocDefault));
            c.msm_tail_cap = cap;
        }
        std::memcpy(c.msm_tail_host, tail_scalars_mont, bytes);
        sv.tail = c.msm_tail_host;
    }
    std::vector<Jac> r(batch);
    UZK_TRY(msm_dispatch_view(srs, offset, sv, total, batch, r.data()));
    std::memcpy(out, r.data(), (size_t)batch * sizeof(Jac));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_g1_batch_tail_device"); }

int uzk_msm_g1_raw(const uzk_g1_affine* points, const uint64_t* scalars_mont, size_t n, uzk_g1_jac* out) try {
    if (!out || (n > 0 && (!points || !scalars_mont))) { set_error("uzk_msm_g1_raw: null pointer"); return UZK_ERR_PARAMETER; }
    uint64_t h = 0;
    UZK_TRY(uzk_srs_register(points, n, &h));
    int rc = uzk_msm_g1(h, 0, scalars_mont, n, out);
    (void)uzk_srs_release(h);
    return rc;
} catch (...) { return uzk::on_exception("uzk_msm_g1_raw"); }

int uzk_g1_fold(const uzk_g1_jac* partials, size_t count, uzk_g1_jac* out) try {
    if (!out || (count > 0 && !partials)) { set_error("uzk_g1_fold: null pointer"); return UZK_ERR_PARAMETER; }
    h64::J acc = h64::j_inf();
    for (size_t i = 0; i < count; ++i) {
        Jac j;
        std::memcpy(&j, &partials[i], sizeof j);
        acc = h64::j_add(acc, h64::j_from(j));
    }
    const Jac r = h64::j_to(acc);
    std::memcpy(out, &r, sizeof r);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g1_fold"); }

int uzk_g1_to_affine(const uzk_g1_jac* p, uzk_g1_affine* out) try {
    if (!p || !out) { set_error("uzk_g1_to_affine: null pointer"); return UZK_ERR_PARAMETER; }
    Jac j;
    std::memcpy(&j, p, sizeof j);
    Affine a = jac_to_affine_host(j);
    std::memcpy(out, &a, sizeof a);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g1_to_affine"); }

/* ---- G2: bases, MSM, fold, affine map ------------------------------------------------------- */
static int g2_checked(const char* who, uint64_t handle, size_t offset, size_t n, const G2Affine** d_points) {
    size_t len = 0;
    int device = 0;
    if (!g2_lookup(handle, d_points, &len, &device)) { set_error("%s: unknown G2 handle %llu", who, (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    if (offset > len || n > len - offset) { set_error("%s: offset %zu + n %zu exceeds the %zu registered points", who, offset, n, len); return UZK_ERR_DEGREE; }
    if (n > ((size_t)1 << UZK_MSM_G2_MAX_LOG2)) { set_error("%s: n %zu exceeds 2^%d points", who, n, UZK_MSM_G2_MAX_LOG2); return UZK_ERR_DEGREE; }
    if (device != ctx().device) { set_error("%s: the bases live on device %d, the calling context on device %d", who, device, ctx().device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

int uzk_g2_register(const uzk_g2_affine* points, size_t n, uint64_t* handle_out) try {
    API_LOCK;
    if (!handle_out || (n > 0 && !points)) { set_error("uzk_g2_register: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return g2_register(ctx(), reinterpret_cast<const G2Affine*>(points), n, handle_out);
} catch (...) { return uzk::on_exception("uzk_g2_register"); }

// The caller makes sure no context still runs an MSM over this handle.
int uzk_g2_release(uint64_t handle) try {
    API_LOCK;
    if (!g2_lookup(handle, nullptr, nullptr, nullptr)) { set_error("uzk_g2_release: unknown handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    Ctx& c = ctx();
    if (c.ready) (void)hipStreamSynchronize(c.stream);
    if (!g2_release(handle)) { set_error("uzk_g2_release: unknown handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g2_release"); }

int uzk_g2_len(uint64_t handle, size_t* n_out) try {
    if (!n_out || !g2_lookup(handle, nullptr, n_out, nullptr)) { set_error("uzk_g2_len: unknown handle"); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g2_len"); }

int uzk_msm_g2_batch_device(uint64_t handle, size_t offset, const void* d_scalars_mont, size_t n, uint32_t batch, uzk_g2_jac* out) try {
    API_LOCK;
    if (batch > 0 && (!out || (n > 0 && !d_scalars_mont))) { set_error("uzk_msm_g2_batch_device: null pointer"); return UZK_ERR_PARAMETER; }
    if (!g2_lookup(handle, nullptr, nullptr, nullptr)) { set_error("uzk_msm_g2_batch_device: unknown G2 handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    const G2Affine* pts = nullptr;
    UZK_TRY(g2_checked("uzk_msm_g2_batch_device", handle, offset, n, &pts));
    return g2_msm_run(ctx(), pts + offset, static_cast<const Fp*>(d_scalars_mont), n, batch, reinterpret_cast<G2Jac*>(out));
} catch (...) { return uzk::on_exception("uzk_msm_g2_batch_device"); }

int uzk_msm_g2_batch_finish(uint64_t handle, size_t offset, const void* d_scalars_mont, size_t n, uint32_t batch, uzk_g2_affine* out, void* d_out) try {
    API_LOCK;
    if (!out && !d_out) { set_error("uzk_msm_g2_batch_finish: no output asked for"); return UZK_ERR_PARAMETER; }
    if (batch > 0 && n > 0 && !d_scalars_mont) { set_error("uzk_msm_g2_batch_finish: null pointer"); return UZK_ERR_PARAMETER; }
    if (!g2_lookup(handle, nullptr, nullptr, nullptr)) { set_error("uzk_msm_g2_batch_finish: unknown G2 handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    const G2Affine* pts = nullptr;
    UZK_TRY(g2_checked("uzk_msm_g2_batch_finish", handle, offset, n, &pts));
    Ctx& c = ctx();
    UZK_TRY(g2_msm_finish_run(c, pts + offset, static_cast<const Fp*>(d_scalars_mont), n, batch, reinterpret_cast<G2Affine*>(out), static_cast<G2Affine*>(d_out)));
    UZK_HIP(hipStreamSynchronize(c.stream));          // d_out is complete when the call returns
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_g2_batch_finish"); }

int uzk_msm_g2_batch(uint64_t handle, size_t offset, const uint64_t* scalars_mont, size_t n, uint32_t batch, uzk_g2_jac* out) try {
    API_LOCK;
    if (batch > 0 && (!out || (n > 0 && !scalars_mont))) { set_error("uzk_msm_g2_batch: null pointer"); return UZK_ERR_PARAMETER; }
    if (!g2_lookup(handle, nullptr, nullptr, nullptr)) { set_error("uzk_msm_g2_batch: unknown G2 handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    const G2Affine* pts = nullptr;
    UZK_TRY(g2_checked("uzk_msm_g2_batch", handle, offset, n, &pts));
    const size_t bytes = n * (size_t)batch * sizeof(Fp);
    if (bytes > 0) {
        UZK_TRY(c.msm_scalars.reserve(bytes));
        UZK_HIP(hipMemcpyAsync(c.msm_scalars.p, scalars_mont, bytes, hipMemcpyHostToDevice, c.stream));
    }
    return g2_msm_run(c, pts + offset, c.msm_scalars.as<Fp>(), n, batch, reinterpret_cast<G2Jac*>(out));
} catch (...) { return uzk::on_exception("uzk_msm_g2_batch"); }

int uzk_msm_g2(uint64_t handle, size_t offset, const uint64_t* scalars_mont, size_t n, uzk_g2_jac* out) try {
    if (!out) { set_error("uzk_msm_g2: null pointer"); return UZK_ERR_PARAMETER; }
    return uzk_msm_g2_batch(handle, offset, scalars_mont, n, 1, out);
} catch (...) { return uzk::on_exception("uzk_msm_g2"); }

int uzk_g2_fold(const uzk_g2_jac* partials, size_t count, uzk_g2_jac* out) try {
    if (!out || (count > 0 && !partials)) { set_error("uzk_g2_fold: null pointer"); return UZK_ERR_PARAMETER; }
    g2_fold_host(reinterpret_cast<const G2Jac*>(partials), count, reinterpret_cast<G2Jac*>(out));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g2_fold"); }

int uzk_g2_to_affine(const uzk_g2_jac* p, uzk_g2_affine* out) try {
    if (!p || !out) { set_error("uzk_g2_to_affine: null pointer"); return UZK_ERR_PARAMETER; }
    g2_to_affine_host(reinterpret_cast<const G2Jac*>(p), reinterpret_cast<G2Affine*>(out));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g2_to_affine"); }

/* ---- Groth16: proving keys, the witness map, the batched prover ----------------------------- */
int uzk_g16_key_create(const uzk_g16_key_desc* desc, uint64_t* key_out) try {
    uint64_t domain = 0;
    if (!key_out) { set_error("uzk_g16_key_create: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(g16_key_check(desc, &domain));            // host-only: before the device is touched
    API_LOCK;
    UZK_TRY(require_ready());
    return g16_key_create(ctx(), desc, key_out);
} catch (...) { return uzk::on_exception("uzk_g16_key_create"); }

int uzk_g16_key_release(uint64_t key) try {
    API_LOCK;
    if (!g16_key_known(key, nullptr, nullptr, nullptr, nullptr, nullptr)) { set_error("uzk_g16_key_release: unknown handle %llu", (unsigned long long)key); return UZK_ERR_PARAMETER; }
    Ctx& c = ctx();
    if (c.ready) (void)hipStreamSynchronize(c.stream);
    if (!g16_key_release(key)) { set_error("uzk_g16_key_release: unknown handle %llu", (unsigned long long)key); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g16_key_release"); }

int uzk_g16_key_info(uint64_t key, uint32_t* n_vars_out, uint32_t* n_inputs_out, uint32_t* n_constraints_out, uint64_t* domain_out, int* device_out) try {
    if (!g16_key_known(key, n_vars_out, n_inputs_out, n_constraints_out, domain_out, device_out)) { set_error("uzk_g16_key_info: unknown handle %llu", (unsigned long long)key); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g16_key_info"); }

static int g16_checked(const char* who, uint64_t key) {
    int device = 0;
    if (!g16_key_known(key, nullptr, nullptr, nullptr, nullptr, &device)) { set_error("%s: unknown key handle %llu", who, (unsigned long long)key); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    if (device != ctx().device) { set_error("%s: the key lives on device %d, the calling context on device %d", who, device, ctx().device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

int uzk_g16_h_device(uint64_t key, const void* d_z, uint32_t batch, void* d_h) try {
    API_LOCK;
    if (batch == 0) { set_error("uzk_g16_h_device: batch is 0"); return UZK_ERR_PARAMETER; }
    if (!d_z || !d_h) { set_error("uzk_g16_h_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(g16_checked("uzk_g16_h_device", key));
    return g16_h_run(ctx(), key, static_cast<const Fp*>(d_z), batch, static_cast<Fp*>(d_h));
} catch (...) { return uzk::on_exception("uzk_g16_h_device"); }

// the checks of every prover entry; the outputs are the caller's to check
static int g16_prove_checked(const char* who, uint64_t key, const void* z, bool on_device, const uint64_t* r, const uint64_t* s, uint32_t batch) {
    if (batch == 0) { set_error("%s: batch is 0", who); return UZK_ERR_PARAMETER; }
    if (!z || !r || !s) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    uint32_t m = 0;
    if (!g16_key_known(key, &m, nullptr, nullptr, nullptr, nullptr)) { set_error("%s: unknown key handle %llu", who, (unsigned long long)key); return UZK_ERR_PARAMETER; }
    if (!on_device) {
        const Fp one = Fr::one();
        for (uint32_t b = 0; b < batch; ++b)
            if (std::memcmp(static_cast<const Fp*>(z) + (size_t)b * m, &one, sizeof one) != 0) { set_error("%s: assignment %u does not start with the constant one", who, b); return UZK_ERR_PARAMETER; }
    }
    return g16_checked(who, key);
}
static int g16_prove_common(const char* who, uint64_t key, const void* z, bool on_device, const uint64_t* r, const uint64_t* s, uint32_t batch, uzk_g16_proof* out) {
    if (batch > 0 && !out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(g16_prove_checked(who, key, z, on_device, r, s, batch));
    return g16_prove_run(ctx(), key, static_cast<const Fp*>(z), on_device, as_fp(r), as_fp(s), batch, out);
}
int uzk_g16_prove_batch(uint64_t key, const uint64_t* z_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t batch, uzk_g16_proof* out) try {
    API_LOCK;
    return g16_prove_common("uzk_g16_prove_batch", key, z_mont, false, r_mont, s_mont, batch, out);
} catch (...) { return uzk::on_exception("uzk_g16_prove_batch"); }
int uzk_g16_prove_batch_device(uint64_t key, const void* d_z_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t batch, uzk_g16_proof* out) try {
    API_LOCK;
    return g16_prove_common("uzk_g16_prove_batch_device", key, d_z_mont, true, r_mont, s_mont, batch, out);
} catch (...) { return uzk::on_exception("uzk_g16_prove_batch_device"); }
int uzk_g16_prove_batch_finish(uint64_t key, const void* z_mont, int z_on_device, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t batch,
                               uzk_g16_proof* proofs_out, uint8_t* blobs_out, void* d_blobs_out) try {
    static const char* who = "uzk_g16_prove_batch_finish";
    API_LOCK;
    if (!proofs_out && !blobs_out && !d_blobs_out) { set_error("%s: no output asked for", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(g16_prove_checked(who, key, z_mont, z_on_device != 0, r_mont, s_mont, batch));
    return g16_prove_finish_run(ctx(), key, static_cast<const Fp*>(z_mont), z_on_device != 0, as_fp(r_mont), as_fp(s_mont), batch, proofs_out, blobs_out,
                                static_cast<uint8_t*>(d_blobs_out));
} catch (...) { return uzk::on_exception("uzk_g16_prove_batch_finish"); }

/* ---- NTT ---------------------------------------------------------------------------------- */
int uzk_domain_supported(uint64_t n) try { return domain_supported(n) ? 1 : 0; } catch (...) { return uzk::on_exception("uzk_domain_supported"); }

int uzk_domain_group_gen(uint64_t n, uint64_t out_mont[4]) try {
    if (!out_mont) { set_error("uzk_domain_group_gen: null pointer"); return UZK_ERR_PARAMETER; }
    if (!domain_exists(n)) { set_error("no evaluation domain of size %llu", (unsigned long long)n); return UZK_ERR_FFT; }
    Fp w = fr_root_of_unity(n);
    std::memcpy(out_mont, &w, sizeof w);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_domain_group_gen"); }

static int ntt_device_common(const void* d_in, void* d_out, uint64_t n, uint32_t batch, int inverse,
                             const uint64_t* coset_shift_mont, int sync) {
    if (!domain_supported(n)) {
        set_error("no evaluation domain of size %llu (need 2^k, k <= %d, or 3 * 2^k, k <= %d)", (unsigned long long)n, UZK_NTT_MAX_LOG2, UZK_NTT_MAX_LOG2_MIXED);
        return UZK_ERR_FFT;
    }
    if (!d_in || !d_out) { set_error("uzk_ntt_fr*_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(ntt_run(c, static_cast<const Fp*>(d_in), static_cast<Fp*>(d_out), n, inverse != 0,
                    coset_shift_mont ? as_fp(coset_shift_mont) : nullptr, batch));
    if (sync) UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}
static int ntt_host_common(uint64_t* data, uint64_t n, uint32_t batch, int inverse, const uint64_t* coset_shift_mont) {
    if (!domain_supported(n)) {
        set_error("no evaluation domain of size %llu (need 2^k, k <= %d, or 3 * 2^k, k <= %d)", (unsigned long long)n, UZK_NTT_MAX_LOG2, UZK_NTT_MAX_LOG2_MIXED);
        return UZK_ERR_FFT;
    }
    if (!data) { set_error("uzk_ntt_fr*: null pointer"); return UZK_ERR_PARAMETER; }
    if (batch == 0) return UZK_OK;
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    const size_t bytes = (size_t)n * batch * sizeof(Fp);
    UZK_TRY(c.ntt_io.reserve(bytes));
    UZK_HIP(hipMemcpyAsync(c.ntt_io.p, data, bytes, hipMemcpyHostToDevice, c.stream));
    UZK_TRY(ntt_run(c, c.ntt_io.as<Fp>(), c.ntt_io.as<Fp>(), n, inverse != 0,
                    coset_shift_mont ? as_fp(coset_shift_mont) : nullptr, batch));
    UZK_HIP(hipMemcpyAsync(data, c.ntt_io.p, bytes, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int uzk_ntt_fr_device(const void* d_in, void* d_out, uint64_t n, int inverse, const uint64_t* coset_shift_mont, int sync) try {
    API_LOCK;
    return ntt_device_common(d_in, d_out, n, 1, inverse, coset_shift_mont, sync);
} catch (...) { return uzk::on_exception("uzk_ntt_fr_device"); }
int uzk_ntt_fr_batch_device(const void* d_in, void* d_out, uint64_t n, uint32_t batch, int inverse,
                            const uint64_t* coset_shift_mont, int sync) try {
    API_LOCK;
    return ntt_device_common(d_in, d_out, n, batch, inverse, coset_shift_mont, sync);
} catch (...) { return uzk::on_exception("uzk_ntt_fr_batch_device"); }
int uzk_ntt_fr_batch_strided_device(const void* d_in, uint64_t in_stride, void* d_out, uint64_t out_stride, uint64_t n, uint32_t batch,
                                    int inverse, const uint64_t* coset_shift_mont, int sync) try {
    API_LOCK;
    if (!domain_supported(n)) {
        set_error("no evaluation domain of size %llu (need 2^k, k <= %d, or 3 * 2^k, k <= %d)", (unsigned long long)n, UZK_NTT_MAX_LOG2, UZK_NTT_MAX_LOG2_MIXED);
        return UZK_ERR_FFT;
    }
    if (!d_in || !d_out) { set_error("uzk_ntt_fr_batch_strided_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(ntt_run(c, static_cast<const Fp*>(d_in), static_cast<Fp*>(d_out), n, inverse != 0,
                    coset_shift_mont ? as_fp(coset_shift_mont) : nullptr, batch, in_stride, out_stride));
    if (sync) UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ntt_fr_batch_strided_device"); }
int uzk_ntt_fr(uint64_t* data, uint64_t n, int inverse, const uint64_t* coset_shift_mont) try {
    API_LOCK;
    return ntt_host_common(data, n, 1, inverse, coset_shift_mont);
} catch (...) { return uzk::on_exception("uzk_ntt_fr"); }
int uzk_ntt_fr_batch(uint64_t* data, uint64_t n, uint32_t batch, int inverse, const uint64_t* coset_shift_mont) try {
    API_LOCK;
    return ntt_host_common(data, n, batch, inverse, coset_shift_mont);
} catch (...) { return uzk::on_exception("uzk_ntt_fr_batch"); }

/* ---- NTT over G1 --------------------------------------------------------------------------- */
static bool g1_ntt_supported(uint64_t n) { return n != 0 && (n & (n - 1)) == 0 && n <= (1ull << UZK_NTT_G1_MAX_LOG2); }
static int g1_ntt_size_checked(uint64_t n, const char* who) {
    if (g1_ntt_supported(n)) return UZK_OK;
    set_error("%s: no G1 transform of size %llu (need 2^k, k <= %d)", who, (unsigned long long)n, UZK_NTT_G1_MAX_LOG2);
    return UZK_ERR_FFT;
}
int uzk_ntt_g1_supported(uint64_t n) try { return g1_ntt_supported(n) ? 1 : 0; } catch (...) { return uzk::on_exception("uzk_ntt_g1_supported"); }

int uzk_ntt_g1_plan_info(uint64_t n, int inverse, uint64_t* doublings_out, uint64_t* additions_out) try {
    if (!doublings_out || !additions_out) { set_error("uzk_ntt_g1_plan_info: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(g1_ntt_size_checked(n, "uzk_ntt_g1_plan_info"));
    g1ntt_op_count(n, inverse != 0, doublings_out, additions_out);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ntt_g1_plan_info"); }

int uzk_ntt_g1_device(const void* d_in, void* d_out, uint64_t n, int inverse, int sync) try {
    API_LOCK;
    UZK_TRY(g1_ntt_size_checked(n, "uzk_ntt_g1_device"));
    if (!d_in || !d_out) { set_error("uzk_ntt_g1_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(g1ntt_run(c, static_cast<const Affine*>(d_in), static_cast<Affine*>(d_out), n, inverse != 0));
    if (sync) UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ntt_g1_device"); }

int uzk_ntt_g1(const uzk_g1_affine* points, uzk_g1_affine* out, uint64_t n, int inverse) try {
    API_LOCK;
    UZK_TRY(g1_ntt_size_checked(n, "uzk_ntt_g1"));
    if (!points || !out) { set_error("uzk_ntt_g1: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    const size_t bytes = (size_t)n * sizeof(Affine);
    UZK_TRY(c.g1ntt_io.reserve(bytes));
    UZK_HIP(hipMemcpyAsync(c.g1ntt_io.p, points, bytes, hipMemcpyHostToDevice, c.stream));
    UZK_TRY(g1ntt_run(c, c.g1ntt_io.as<Affine>(), c.g1ntt_io.as<Affine>(), n, inverse != 0));
    UZK_HIP(hipMemcpyAsync(out, c.g1ntt_io.p, bytes, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_ntt_g1"); }

int uzk_srs_to_lagrange(uint64_t monomial_handle, uint64_t n, uint64_t* lagrange_handle_out) try {
    API_LOCK;
    if (!lagrange_handle_out) { set_error("uzk_srs_to_lagrange: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(g1_ntt_size_checked(n, "uzk_srs_to_lagrange"));
    Ctx::Srs m;
    if (!srs_lookup(monomial_handle, &m)) { set_error("uzk_srs_to_lagrange: unknown SRS handle %llu", (unsigned long long)monomial_handle); return UZK_ERR_PARAMETER; }
    if (n > m.n) { set_error("uzk_srs_to_lagrange: n %llu exceeds SRS length %zu", (unsigned long long)n, m.n); return UZK_ERR_DEGREE; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    if (m.device != c.device) { set_error("uzk_srs_to_lagrange: the SRS lives on device %d, the calling context on device %d", m.device, c.device); return UZK_ERR_PARAMETER; }
    Ctx::Srs l;
    l.n = n;
    l.owned = true;
    l.device = c.device;
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&l.d_points), (size_t)n * sizeof(Affine)));
    int rc = g1ntt_run(c, m.d_points, l.d_points, n, true);
    if (rc == UZK_OK && hipStreamSynchronize(c.stream) != hipSuccess) { (void)hipGetLastError(); set_error("uzk_srs_to_lagrange: the transform failed on the device"); rc = UZK_ERR_DEVICE; }
    if (rc != UZK_OK) { (void)hipFree(l.d_points); return rc; }
    *lagrange_handle_out = srs_insert(l);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_to_lagrange"); }

int uzk_srs_download(uint64_t handle, size_t offset, size_t n, uzk_g1_affine* out) try {
    API_LOCK;
    if (n > 0 && !out) { set_error("uzk_srs_download: null pointer"); return UZK_ERR_PARAMETER; }
    Ctx::Srs s;
    if (!srs_lookup(handle, &s)) { set_error("uzk_srs_download: unknown SRS handle %llu", (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    if (offset > s.n || n > s.n - offset) { set_error("uzk_srs_download: offset %zu + n %zu exceeds SRS length %zu", offset, n, s.n); return UZK_ERR_DEGREE; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    if (s.device != c.device) { set_error("uzk_srs_download: the SRS lives on device %d, the calling context on device %d", s.device, c.device); return UZK_ERR_PARAMETER; }
    if (n == 0) return UZK_OK;
    UZK_HIP(hipMemcpyAsync(out, s.d_points + offset, n * sizeof(Affine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_download"); }

/* ---- SRS validation: curve check and powers-of-tau fold -------------------------------------- */
// the handle and the range P[offset .. offset + count) of a validation call; needs no device
static int srs_range_checked(const char* who, uint64_t handle, size_t offset, size_t count, Ctx::Srs* s) {
    if (!srs_lookup(handle, s)) { set_error("%s: unknown SRS handle %llu", who, (unsigned long long)handle); return UZK_ERR_PARAMETER; }
    if (offset > s->n || count > s->n - offset) { set_error("%s: offset %zu + count %zu exceeds SRS length %zu", who, offset, count, s->n); return UZK_ERR_DEGREE; }
    return UZK_OK;
}
static int srs_device_checked(const char* who, const Ctx::Srs& s, const Ctx& c) {
    if (s.device != c.device) { set_error("%s: the SRS lives on device %d, the calling context on device %d", who, s.device, c.device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

int uzk_srs_check_curve(uint64_t handle, size_t offset, size_t count, uzk_srs_curve_report* out) try {
    API_LOCK;
    if (!out) { set_error("uzk_srs_check_curve: null pointer"); return UZK_ERR_PARAMETER; }
    Ctx::Srs s;
    UZK_TRY(srs_range_checked("uzk_srs_check_curve", handle, offset, count, &s));
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(srs_device_checked("uzk_srs_check_curve", s, c));
    uzk_srs_curve_report r;
    UZK_TRY(srs_curve_run(c, s.d_points + offset, count, &r));
    if (r.first_bad != UINT64_MAX) r.first_bad += offset;
    *out = r;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_check_curve"); }

int uzk_srs_fold_weights(const uint8_t seed[32], uint64_t first, uint64_t count, uint64_t* out_mont) try {
    if (!seed || (count > 0 && !out_mont)) { set_error("uzk_srs_fold_weights: null pointer"); return UZK_ERR_PARAMETER; }
    if (count > UINT64_MAX - first) { set_error("uzk_srs_fold_weights: first + count exceeds 2^64 - 1"); return UZK_ERR_PARAMETER; }
    srs_weights_host(seed, first, count, reinterpret_cast<Fp*>(out_mont));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_fold_weights"); }

// left = sum_{i < count - 1} rho_i P[i], right = sum rho_i P[i + 1] over the device array P[0 .. count): the weights expanded into
// the context's workspace, two MSMs over the one scalar vector (plain bases: the array is not a handle's, a window table would not
// cover the shifted run)
static int srs_fold_run(Ctx& c, const Affine* d_points, size_t count, const uint8_t seed[32], Jac* left, Jac* right) {
    const size_t m = count - 1;
    UZK_TRY(c.srs_weights.reserve(m * sizeof(Fp)));
    Fp* d_w = c.srs_weights.as<Fp>();
    UZK_TRY(srs_weights_run(c, seed, 0, m, d_w));
    if (c.prof_on) UZK_HIP(hipStreamSynchronize(c.stream));        // so that the two host sections below time the MSMs alone
    Ctx::Srs run;
    run.d_points = const_cast<Affine*>(d_points);
    run.n = count;
    run.device = c.device;
    {
        HostScope hs(c, "host_srs_fold_msm_left");
        UZK_TRY(msm_dispatch(run, 0, d_w, m, 1, left));
    }
    {
        HostScope hs(c, "host_srs_fold_msm_right");
        UZK_TRY(msm_dispatch(run, 1, d_w, m, 1, right));
    }
    return UZK_OK;
}

int uzk_srs_fold_powers(uint64_t handle, size_t offset, size_t count, const uint8_t seed[32], uzk_g1_jac* left_out, uzk_g1_jac* right_out) try {
    API_LOCK;
    if (!seed || !left_out || !right_out) { set_error("uzk_srs_fold_powers: null pointer"); return UZK_ERR_PARAMETER; }
    if (count < 2) { set_error("uzk_srs_fold_powers: a run of %zu points holds no equation (count >= 2)", count); return UZK_ERR_PARAMETER; }
    Ctx::Srs s;
    UZK_TRY(srs_range_checked("uzk_srs_fold_powers", handle, offset, count, &s));
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(srs_device_checked("uzk_srs_fold_powers", s, c));
    Jac l, r;
    UZK_TRY(srs_fold_run(c, s.d_points + offset, count, seed, &l, &r));
    std::memcpy(left_out, &l, sizeof l);
    std::memcpy(right_out, &r, sizeof r);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_fold_powers"); }

int uzk_srs_fold_powers_lagrange(uint64_t lagrange_handle, uint64_t n, const uint8_t seed[32], uzk_g1_affine* first_out, uzk_g1_jac* left_out,
                                 uzk_g1_jac* right_out) try {
    API_LOCK;
    if (!seed || !first_out || !left_out || !right_out) { set_error("uzk_srs_fold_powers_lagrange: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(g1_ntt_size_checked(n, "uzk_srs_fold_powers_lagrange"));
    if (n < 2) { set_error("uzk_srs_fold_powers_lagrange: a run of %llu points holds no equation (n >= 2)", (unsigned long long)n); return UZK_ERR_PARAMETER; }
    Ctx::Srs s;
    UZK_TRY(srs_range_checked("uzk_srs_fold_powers_lagrange", lagrange_handle, 0, (size_t)n, &s));
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(srs_device_checked("uzk_srs_fold_powers_lagrange", s, c));
    UZK_TRY(c.srs_points.reserve((size_t)n * sizeof(Affine)));
    Affine* d_m = c.srs_points.as<Affine>();
    UZK_TRY(g1ntt_run(c, s.d_points, d_m, n, false));
    Jac l, r;
    UZK_TRY(srs_fold_run(c, d_m, (size_t)n, seed, &l, &r));
    UZK_HIP(hipMemcpyAsync(first_out, d_m, sizeof(Affine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    std::memcpy(left_out, &l, sizeof l);
    std::memcpy(right_out, &r, sizeof r);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_fold_powers_lagrange"); }

int uzk_test_srs_weights_device(const uint8_t seed[32], uint64_t count, uint64_t* out_mont) try {
    API_LOCK;
    if (!seed || (count > 0 && !out_mont)) { set_error("uzk_test_srs_weights_device: null pointer"); return UZK_ERR_PARAMETER; }
    if (count == 0) return UZK_OK;
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(c.srs_weights.reserve((size_t)count * sizeof(Fp)));
    UZK_TRY(srs_weights_run(c, seed, 0, count, c.srs_weights.as<Fp>()));
    UZK_HIP(hipMemcpyAsync(out_mont, c.srs_weights.p, (size_t)count * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_test_srs_weights_device"); }

/* ---- batch verification -------------------------------------------------------------------- */
int uzk_vk_create(const uzk_vk_desc* desc, uint64_t* vk_out) try {
    API_LOCK;
    if (!desc || !vk_out) { set_error("uzk_vk_create: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(vf_key_check(desc));
    UZK_TRY(require_ready());
    return vf_key_create(ctx(), desc, vk_out);
} catch (...) { return uzk::on_exception("uzk_vk_create"); }

int uzk_vk_release(uint64_t vk) try {
    API_LOCK;
    return vf_key_release(vk);
} catch (...) { return uzk::on_exception("uzk_vk_release"); }

int uzk_vk_info(uint64_t vk, uint32_t* cs_size_out, uint32_t* n_pi_out, uint32_t* proof_bytes_out, int* device_out) try {
    if (!vf_key_known(vk, cs_size_out, n_pi_out, proof_bytes_out, device_out)) { set_error("uzk_vk_info: unknown verifier key %llu", (unsigned long long)vk); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_vk_info"); }

int uzk_vk_set_public_key(uint64_t vk, const uzk_g1_affine pk[12]) try {
    API_LOCK;
    if (!pk) { set_error("uzk_vk_set_public_key: null pointer"); return UZK_ERR_PARAMETER; }
    if (!vf_key_known(vk, nullptr, nullptr, nullptr, nullptr)) { set_error("uzk_vk_set_public_key: unknown verifier key %llu", (unsigned long long)vk); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return vf_key_set_public_key(ctx(), vk, reinterpret_cast<const Affine*>(pk));
} catch (...) { return uzk::on_exception("uzk_vk_set_public_key"); }

int uzk_verify_fold(uint64_t vk, const uint8_t* proofs, const uint64_t* pi_mont, uint32_t m, const uint64_t* weights_mont, uzk_g1_jac* left_out,
                    uzk_g1_jac* right_out, uint8_t* status_out, uint64_t* challenges_out) try {
    API_LOCK;
    if (m > UZK_VERIFY_MAX_BATCH) { set_error("uzk_verify_fold: %u proofs (at most %d per call)", m, UZK_VERIFY_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (m > 1 && !weights_mont) { set_error("uzk_verify_fold: %u proofs need a weight each (unweighted sums let errors cancel)", m); return UZK_ERR_PARAMETER; }
    if (!left_out || !right_out || (m > 0 && (!proofs || !status_out))) { set_error("uzk_verify_fold: null pointer"); return UZK_ERR_PARAMETER; }
    uint32_t n_pi = 0;
    if (!vf_key_known(vk, nullptr, &n_pi, nullptr, nullptr)) { set_error("uzk_verify_fold: unknown verifier key %llu", (unsigned long long)vk); return UZK_ERR_PARAMETER; }
    if (m > 0 && n_pi > 0 && !pi_mont) { set_error("uzk_verify_fold: null public inputs"); return UZK_ERR_PARAMETER; }
    Jac l = jac_inf(), r = jac_inf();
    if (m > 0) {
        UZK_TRY(require_ready());
        UZK_TRY(vf_fold_run(ctx(), vk, proofs, as_fp(pi_mont), m, weights_mont ? as_fp(weights_mont) : nullptr, &l, &r, status_out,
                            reinterpret_cast<Fp*>(challenges_out)));
    }
    std::memcpy(left_out, &l, sizeof l);
    std::memcpy(right_out, &r, sizeof r);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_verify_fold"); }

/* ---- batch Groth16 verification ------------------------------------------------------------ */
int uzk_g16_vk_create(const uzk_g16_vk_desc* desc, uint64_t* vk_out) try {
    API_LOCK;
    if (!desc || !vk_out) { set_error("uzk_g16_vk_create: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(g16v_key_check(desc));
    UZK_TRY(require_ready());
    return g16v_key_create(ctx(), desc, vk_out);
} catch (...) { return uzk::on_exception("uzk_g16_vk_create"); }

int uzk_g16_vk_release(uint64_t vk) try {
    API_LOCK;
    return g16v_key_release(vk);
} catch (...) { return uzk::on_exception("uzk_g16_vk_release"); }

int uzk_g16_vk_info(uint64_t vk, uint32_t* n_inputs_out, int* device_out) try {
    if (!g16v_key_known(vk, n_inputs_out, device_out)) { set_error("uzk_g16_vk_info: unknown verifying key %llu", (unsigned long long)vk); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g16_vk_info"); }

int uzk_g16_verify_fold(uint64_t vk, const uint8_t* proofs, const uint64_t* public_mont, uint32_t m, const uint64_t* weights_mont, uzk_g1_affine* a_out,
                        uzk_g2_affine* b_out, uzk_g1_jac* alpha_out, uzk_g1_jac* x_out, uzk_g1_jac* c_out, uint8_t* status_out) try {
    API_LOCK;
    if (m > UZK_G16_VERIFY_MAX_BATCH) { set_error("uzk_g16_verify_fold: %u proofs (at most %d per call)", m, UZK_G16_VERIFY_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (m > 1 && !weights_mont) { set_error("uzk_g16_verify_fold: %u proofs need a weight each (unweighted sums let errors cancel)", m); return UZK_ERR_PARAMETER; }
    if (!alpha_out || !x_out || !c_out || (m > 0 && (!proofs || !a_out || !b_out || !status_out))) { set_error("uzk_g16_verify_fold: null pointer"); return UZK_ERR_PARAMETER; }
    uint32_t n_inputs = 0;
    if (!g16v_key_known(vk, &n_inputs, nullptr)) { set_error("uzk_g16_verify_fold: unknown verifying key %llu", (unsigned long long)vk); return UZK_ERR_PARAMETER; }
    if (m > 0 && n_inputs > 1 && !public_mont) { set_error("uzk_g16_verify_fold: null public inputs"); return UZK_ERR_PARAMETER; }
    Jac al = jac_inf(), x = jac_inf(), cc = jac_inf();
    if (m > 0) {
        UZK_TRY(require_ready());
        UZK_TRY(g16v_fold_run(ctx(), vk, proofs, as_fp(public_mont), m, weights_mont ? as_fp(weights_mont) : nullptr, reinterpret_cast<Affine*>(a_out),
                              reinterpret_cast<G2Affine*>(b_out), &al, &x, &cc, status_out));
    }
    std::memcpy(alpha_out, &al, sizeof al);
    std::memcpy(x_out, &x, sizeof x);
    std::memcpy(c_out, &cc, sizeof cc);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g16_verify_fold"); }

/* ---- the pairing product -------------------------------------------------------------------- */
static const char* pairing_status_text(uint8_t st) { return st == 1 ? "a coordinate word is not below p" : "a point is not on its curve"; }

int uzk_pairing_product(const uzk_g1_affine* p, const uzk_g2_affine* q, uint32_t n, uzk_gt* gt_out, int* is_one_out) try {
    API_LOCK;
    if (n > UZK_PAIRING_MAX_PAIRS) { set_error("uzk_pairing_product: %u pairs (at most %d per call)", n, UZK_PAIRING_MAX_PAIRS); return UZK_ERR_PARAMETER; }
    if (!is_one_out || (n > 0 && (!p || !q))) { set_error("uzk_pairing_product: null pointer"); return UZK_ERR_PARAMETER; }
    Fq12w gt;
    uint32_t bad = n;
    uint8_t bad_status = 0;
    if (n > 0) UZK_TRY(require_ready());
    UZK_TRY(pairing_product_run(ctx(), reinterpret_cast<const Affine*>(p), reinterpret_cast<const G2Affine*>(q), false, n, &gt, &bad, &bad_status));
    if (bad < n) { set_error("uzk_pairing_product: pair %u: %s", bad, pairing_status_text(bad_status)); return UZK_ERR_PARAMETER; }
    static_assert(sizeof(uzk_gt) == sizeof(Fq12w), "uzk_gt is the wire form of Fq12");
    if (gt_out) std::memcpy(gt_out, &gt, sizeof gt);
    *is_one_out = gt_is_one(gt) ? 1 : 0;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_pairing_product"); }

int uzk_g16_verify_batch(uint64_t vk, const uint8_t* proofs, const uint64_t* public_mont, uint32_t m, const uint64_t* weights_mont, const uzk_g2_affine g2[3],
                         uint8_t* status_out, int* accepted_out) try {
    API_LOCK;
    if (m > UZK_G16_VERIFY_MAX_BATCH) { set_error("uzk_g16_verify_batch: %u proofs (at most %d per call)", m, UZK_G16_VERIFY_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (m > 1 && !weights_mont) { set_error("uzk_g16_verify_batch: %u proofs need a weight each (unweighted sums let errors cancel)", m); return UZK_ERR_PARAMETER; }
    if (!accepted_out || !g2 || (m > 0 && (!proofs || !status_out))) { set_error("uzk_g16_verify_batch: null pointer"); return UZK_ERR_PARAMETER; }
    uint32_t n_inputs = 0;
    if (!g16v_key_known(vk, &n_inputs, nullptr)) { set_error("uzk_g16_verify_batch: unknown verifying key %llu", (unsigned long long)vk); return UZK_ERR_PARAMETER; }
    if (m > 0 && n_inputs > 1 && !public_mont) { set_error("uzk_g16_verify_batch: null public inputs"); return UZK_ERR_PARAMETER; }
    if (m == 0) { *accepted_out = 1; return UZK_OK; }              // the empty product
    UZK_TRY(require_ready());
    Fq12w gt;
    uint32_t bad_g2 = 3;
    UZK_TRY(g16v_verify_run(ctx(), vk, proofs, as_fp(public_mont), m, weights_mont ? as_fp(weights_mont) : nullptr, reinterpret_cast<const G2Affine*>(g2), status_out,
                            &gt, &bad_g2));
    if (bad_g2 < 3) { set_error("uzk_g16_verify_batch: g2[%u] is not a canonical point of the twist", bad_g2); return UZK_ERR_PARAMETER; }
    bool ok = gt_is_one(gt);
    for (uint32_t i = 0; i < m; ++i) ok = ok && status_out[i] == 0;
    *accepted_out = ok ? 1 : 0;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_g16_verify_batch"); }

/* ---- Baby Jubjub and the Chaum-Pedersen reveal proofs ------------------------------------------- */
static const EdAffine* as_ed(const uint64_t* p) { return reinterpret_cast<const EdAffine*>(p); }
static EdAffine* as_ed(uint64_t* p) { return reinterpret_cast<EdAffine*>(p); }
// the callers' points enter the lazy limbs as canonical words: anything else is refused before the device is touched
static int ed_require_canonical(const char* who, const char* what, const uint64_t* words, size_t points) {
    const size_t bad = ed_first_noncanonical(as_fp(words), 2 * points);
    if (bad < 2 * points) { set_error("%s: %s[%zu]: the %c coordinate is not below q", who, what, bad / 2, bad % 2 ? 'y' : 'x'); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

int uzk_ed_check_points(const uint64_t* points_mont, size_t n, uint8_t* status_out) try {
    API_LOCK;
    if (n == 0 || n > UZK_ED_MAX_BATCH) { set_error("uzk_ed_check_points: %zu points (1 .. %d per call)", n, UZK_ED_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!points_mont || !status_out) { set_error("uzk_ed_check_points: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return ed_check_run(ctx(), as_ed(points_mont), n, status_out);
} catch (...) { return uzk::on_exception("uzk_ed_check_points"); }

int uzk_ed_mul_batch(const uint64_t* points_mont, size_t point_stride, const uint64_t* scalars, size_t n, uint64_t* out_mont) try {
    API_LOCK;
    if (n == 0 || n > UZK_ED_MAX_BATCH) { set_error("uzk_ed_mul_batch: %zu items (1 .. %d per call)", n, UZK_ED_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (point_stride > 1) { set_error("uzk_ed_mul_batch: point stride %zu (0: one shared base, 1: a base per item)", point_stride); return UZK_ERR_PARAMETER; }
    if (!points_mont || !scalars || !out_mont) { set_error("uzk_ed_mul_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical("uzk_ed_mul_batch", "points", points_mont, point_stride ? n : 1));
    UZK_TRY(require_ready());
    return ed_mul_run(ctx(), as_ed(points_mont), point_stride == 0, as_fp(scalars), n, as_ed(out_mont));
} catch (...) { return uzk::on_exception("uzk_ed_mul_batch"); }

int uzk_ed_sum_batch(const uint64_t* rows_mont, uint32_t k, uint32_t n, uint64_t* out_mont) try {
    API_LOCK;
    if (k == 0 || k > UZK_ED_MAX_ROWS || n == 0 || n > UZK_ED_MAX_BATCH) {
        set_error("uzk_ed_sum_batch: %u rows of %u points (1 .. %d rows of 1 .. %d)", k, n, UZK_ED_MAX_ROWS, UZK_ED_MAX_BATCH);
        return UZK_ERR_PARAMETER;
    }
    if (!rows_mont || !out_mont) { set_error("uzk_ed_sum_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical("uzk_ed_sum_batch", "rows", rows_mont, (size_t)k * n));
    UZK_TRY(require_ready());
    return ed_sum_run(ctx(), nullptr, as_ed(rows_mont), k, n, as_ed(out_mont));
} catch (...) { return uzk::on_exception("uzk_ed_sum_batch"); }

int uzk_ed_unmask_batch(const uint64_t* e2_mont, const uint64_t* reveals_mont, uint32_t k, uint32_t n, uint64_t* out_mont) try {
    API_LOCK;
    if (k == 0 || k > UZK_ED_MAX_ROWS || n == 0 || n > UZK_ED_MAX_BATCH) {
        set_error("uzk_ed_unmask_batch: %u rows of %u points (1 .. %d rows of 1 .. %d)", k, n, UZK_ED_MAX_ROWS, UZK_ED_MAX_BATCH);
        return UZK_ERR_PARAMETER;
    }
    if (!e2_mont || !reveals_mont || !out_mont) { set_error("uzk_ed_unmask_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical("uzk_ed_unmask_batch", "e2", e2_mont, n));
    UZK_TRY(ed_require_canonical("uzk_ed_unmask_batch", "reveals", reveals_mont, (size_t)k * n));
    UZK_TRY(require_ready());
    return ed_sum_run(ctx(), as_ed(e2_mont), as_ed(reveals_mont), k, n, as_ed(out_mont));
} catch (...) { return uzk::on_exception("uzk_ed_unmask_batch"); }

// the Keccak transcript (anemoi == false) and the zk-friendly one share everything but the challenge
static int cp_reveal_prove(const char* who, bool anemoi, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* omegas, uint32_t m, uint64_t* reveal_out,
                           uint64_t* pk_out, uint8_t* proofs_out) {
    if (m == 0 || m > UZK_CP_MAX_BATCH) { set_error("%s: %u cards (1 .. %d per call)", who, m, UZK_CP_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!sk || !e1_mont || !omegas || !reveal_out || !pk_out || !proofs_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical(who, "e1", e1_mont, m));
    UZK_TRY(require_ready());
    return cp_prove_run(ctx(), as_fp(sk), as_ed(e1_mont), as_fp(omegas), m, as_ed(reveal_out), as_ed(pk_out), proofs_out, anemoi);
}
static int cp_reveal_verify(const char* who, bool anemoi, const uint64_t* statements_mont, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out,
                            uint64_t* challenges_out) {
    if (m == 0 || m > UZK_CP_MAX_BATCH) { set_error("%s: %u proofs (1 .. %d per call)", who, m, UZK_CP_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!statements_mont || !proofs || !verdict_out) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return cp_verify_run(ctx(), as_ed(statements_mont), proofs, m, verdict_out, reinterpret_cast<Fp*>(challenges_out), anemoi);
}

int uzk_cp_reveal_prove_batch(const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* omegas, uint32_t m, uint64_t* reveal_out, uint64_t* pk_out,
                              uint8_t* proofs_out) try {
    API_LOCK;
    return cp_reveal_prove("uzk_cp_reveal_prove_batch", false, sk, e1_mont, omegas, m, reveal_out, pk_out, proofs_out);
} catch (...) { return uzk::on_exception("uzk_cp_reveal_prove_batch"); }

int uzk_cp_reveal_verify_batch(const uint64_t* statements_mont, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, uint64_t* challenges_out) try {
    API_LOCK;
    return cp_reveal_verify("uzk_cp_reveal_verify_batch", false, statements_mont, proofs, m, verdict_out, challenges_out);
} catch (...) { return uzk::on_exception("uzk_cp_reveal_verify_batch"); }

int uzk_cp_reveal_prove0_batch(const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* omegas, uint32_t m, uint64_t* reveal_out, uint64_t* pk_out,
                               uint8_t* proofs_out) try {
    API_LOCK;
    return cp_reveal_prove("uzk_cp_reveal_prove0_batch", true, sk, e1_mont, omegas, m, reveal_out, pk_out, proofs_out);
} catch (...) { return uzk::on_exception("uzk_cp_reveal_prove0_batch"); }

int uzk_cp_reveal_verify0_batch(const uint64_t* statements_mont, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, uint64_t* challenges_out) try {
    API_LOCK;
    return cp_reveal_verify("uzk_cp_reveal_verify0_batch", true, statements_mont, proofs, m, verdict_out, challenges_out);
} catch (...) { return uzk::on_exception("uzk_cp_reveal_verify0_batch"); }

/* ---- Anemoi-Jive: hashes, the stream cipher, their traces ---------------------------------------- */
// every element enters the lazy limbs as canonical words: anything else is refused before the device is touched
static int anemoi_require_canonical(const char* who, const uint64_t* words, size_t elems, size_t per_item) {
    const size_t bad = ed_first_noncanonical(as_fp(words), elems);
    if (bad < elems) { set_error("%s: element %zu of item %zu is not below r", who, bad % per_item, bad / per_item); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}
static int anemoi_sponge(const char* who, const uint64_t* inputs_mont, uint32_t len, size_t n, uint32_t out_len, uint64_t* out_mont, uint64_t* trace_out) {
    if (n == 0 || n > UZK_ANEMOI_MAX_BATCH) { set_error("%s: %zu items (1 .. %d per call)", who, n, UZK_ANEMOI_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (len > UZK_ANEMOI_MAX_INPUT) { set_error("%s: %u input elements (at most %d)", who, len, UZK_ANEMOI_MAX_INPUT); return UZK_ERR_PARAMETER; }
    if ((len > 0 && !inputs_mont) || !out_mont) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    if (len > 0) UZK_TRY(anemoi_require_canonical(who, inputs_mont, n * len, len));
    UZK_TRY(require_ready());
    return anemoi_sponge_run(ctx(), as_fp(inputs_mont), len, n, out_len, reinterpret_cast<Fp*>(out_mont), reinterpret_cast<Fp*>(trace_out));
}

int uzk_anemoi_permute_batch(const uint64_t* states_mont, size_t n, uint64_t* out_mont) try {
    API_LOCK;
    if (n == 0 || n > UZK_ANEMOI_MAX_BATCH) { set_error("uzk_anemoi_permute_batch: %zu states (1 .. %d per call)", n, UZK_ANEMOI_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!states_mont || !out_mont) { set_error("uzk_anemoi_permute_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(anemoi_require_canonical("uzk_anemoi_permute_batch", states_mont, 4 * n, 4));
    UZK_TRY(require_ready());
    return anemoi_permute_run(ctx(), as_fp(states_mont), n, reinterpret_cast<Fp*>(out_mont));
} catch (...) { return uzk::on_exception("uzk_anemoi_permute_batch"); }

int uzk_anemoi_hash_batch(const uint64_t* inputs_mont, uint32_t len, size_t n, uint64_t* out_mont, uint64_t* trace_out) try {
    API_LOCK;
    return anemoi_sponge("uzk_anemoi_hash_batch", inputs_mont, len, n, 0, out_mont, trace_out);
} catch (...) { return uzk::on_exception("uzk_anemoi_hash_batch"); }

int uzk_anemoi_stream_batch(const uint64_t* inputs_mont, uint32_t len, size_t n, uint32_t out_len, uint64_t* out_mont, uint64_t* trace_out) try {
    API_LOCK;
    if (out_len == 0 || out_len > UZK_ANEMOI_MAX_OUTPUT) {
        set_error("uzk_anemoi_stream_batch: %u outputs (1 .. %d)", out_len, UZK_ANEMOI_MAX_OUTPUT);
        return UZK_ERR_PARAMETER;
    }
    return anemoi_sponge("uzk_anemoi_stream_batch", inputs_mont, len, n, out_len, out_mont, trace_out);
} catch (...) { return uzk::on_exception("uzk_anemoi_stream_batch"); }

uint32_t uzk_anemoi_permutations(uint32_t len, uint32_t out_len) { return uzk::anemoi_permutations(len, out_len); }

int uzk_remark_key_create(const uint64_t* pk_mont, uint64_t* key_out) try {
    API_LOCK;
    if (!pk_mont || !key_out) { set_error("uzk_remark_key_create: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical("uzk_remark_key_create", "pk", pk_mont, 1));
    UZK_TRY(require_ready());
    return remark_key_create(ctx(), as_ed(pk_mont), key_out);
} catch (...) { return uzk::on_exception("uzk_remark_key_create"); }

int uzk_remark_key_release(uint64_t key) try {
    API_LOCK;
    return remark_key_release(key);
} catch (...) { return uzk::on_exception("uzk_remark_key_release"); }

int uzk_remark_key_tables(uint64_t key, uint64_t* pk_tables_out, uint64_t* gen_tables_out) try {
    API_LOCK;
    if (!remark_key_known(key, nullptr)) { set_error("uzk_remark_key_tables: unknown remask key %llu", (unsigned long long)key); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return remark_tables_run(ctx(), key, reinterpret_cast<Fp*>(pk_tables_out), reinterpret_cast<Fp*>(gen_tables_out));
} catch (...) { return uzk::on_exception("uzk_remark_key_tables"); }

int uzk_remark_batch(uint64_t key, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* digits, const uint32_t* perm, uint32_t n, uint64_t* e1_out,
                     uint64_t* e2_out, uint64_t* trace_out) try {
    API_LOCK;
    if (n == 0 || n > UZK_ED_MAX_BATCH) { set_error("uzk_remark_batch: %u cards (1 .. %d per call)", n, UZK_ED_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!e1_mont || !e2_mont || !digits || !e1_out || !e2_out) { set_error("uzk_remark_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical("uzk_remark_batch", "e1", e1_mont, n));
    UZK_TRY(ed_require_canonical("uzk_remark_batch", "e2", e2_mont, n));
    for (size_t i = 0; i < (size_t)n * UZK_REMARK_ITERATIONS; ++i)
        if (digits[i] > 7) {
            set_error("uzk_remark_batch: digit %zu of card %zu is %u (three bits: 0 .. 7)", i % UZK_REMARK_ITERATIONS, i / UZK_REMARK_ITERATIONS, digits[i]);
            return UZK_ERR_PARAMETER;
        }
    std::vector<uint32_t> slot;                                     // slot[perm[i]] = i: where card perm[i] goes
    if (perm) {
        slot.assign(n, 0xffffffffu);
        for (uint32_t i = 0; i < n; ++i) {
            if (perm[i] >= n || slot[perm[i]] != 0xffffffffu) { set_error("uzk_remark_batch: perm[%u] = %u: not a permutation of 0 .. %u", i, perm[i], n - 1); return UZK_ERR_PARAMETER; }
            slot[perm[i]] = i;
        }
    }
    if (!remark_key_known(key, nullptr)) { set_error("uzk_remark_batch: unknown remask key %llu", (unsigned long long)key); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return remark_run(ctx(), key, as_ed(e1_mont), as_ed(e2_mont), digits, perm ? slot.data() : nullptr, n, as_ed(e1_out), as_ed(e2_out), reinterpret_cast<Fp*>(trace_out));
} catch (...) { return uzk::on_exception("uzk_remark_batch"); }

/* ---- the shuffle circuit (shufflecs.cpp takes the context lock itself) ---------------------------- */
int uzk_shuffle_cs_info(uint32_t cards, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out) try {
    return shcs_info(cards, size_out, n_out, num_vars_out, pi_count_out, pi_rows_out);
} catch (...) { return uzk::on_exception("uzk_shuffle_cs_info"); }

int uzk_shuffle_circuit_create(const uzk_shuffle_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out) try {
    return shcs_circuit_create(desc, circuit_out, commitments_out);
} catch (...) { return uzk::on_exception("uzk_shuffle_circuit_create"); }

int uzk_shuffle_circuit_set_key(uint64_t circuit, uint64_t remark_key, uzk_g1_jac* commitments_out) try {
    return shcs_circuit_set_key(circuit, remark_key, commitments_out);
} catch (...) { return uzk::on_exception("uzk_shuffle_circuit_set_key"); }

int uzk_shuffle_witness_batch(uint64_t circuit, uint64_t remark_key, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* digits,
                              const uint32_t* perms, uint32_t cards, uint32_t batch, void* d_witness, void* d_wsel, uint64_t* pi_values_out,
                              uint64_t* e1_out, uint64_t* e2_out) try {
    return shcs_witness_batch(circuit, remark_key, e1_mont, e2_mont, digits, perms, cards, batch, d_witness, d_wsel, pi_values_out, e1_out, e2_out);
} catch (...) { return uzk::on_exception("uzk_shuffle_witness_batch"); }

int uzk_test_shuffle_cs_tables(uint64_t circuit, uint64_t remark_key, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out) try {
    return shcs_test_tables(circuit, remark_key, wiring_out, perm_out, evals_out);
} catch (...) { return uzk::on_exception("uzk_test_shuffle_cs_tables"); }

/* ---- the matchmaking circuit (matchcs.cpp takes the context lock itself) -------------------------- */
int uzk_match_cs_info(uint32_t players, uint32_t* size_out, uint32_t* n_out, uint32_t* num_vars_out, uint32_t* pi_count_out, uint32_t* pi_rows_out) try {
    return mcs_info(players, size_out, n_out, num_vars_out, pi_count_out, pi_rows_out);
} catch (...) { return uzk::on_exception("uzk_match_cs_info"); }

int uzk_match_circuit_create(const uzk_match_circuit_desc* desc, uint64_t* circuit_out, uzk_g1_jac* commitments_out) try {
    return mcs_circuit_create(desc, circuit_out, commitments_out);
} catch (...) { return uzk::on_exception("uzk_match_circuit_create"); }

int uzk_match_witness_batch(uint64_t circuit, const uint64_t* inputs_mont, const uint64_t* seeds_mont, const uint64_t* randoms_mont, uint32_t players,
                            uint32_t batch, void* d_witness, uint64_t* pi_values_out, uint64_t* outputs_out, uint64_t* commitments_out) try {
    return mcs_witness_batch(circuit, inputs_mont, seeds_mont, randoms_mont, players, batch, d_witness, pi_values_out, outputs_out, commitments_out);
} catch (...) { return uzk::on_exception("uzk_match_witness_batch"); }

int uzk_test_match_cs_tables(uint64_t circuit, uint32_t* wiring_out, uint32_t* perm_out, uint64_t* evals_out) try {
    return mcs_test_tables(circuit, wiring_out, perm_out, evals_out);
} catch (...) { return uzk::on_exception("uzk_test_match_cs_tables"); }

int uzk_test_match_divrem(const uint64_t* values, uint32_t m, uint32_t count, uint64_t* quot_out, uint32_t* rem_out) try {
    return mcs_test_divrem(values, m, count, quot_out, rem_out);
} catch (...) { return uzk::on_exception("uzk_test_match_divrem"); }

/* ---- the reveal circuit (revealcs.hip takes the context lock itself) ------------------------------- */
int uzk_reveal_cs_info(uint32_t* n_vars_out, uint32_t* n_inputs_out, uint32_t* n_constraints_out, uint64_t* domain_out, uint64_t nnz_out[3]) try {
    return rcs_info(n_vars_out, n_inputs_out, n_constraints_out, domain_out, nnz_out);
} catch (...) { return uzk::on_exception("uzk_reveal_cs_info"); }

int uzk_reveal_cs_matrices(uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]) try {
    return rcs_matrices(row_ptr, col, val);
} catch (...) { return uzk::on_exception("uzk_reveal_cs_matrices"); }

int uzk_reveal_circuit_create(const uzk_g16_key_desc* desc, uint64_t* circuit_out) try {
    return rcs_circuit_create(desc, circuit_out);
} catch (...) { return uzk::on_exception("uzk_reveal_circuit_create"); }

int uzk_reveal_circuit_release(uint64_t circuit) try {
    return rcs_circuit_release(circuit);
} catch (...) { return uzk::on_exception("uzk_reveal_circuit_release"); }

int uzk_reveal_circuit_key(uint64_t circuit, uint64_t* key_out) try {
    return rcs_circuit_key(circuit, key_out);
} catch (...) { return uzk::on_exception("uzk_reveal_circuit_key"); }

int uzk_reveal_witness_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, uint32_t m, void* d_z, uint64_t* statements_out) try {
    return rcs_witness_batch(circuit, sk, e1_mont, m, d_z, statements_out);
} catch (...) { return uzk::on_exception("uzk_reveal_witness_batch"); }

int uzk_reveal_prove_snark_batch(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                                 uint64_t* statements_out, uzk_g16_proof* proofs_out) try {
    return rcs_prove_snark_batch(circuit, sk, e1_mont, r_mont, s_mont, m, statements_out, proofs_out);
} catch (...) { return uzk::on_exception("uzk_reveal_prove_snark_batch"); }

int uzk_reveal_prove_snark_batch_finish(uint64_t circuit, const uint64_t* sk, const uint64_t* e1_mont, const uint64_t* r_mont, const uint64_t* s_mont, uint32_t m,
                                        uint64_t* statements_out, uzk_g16_proof* proofs_out, uint8_t* blobs_out, void* d_blobs_out) try {
    return rcs_prove_snark_batch_finish(circuit, sk, e1_mont, r_mont, s_mont, m, statements_out, proofs_out, blobs_out, d_blobs_out);
} catch (...) { return uzk::on_exception("uzk_reveal_prove_snark_batch_finish"); }

/* ---- the point codec ------------------------------------------------------------------------------ */
static int codec_batch_args(const char* who, const void* in, size_t n, const void* out, const void* status) {
    if (n == 0 || n > UZK_CODEC_MAX_BATCH) { set_error("%s: %zu points (1 .. %d per call)", who, n, UZK_CODEC_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!in || !out || !status) { set_error("%s: null pointer", who); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}
static int codec_decompress_entry(const char* who, int group, const uint8_t* in, size_t n, int check_subgroup, void* out, uint8_t* status_out) {
    API_LOCK;
    UZK_TRY(codec_batch_args(who, in, n, out, status_out));
    UZK_TRY(require_ready());
    return codec_decompress_run(ctx(), group, in, n, check_subgroup != 0, out, nullptr, status_out);
}
static int codec_compress_entry(const char* who, int group, const void* points, size_t n, uint8_t* out, uint8_t* status_out) {
    API_LOCK;
    UZK_TRY(codec_batch_args(who, points, n, out, status_out));
    UZK_TRY(require_ready());
    return codec_compress_run(ctx(), group, points, n, out, status_out);
}

int uzk_g1_decompress_batch(const uint8_t* enc, size_t n, uzk_g1_affine* out, uint8_t* status_out) try {
    return codec_decompress_entry("uzk_g1_decompress_batch", 0, enc, n, 0, out, status_out);
} catch (...) { return uzk::on_exception("uzk_g1_decompress_batch"); }

int uzk_g2_decompress_batch(const uint8_t* enc, size_t n, int check_subgroup, uzk_g2_affine* out, uint8_t* status_out) try {
    return codec_decompress_entry("uzk_g2_decompress_batch", 1, enc, n, check_subgroup, out, status_out);
} catch (...) { return uzk::on_exception("uzk_g2_decompress_batch"); }

int uzk_ed_decompress_batch(const uint8_t* enc, size_t n, int check_subgroup, uint64_t* points_mont_out, uint8_t* status_out) try {
    return codec_decompress_entry("uzk_ed_decompress_batch", 2, enc, n, check_subgroup, points_mont_out, status_out);
} catch (...) { return uzk::on_exception("uzk_ed_decompress_batch"); }

int uzk_g1_compress_batch(const uzk_g1_affine* points, size_t n, uint8_t* out, uint8_t* status_out) try {
    return codec_compress_entry("uzk_g1_compress_batch", 0, points, n, out, status_out);
} catch (...) { return uzk::on_exception("uzk_g1_compress_batch"); }

int uzk_g2_compress_batch(const uzk_g2_affine* points, size_t n, uint8_t* out, uint8_t* status_out) try {
    return codec_compress_entry("uzk_g2_compress_batch", 1, points, n, out, status_out);
} catch (...) { return uzk::on_exception("uzk_g2_compress_batch"); }

int uzk_ed_compress_batch(const uint64_t* points_mont, size_t n, uint8_t* out, uint8_t* status_out) try {
    return codec_compress_entry("uzk_ed_compress_batch", 2, points_mont, n, out, status_out);
} catch (...) { return uzk::on_exception("uzk_ed_compress_batch"); }

// n encodings of `group` decoded into a fresh device array, UZK_CODEC_MAX_BATCH at a time; a non-zero status frees it and is the error
static int codec_register_decode(const char* who, int group, const uint8_t* in, size_t n, bool check_subgroup, void** d_out) {
    Ctx& c = ctx();
    const size_t enc = group == 1 ? 64 : 32, pt = group == 1 ? sizeof(G2Affine) : sizeof(Affine);
    char* d = nullptr;
    UZK_HIP(hipMalloc(reinterpret_cast<void**>(&d), n * pt));
    std::vector<uint8_t> st;
    int rc = UZK_OK;
    for (size_t at = 0; at < n && rc == UZK_OK; at += UZK_CODEC_MAX_BATCH) {
        const size_t m = std::min<size_t>(UZK_CODEC_MAX_BATCH, n - at);
        st.assign(m, 0);
        rc = codec_decompress_run(c, group, in + at * enc, m, check_subgroup, nullptr, d + at * pt, st.data());
        for (size_t i = 0; i < m && rc == UZK_OK; ++i)
            if (st[i]) { set_error("%s: point %zu: status %u", who, at + i, (unsigned)st[i]); rc = UZK_ERR_PARAMETER; }
    }
    if (rc != UZK_OK) { (void)hipFree(d); return rc; }
    *d_out = d;
    return UZK_OK;
}

int uzk_srs_register_compressed(const uint8_t* enc, size_t n, uint64_t* handle_out) try {
    API_LOCK;
    if (!enc || !handle_out) { set_error("uzk_srs_register_compressed: null pointer"); return UZK_ERR_PARAMETER; }
    if (n == 0 || n > (SIZE_MAX >> 8)) { set_error("uzk_srs_register_compressed: %zu points", n); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    void* d = nullptr;
    UZK_TRY(codec_register_decode("uzk_srs_register_compressed", 0, enc, n, false, &d));
    Ctx::Srs s;
    s.d_points = static_cast<Affine*>(d);
    s.n = n;
    s.owned = true;
    s.device = ctx().device;
    *handle_out = srs_insert(s);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_srs_register_compressed"); }

int uzk_g2_register_compressed(const uint8_t* enc, size_t n, int check_subgroup, uint64_t* handle_out) try {
    API_LOCK;
    if (!enc || !handle_out) { set_error("uzk_g2_register_compressed: null pointer"); return UZK_ERR_PARAMETER; }
    if (n == 0 || n > (SIZE_MAX >> 8)) { set_error("uzk_g2_register_compressed: %zu points", n); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    void* d = nullptr;
    UZK_TRY(codec_register_decode("uzk_g2_register_compressed", 1, enc, n, check_subgroup != 0, &d));
    return g2_register_owned(static_cast<G2Affine*>(d), n, ctx().device, handle_out);
} catch (...) { return uzk::on_exception("uzk_g2_register_compressed"); }

static int pk_layout_checked(const char* who, const uint8_t* pk, size_t len, bool whole_key, uzk_g16_pk_sections* out) {
    int bad = 0;
    switch (g16_pk_layout_parse(pk, len, whole_key, out, &bad)) {
        case PK_PARSE_OK: return UZK_OK;
        case PK_PARSE_TRUNCATED: set_error("%s: %zu bytes end inside %s", who, len, g16_pk_section_name(bad)); break;
        case PK_PARSE_LENGTH: set_error("%s: the length of %s does not fit the %zu bytes of the key", who, g16_pk_section_name(bad), len); break;
        case PK_PARSE_TRAILING: set_error("%s: bytes behind %s, the last section", who, g16_pk_section_name(bad)); break;
    }
    return UZK_ERR_PARAMETER;
}

int uzk_g16_pk_layout(const uint8_t* pk, size_t len, uzk_g16_pk_sections* out) try {
    if (!pk || !out) { set_error("uzk_g16_pk_layout: null pointer"); return UZK_ERR_PARAMETER; }
    return pk_layout_checked("uzk_g16_pk_layout", pk, len, true, out);
} catch (...) { return uzk::on_exception("uzk_g16_pk_layout"); }

// The points of sections [0, sections) of a key: every G1 encoding in one launch, every G2 encoding in one (two with validate).
// first[s]: where section s begins in g1 or g2.  Takes the context lock for the decoding only.
static int key_decode(const char* who, const uint8_t* key, const uzk_g16_pk_sections& lay, int sections, bool validate, std::vector<Affine>& g1,
                      std::vector<G2Affine>& g2, size_t (&first)[UZK_G16_PK_SECTIONS]) {
    std::vector<uint8_t> e1, e2;
    for (int s = 0; s < sections; ++s) {
        std::vector<uint8_t>& e = g16_pk_section_is_g2(s) ? e2 : e1;
        const size_t width = g16_pk_section_width(s);
        first[s] = e.size() / width;
        e.insert(e.end(), key + lay.offset[s], key + lay.offset[s] + (size_t)lay.count[s] * width);
    }
    const size_t n1 = e1.size() / 32, n2 = e2.size() / 64;
    if (n1 > UZK_CODEC_MAX_BATCH || n2 > UZK_CODEC_MAX_BATCH) { set_error("%s: %zu G1 and %zu G2 points (at most %d each)", who, n1, n2, UZK_CODEC_MAX_BATCH); return UZK_ERR_PARAMETER; }
    g1.resize(n1);
    g2.resize(n2);
    std::vector<uint8_t> s1(n1), s2(n2);
    {
        API_LOCK;
        UZK_TRY(require_ready());
        if (n1) UZK_TRY(codec_decompress_run(ctx(), 0, e1.data(), n1, false, g1.data(), nullptr, s1.data()));
        if (n2) UZK_TRY(codec_decompress_run(ctx(), 1, e2.data(), n2, validate, g2.data(), nullptr, s2.data()));
    }
    for (int s = 0; s < sections; ++s) {
        const std::vector<uint8_t>& st = g16_pk_section_is_g2(s) ? s2 : s1;
        for (size_t i = 0; i < lay.count[s]; ++i)
            if (st[first[s] + i]) {
                set_error("%s: %s[%zu]: status %u (1 not canonical, 2 no point, 3 outside the subgroup)", who, g16_pk_section_name(s), i, (unsigned)st[first[s] + i]);
                return UZK_ERR_PARAMETER;
            }
    }
    return UZK_OK;
}
static uzk_g1_affine as_c_g1(const Affine& p) { uzk_g1_affine r; memcpy(&r, &p, sizeof r); return r; }
static uzk_g2_affine as_c_g2(const G2Affine& p) { uzk_g2_affine r; memcpy(&r, &p, sizeof r); return r; }

int uzk_g16_vk_create_compressed(const uint8_t* key, size_t len, int validate, uint64_t* vk_out) try {
    if (!key || !vk_out) { set_error("uzk_g16_vk_create_compressed: null pointer"); return UZK_ERR_PARAMETER; }
    uzk_g16_pk_sections lay;
    UZK_TRY(pk_layout_checked("uzk_g16_vk_create_compressed", key, len, false, &lay));
    const uint64_t l = lay.count[UZK_PK_GAMMA_ABC_G1];
    if (l < 1 || l > UZK_G16_VERIFY_MAX_INPUTS) { set_error("uzk_g16_vk_create_compressed: gamma_abc_g1 of %llu points (1 .. %d)", (unsigned long long)l, UZK_G16_VERIFY_MAX_INPUTS); return UZK_ERR_PARAMETER; }
    std::vector<Affine> g1;
    std::vector<G2Affine> g2;
    size_t first[UZK_G16_PK_SECTIONS] = {};
    UZK_TRY(key_decode("uzk_g16_vk_create_compressed", key, lay, 5, validate != 0, g1, g2, first));
    uzk_g16_vk_desc d = {};
    d.n_inputs = (uint32_t)l;
    d.alpha_g1 = as_c_g1(g1[first[UZK_PK_ALPHA_G1]]);
    d.beta_g2 = as_c_g2(g2[first[UZK_PK_BETA_G2]]);
    d.gamma_g2 = as_c_g2(g2[first[UZK_PK_GAMMA_G2]]);
    d.delta_g2 = as_c_g2(g2[first[UZK_PK_DELTA_G2]]);
    d.gamma_abc_g1 = reinterpret_cast<const uzk_g1_affine*>(g1.data() + first[UZK_PK_GAMMA_ABC_G1]);
    return uzk_g16_vk_create(&d, vk_out);
} catch (...) { return uzk::on_exception("uzk_g16_vk_create_compressed"); }

int uzk_reveal_circuit_create_compressed(const uint8_t* pk, size_t len, int validate, uint64_t* circuit_out) try {
    if (!pk || !circuit_out) { set_error("uzk_reveal_circuit_create_compressed: null pointer"); return UZK_ERR_PARAMETER; }
    uzk_g16_pk_sections lay;
    UZK_TRY(pk_layout_checked("uzk_reveal_circuit_create_compressed", pk, len, true, &lay));
    const uint64_t n_vars = lay.count[UZK_PK_A_QUERY];
    if (n_vars > UINT32_MAX || lay.count[UZK_PK_GAMMA_ABC_G1] > UINT32_MAX || lay.count[UZK_PK_B_G1_QUERY] != n_vars || lay.count[UZK_PK_B_G2_QUERY] != n_vars) {
        set_error("uzk_reveal_circuit_create_compressed: a_query, b_g1_query and b_g2_query of %llu, %llu and %llu points", (unsigned long long)n_vars,
                  (unsigned long long)lay.count[UZK_PK_B_G1_QUERY], (unsigned long long)lay.count[UZK_PK_B_G2_QUERY]);
        return UZK_ERR_PARAMETER;
    }
    std::vector<Affine> g1;
    std::vector<G2Affine> g2;
    size_t first[UZK_G16_PK_SECTIONS] = {};
    UZK_TRY(key_decode("uzk_reveal_circuit_create_compressed", pk, lay, UZK_G16_PK_SECTIONS, validate != 0, g1, g2, first));
    const auto g1s = [&](int s) { return reinterpret_cast<const uzk_g1_affine*>(g1.data() + first[s]); };
    uzk_g16_key_desc d = {};
    d.n_vars = (uint32_t)n_vars;
    d.n_inputs = (uint32_t)lay.count[UZK_PK_GAMMA_ABC_G1];
    d.l_query_len = lay.count[UZK_PK_L_QUERY];
    d.h_query_len = lay.count[UZK_PK_H_QUERY];
    d.alpha_g1 = *g1s(UZK_PK_ALPHA_G1);
    d.beta_g1 = *g1s(UZK_PK_BETA_G1);
    d.delta_g1 = *g1s(UZK_PK_DELTA_G1);
    d.beta_g2 = as_c_g2(g2[first[UZK_PK_BETA_G2]]);
    d.delta_g2 = as_c_g2(g2[first[UZK_PK_DELTA_G2]]);
    d.a_query = g1s(UZK_PK_A_QUERY);
    d.b_g1_query = g1s(UZK_PK_B_G1_QUERY);
    d.l_query = g1s(UZK_PK_L_QUERY);
    d.h_query = g1s(UZK_PK_H_QUERY);
    d.b_g2_query = reinterpret_cast<const uzk_g2_affine*>(g2.data() + first[UZK_PK_B_G2_QUERY]);
    return rcs_circuit_create(&d, circuit_out);
} catch (...) { return uzk::on_exception("uzk_reveal_circuit_create_compressed"); }

int uzk_test_sqrt_kat(int field, const uint64_t* a_mont, size_t n, uint64_t* root_out, uint8_t* is_square_out) try {
    API_LOCK;
    if (field < 0 || field > 2) { set_error("uzk_test_sqrt_kat: field %d (0 Fq, 1 Fq2, 2 Fr)", field); return UZK_ERR_PARAMETER; }
    UZK_TRY(codec_batch_args("uzk_test_sqrt_kat", a_mont, n, root_out, is_square_out));
    const size_t words = field == 1 ? 2 * n : n;
    for (size_t i = 0; i < words; ++i)
        if (!(field == 2 ? below_modulus<FrCfg>(as_fp(a_mont)[i]) : below_modulus<FqCfg>(as_fp(a_mont)[i]))) {
            set_error("uzk_test_sqrt_kat: element %zu is not below the modulus", i);
            return UZK_ERR_PARAMETER;
        }
    UZK_TRY(require_ready());
    return codec_sqrt_kat_run(ctx(), field, as_fp(a_mont), n, reinterpret_cast<Fp*>(root_out), is_square_out);
} catch (...) { return uzk::on_exception("uzk_test_sqrt_kat"); }

int uzk_cp_mask_prove_batch(const uint64_t* pk_mont, const uint64_t* cards_mont, const uint64_t* rs, const uint64_t* omegas, uint32_t m, uint64_t* e1_out,
                            uint64_t* e2_out, uint8_t* proofs_out) try {
    API_LOCK;
    if (m == 0 || m > UZK_CP_MAX_BATCH) { set_error("uzk_cp_mask_prove_batch: %u cards (1 .. %d per call)", m, UZK_CP_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!pk_mont || !cards_mont || !rs || !omegas || !e1_out || !e2_out || !proofs_out) { set_error("uzk_cp_mask_prove_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(ed_require_canonical("uzk_cp_mask_prove_batch", "pk", pk_mont, 1));
    UZK_TRY(ed_require_canonical("uzk_cp_mask_prove_batch", "cards", cards_mont, m));
    UZK_TRY(require_ready());
    return cp_mask_prove_run(ctx(), as_ed(pk_mont), as_ed(cards_mont), as_fp(rs), as_fp(omegas), m, as_ed(e1_out), as_ed(e2_out), proofs_out);
} catch (...) { return uzk::on_exception("uzk_cp_mask_prove_batch"); }

int uzk_cp_mask_verify_batch(const uint64_t* pk_mont, const uint64_t* cards_mont, const uint64_t* e1_mont, const uint64_t* e2_mont, const uint8_t* proofs, uint32_t m,
                             uint8_t* verdict_out, uint64_t* challenges_out) try {
    API_LOCK;
    if (m == 0 || m > UZK_CP_MAX_BATCH) { set_error("uzk_cp_mask_verify_batch: %u proofs (1 .. %d per call)", m, UZK_CP_MAX_BATCH); return UZK_ERR_PARAMETER; }
    if (!pk_mont || !cards_mont || !e1_mont || !e2_mont || !proofs || !verdict_out) { set_error("uzk_cp_mask_verify_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return cp_mask_verify_run(ctx(), as_ed(pk_mont), as_ed(cards_mont), as_ed(e1_mont), as_ed(e2_mont), proofs, m, verdict_out, reinterpret_cast<Fp*>(challenges_out));
} catch (...) { return uzk::on_exception("uzk_cp_mask_verify_batch"); }

int uzk_test_fq12_kat(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) try {
    API_LOCK;
    if (op < 0 || op > 10) { set_error("uzk_test_fq12_kat: unknown op %d", op); return UZK_ERR_PARAMETER; }
    if (n > (1u << 20) || (n > 0 && (!a || !b || !out))) { set_error("uzk_test_fq12_kat: null pointer or more than 2^20 elements"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return pairing_kat_device(ctx(), op, reinterpret_cast<const Fq12w*>(a), reinterpret_cast<const Fq12w*>(b), reinterpret_cast<Fq12w*>(out), (uint32_t)n);
} catch (...) { return uzk::on_exception("uzk_test_fq12_kat"); }

int uzk_test_miller(const uzk_g1_affine* p, const uzk_g2_affine* q, uint32_t n, uzk_gt* out) try {
    API_LOCK;
    if (n > UZK_PAIRING_MAX_PAIRS || (n > 0 && (!p || !q || !out))) { set_error("uzk_test_miller: null pointer or too many pairs"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return pairing_miller_device(ctx(), reinterpret_cast<const Affine*>(p), reinterpret_cast<const G2Affine*>(q), n, reinterpret_cast<Fq12w*>(out));
} catch (...) { return uzk::on_exception("uzk_test_miller"); }

int uzk_test_keccak256(const uint8_t* msgs, const uint64_t* offsets, uint32_t count, uint8_t* digests_out) try {
    API_LOCK;
    if (!offsets || (count > 0 && !digests_out) || (count > 0 && offsets[count] > offsets[0] && !msgs)) { set_error("uzk_test_keccak256: null pointer"); return UZK_ERR_PARAMETER; }
    for (uint32_t i = 0; i < count; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[0] != 0) { set_error("uzk_test_keccak256: offsets must start at 0 and not decrease"); return UZK_ERR_PARAMETER; }
    }
    if (count == 0) return UZK_OK;
    UZK_TRY(require_ready());
    return vf_keccak_test(ctx(), msgs, offsets, count, digests_out);
} catch (...) { return uzk::on_exception("uzk_test_keccak256"); }

/* ---- polynomial helpers next to the hot path ------------------------------------------------ */
int uzk_poly_eval_batch(const uint64_t* coefs, uint64_t n, uint32_t batch, const uint64_t* x_mont, uint64_t* out) try {
    API_LOCK;
    if (!x_mont || (batch > 0 && (!out || (n > 0 && !coefs)))) { set_error("uzk_poly_eval_batch: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return poly_eval_batch_host(ctx(), as_fp(coefs), n, batch, *as_fp(x_mont), reinterpret_cast<Fp*>(out));
} catch (...) { return uzk::on_exception("uzk_poly_eval_batch"); }
int uzk_poly_eval_batch_device(const void* d_coefs, uint64_t n, uint32_t batch, const uint64_t* x_mont, uint64_t* out) try {
    API_LOCK;
    if (!x_mont || (batch > 0 && (!out || (n > 0 && !d_coefs)))) { set_error("uzk_poly_eval_batch_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return poly_eval_batch(ctx(), static_cast<const Fp*>(d_coefs), n, batch, *as_fp(x_mont), reinterpret_cast<Fp*>(out));
} catch (...) { return uzk::on_exception("uzk_poly_eval_batch_device"); }
int uzk_z_poly_device(const void* d_w, const uint32_t* d_perm, const void* d_group, const uint64_t* k, const uint64_t* beta_mont,
                      const uint64_t* gamma_mont, uint32_t n, uint32_t n_wires, void* d_z) try {
    API_LOCK;
    if (n > 0 && (!d_w || !d_perm || !d_group || !k || !beta_mont || !gamma_mont || !d_z)) { set_error("uzk_z_poly_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return z_poly_device(ctx(), static_cast<const Fp*>(d_w), d_perm, static_cast<const Fp*>(d_group), as_fp(k), *as_fp(beta_mont),
                         *as_fp(gamma_mont), n, n_wires, static_cast<Fp*>(d_z));
} catch (...) { return uzk::on_exception("uzk_z_poly_device"); }

int uzk_open_quotient_device(const void* d_polys, uint64_t n, uint32_t batch, const uint64_t* z_mont,
                             const uint64_t* alpha_mont, void* d_q, uint64_t* evals_out) try {
    API_LOCK;
    if (!d_polys || !z_mont || !alpha_mont || !d_q || !evals_out) { set_error("uzk_open_quotient_device: null pointer"); return UZK_ERR_PARAMETER; }
    if (d_q == d_polys) { set_error("uzk_open_quotient_device: output aliases the input"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return open_quotient_run(ctx(), static_cast<const Fp*>(d_polys), n, batch, *as_fp(z_mont), *as_fp(alpha_mont),
                             static_cast<Fp*>(d_q), reinterpret_cast<Fp*>(evals_out));
} catch (...) { return uzk::on_exception("uzk_open_quotient_device"); }

int uzk_open_quotient(const uint64_t* polys, uint64_t n, uint32_t batch, const uint64_t* z_mont, const uint64_t* alpha_mont,
                      uint64_t* q_out, uint64_t* evals_out) try {
    API_LOCK;
    if (!polys || !z_mont || !alpha_mont || !q_out || !evals_out) { set_error("uzk_open_quotient: null pointer"); return UZK_ERR_PARAMETER; }
    if (n == 0 || batch == 0) { set_error("uzk_open_quotient: need batch > 0 and n > 0"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    const size_t in_bytes = (size_t)n * batch * sizeof(Fp);
    UZK_TRY(c.poly_io.reserve(in_bytes + (size_t)n * sizeof(Fp)));
    Fp* d_p = c.poly_io.as<Fp>();
    Fp* d_q = d_p + (size_t)n * batch;
    UZK_HIP(hipMemcpyAsync(d_p, polys, in_bytes, hipMemcpyHostToDevice, c.stream));
    UZK_TRY(open_quotient_run(c, d_p, n, batch, *as_fp(z_mont), *as_fp(alpha_mont), d_q, reinterpret_cast<Fp*>(evals_out)));
    UZK_HIP(hipMemcpyAsync(q_out, d_q, (size_t)n * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_open_quotient"); }

int uzk_fold_blinds_device(const void* d_coefs, uint64_t len, uint64_t n_fold, void* d_out, uint64_t* blinds_out) try {
    API_LOCK;
    if (!d_coefs || !d_out || (len > n_fold && !blinds_out)) { set_error("uzk_fold_blinds_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return fold_blinds_run(ctx(), static_cast<const Fp*>(d_coefs), len, n_fold, static_cast<Fp*>(d_out), reinterpret_cast<Fp*>(blinds_out));
} catch (...) { return uzk::on_exception("uzk_fold_blinds_device"); }

int uzk_poly_lincomb_device(const void* const* d_polys, const uint64_t* lens, const uint64_t* scalars_mont, uint32_t count,
                            void* d_out, uint64_t out_len) try {
    API_LOCK;
    if (!d_polys || !lens || !scalars_mont || (out_len > 0 && !d_out)) { set_error("uzk_poly_lincomb_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return poly_lincomb_run(ctx(), d_polys, lens, as_fp(scalars_mont), count, static_cast<Fp*>(d_out), out_len);
} catch (...) { return uzk::on_exception("uzk_poly_lincomb_device"); }

int uzk_hide_polynomial_device(void* d_coefs, uint64_t len, const uint64_t* blinds_mont, uint32_t hiding_degree, uint64_t zeroing_degree) try {
    API_LOCK;
    if (!d_coefs || (hiding_degree > 0 && !blinds_mont)) { set_error("uzk_hide_polynomial_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return poly_hide_run(ctx(), static_cast<Fp*>(d_coefs), len, as_fp(blinds_mont), hiding_degree, zeroing_degree);
} catch (...) { return uzk::on_exception("uzk_hide_polynomial_device"); }

int uzk_hide_polynomial_batch_device(void* d_coefs, uint64_t stride, uint64_t len_in, uint32_t count, const uint64_t* blinds_mont,
                                     uint32_t hiding_degree, uint64_t zeroing_degree) try {
    API_LOCK;
    if (count > 0 && hiding_degree > 0 && (!d_coefs || !blinds_mont)) { set_error("uzk_hide_polynomial_batch_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return poly_hide_batch_run(ctx(), static_cast<Fp*>(d_coefs), stride, len_in, count, as_fp(blinds_mont), hiding_degree, zeroing_degree);
} catch (...) { return uzk::on_exception("uzk_hide_polynomial_batch_device"); }

int uzk_fold_blinds_batch_device(const void* d_polys, uint64_t in_stride, const uint64_t* lens, uint64_t n_fold, uint32_t batch, void* d_out,
                                 uint64_t out_stride, void* d_tail, uint32_t tail_n, uint64_t* blinds_out) try {
    API_LOCK;
    if (batch > 0 && (!d_polys || !lens || !d_out || (tail_n > 0 && !d_tail))) { set_error("uzk_fold_blinds_batch_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return fold_blinds_batch_run(ctx(), static_cast<const Fp*>(d_polys), in_stride, lens, n_fold, batch, static_cast<Fp*>(d_out), out_stride,
                                 static_cast<Fp*>(d_tail), tail_n, reinterpret_cast<Fp*>(blinds_out));
} catch (...) { return uzk::on_exception("uzk_fold_blinds_batch_device"); }

int uzk_poly_trimmed_len_device(const void* d_polys, uint64_t stride, const uint64_t* lens, uint32_t batch, uint64_t* out_lens, int sync) try {
    API_LOCK;
    if (batch > 0 && (!d_polys || !lens || !out_lens)) { set_error("uzk_poly_trimmed_len_device: null pointer"); return UZK_ERR_PARAMETER; }
    if (!sync && batch > 0 && !is_pinned_block(out_lens, batch * sizeof(uint64_t))) {
        set_error("uzk_poly_trimmed_len_device: an asynchronous call needs out_lens in uzk_host_alloc memory");
        return UZK_ERR_PARAMETER;
    }
    UZK_TRY(require_ready());
    return poly_trimmed_len_run(ctx(), static_cast<const Fp*>(d_polys), stride, lens, batch, out_lens, sync != 0);
} catch (...) { return uzk::on_exception("uzk_poly_trimmed_len_device"); }

int uzk_split_t_device(const void* d_t, uint64_t t_len, uint64_t chunk, uint32_t n_chunks, const uint64_t* rands_mont, void* d_chunks,
                       uint64_t chunk_stride, uint64_t* lens_out) try {
    API_LOCK;
    if (!d_t || !rands_mont || !d_chunks) { set_error("uzk_split_t_device: null pointer"); return UZK_ERR_PARAMETER; }
    if (d_t == d_chunks) { set_error("uzk_split_t_device: output aliases the input"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return split_t_run(ctx(), static_cast<const Fp*>(d_t), t_len, chunk, n_chunks, as_fp(rands_mont), static_cast<Fp*>(d_chunks), chunk_stride, lens_out);
} catch (...) { return uzk::on_exception("uzk_split_t_device"); }

int uzk_poly_eval_ptrs_device(const void* const* d_polys, const uint64_t* lens, const uint32_t* point_idx, uint32_t count,
                              const uint64_t* points_mont, uint32_t n_points, uint64_t* out) try {
    API_LOCK;
    if (count > 0 && (!d_polys || !lens || !point_idx || !points_mont || !out)) { set_error("uzk_poly_eval_ptrs_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return poly_eval_ptrs(ctx(), d_polys, lens, point_idx, count, as_fp(points_mont), n_points, reinterpret_cast<Fp*>(out));
} catch (...) { return uzk::on_exception("uzk_poly_eval_ptrs_device"); }

int uzk_open_quotient_ptrs_device(const void* const* d_polys, const uint64_t* lens, uint32_t count, const uint64_t* z_mont,
                                  const uint64_t* alpha_mont, void* d_q, uint64_t q_cap, uint64_t* evals_out) try {
    API_LOCK;
    if (!d_polys || !lens || !z_mont || !alpha_mont || !d_q) { set_error("uzk_open_quotient_ptrs_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return open_quotient_ptrs(ctx(), d_polys, lens, count, *as_fp(z_mont), *as_fp(alpha_mont), static_cast<Fp*>(d_q), q_cap,
                              reinterpret_cast<Fp*>(evals_out));
} catch (...) { return uzk::on_exception("uzk_open_quotient_ptrs_device"); }

int uzk_t_quotient_device(const uzk_quotient_args* args, void* d_out, int sync) try {
    API_LOCK;
    if (!args || !d_out) { set_error("uzk_t_quotient_device: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    static_assert(sizeof(uzk_quotient_args) == 8 + 56 * sizeof(void*) + (3 + 5 + 3 + 16) * 32, "ABI layout");
    UZK_TRY(t_quotient_run(ctx(), args, static_cast<Fp*>(d_out)));
    if (sync) UZK_HIP(hipStreamSynchronize(ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_t_quotient_device"); }

int uzk_z_poly(const uint64_t* w, const uint32_t* perm, const uint64_t* group, const uint64_t* k, const uint64_t* beta_mont,
               const uint64_t* gamma_mont, uint32_t n, uint32_t n_wires, uint64_t* z_out) try {
    API_LOCK;
    if (!w || !perm || !group || !k || !beta_mont || !gamma_mont || !z_out) { set_error("uzk_z_poly: null pointer"); return UZK_ERR_PARAMETER; }
    if (n_wires == 0 || n_wires > 8 || (uint64_t)n * n_wires >= (1ull << 32)) { set_error("uzk_z_poly: bad shape"); return UZK_ERR_PARAMETER; }
    // the kernel indexes k[perm / n] (eight entries) and group[perm % n] unchecked: refuse a foreign index before any launch
    for (uint64_t i = 0, total = (uint64_t)n * n_wires; i < total; ++i)
        if (perm[i] >= total) { set_error("uzk_z_poly: perm[%llu] = %u is not below n_wires * n = %llu", (unsigned long long)i, perm[i], (unsigned long long)total); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return z_poly_run(ctx(), as_fp(w), perm, as_fp(group), as_fp(k), *as_fp(beta_mont), *as_fp(gamma_mont), n, n_wires,
                      reinterpret_cast<Fp*>(z_out));
} catch (...) { return uzk::on_exception("uzk_z_poly"); }

/* ---- synthetic workloads ------------------------------------------------------------------ */
int uzk_synth_points_arith(void* d_points, size_t n, const uint64_t* seed_scalar_mont) try {
    API_LOCK;
    if ((n > 0 && !d_points) || !seed_scalar_mont) { set_error("uzk_synth_points_arith: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return synth_points_arith(ctx(), static_cast<Affine*>(d_points), n, *as_fp(seed_scalar_mont));
} catch (...) { return uzk::on_exception("uzk_synth_points_arith"); }
int uzk_synth_points_random(void* d_points, size_t n, uint64_t seed) try {
    API_LOCK;
    if (n > 0 && !d_points) { set_error("uzk_synth_points_random: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    UZK_TRY(synth_points_random(ctx(), static_cast<Affine*>(d_points), n, seed));
    UZK_HIP(hipStreamSynchronize(ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_synth_points_random"); }
int uzk_synth_scalars(void* d_scalars, size_t n, uint64_t seed) try {
    API_LOCK;
    if (n > 0 && !d_scalars) { set_error("uzk_synth_scalars: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    UZK_TRY(synth_scalars(ctx(), static_cast<Fp*>(d_scalars), n, seed));
    UZK_HIP(hipStreamSynchronize(ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_synth_scalars"); }

int uzk_synth_scalars_mix(void* d_scalars, size_t n, uint64_t seed) try {
    API_LOCK;
    if (n > 0 && !d_scalars) { set_error("uzk_synth_scalars_mix: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    UZK_TRY(synth_scalars_mix(ctx(), static_cast<Fp*>(d_scalars), n, seed));
    UZK_HIP(hipStreamSynchronize(ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_synth_scalars_mix"); }

/* ---- element-wise field arithmetic on host arrays (product: the host mirrors' helper) ----------- */
int uzk_field_op_device(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!a || !b || !out)) { set_error("uzk_field_op_device: null pointer"); return UZK_ERR_PARAMETER; }
    const bool known = op == 0 || op == 1 || op == 2 || op == 4 || op == 5 || op == 6 || op == 7;
    if (field < 0 || field > 1 || !known) { set_error("uzk_field_op_device: bad field/op (mul, add, sub, sqr, neg, from_mont, to_mont)"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return field_op_device(ctx(), field, op, as_fp(a), as_fp(b), reinterpret_cast<Fp*>(out), n);
} catch (...) { return uzk::on_exception("uzk_field_op_device"); }

/* ---- test hooks (include/uzkge_gpu_test.h): known-answer entry points of the arithmetic cores ---- */
int uzk_test_field_kat(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!a || !b || !out)) { set_error("uzk_test_field_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (field < 0 || field > 1 || op < 0 || op > 33) { set_error("uzk_test_field_kat: bad field/op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return field_op_device(ctx(), field, op, as_fp(a), as_fp(b), reinterpret_cast<Fp*>(out), n);
} catch (...) { return uzk::on_exception("uzk_test_field_kat"); }
int uzk_test_const_operands(int field, int op, int form_a, int form_b, int portable, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!a || !b || !out)) { set_error("uzk_test_const_operands: null pointer"); return UZK_ERR_PARAMETER; }
    if (field < 0 || field > 1 || portable < 0 || portable > 1 || !const_operand_case_known(op, form_a, form_b)) {
        set_error("uzk_test_const_operands: bad field, or no kernel of this (op, form, form)");
        return UZK_ERR_PARAMETER;
    }
    UZK_TRY(require_ready());
    return const_operand_device(ctx(), field, op, form_a, form_b, portable != 0, as_fp(a), as_fp(b), reinterpret_cast<Fp*>(out), n);
} catch (...) { return uzk::on_exception("uzk_test_const_operands"); }
int uzk_test_g1_kat(int op, const uzk_g1_affine* a, const uzk_g1_affine* b, uzk_g1_jac* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!a || !b || !out)) { set_error("uzk_test_g1_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (op < 0 || op > 21) { set_error("uzk_test_g1_kat: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return g1_op_device(ctx(), op, reinterpret_cast<const Affine*>(a), reinterpret_cast<const Affine*>(b),
                        reinterpret_cast<Jac*>(out), n);
} catch (...) { return uzk::on_exception("uzk_test_g1_kat"); }

int uzk_test_g16_finish(const uzk_g1_jac* a_jac, const uzk_g1_jac* b1_jac, const uzk_g1_jac* k_jac, const uint64_t* r_mont, const uint64_t* s_mont, size_t n,
                        uzk_g1_affine* a_out, uzk_g1_affine* c_out) try {
    API_LOCK;
    if (n == 0) return UZK_OK;
    if (!a_jac || !b1_jac || !k_jac || !r_mont || !s_mont || !a_out || !c_out) { set_error("uzk_test_g16_finish: null pointer"); return UZK_ERR_PARAMETER; }
    if (n > 4096) { set_error("uzk_test_g16_finish: more than 4096 records"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return g16_finish_test_run(ctx(), reinterpret_cast<const Jac*>(a_jac), reinterpret_cast<const Jac*>(b1_jac), reinterpret_cast<const Jac*>(k_jac), as_fp(r_mont),
                               as_fp(s_mont), (uint32_t)n, reinterpret_cast<Affine*>(a_out), reinterpret_cast<Affine*>(c_out));
} catch (...) { return uzk::on_exception("uzk_test_g16_finish"); }

int uzk_test_g16_plan(uint32_t n_vars, uint32_t n_inputs, uint32_t n_constraints, uint32_t* group_out, uint64_t lens_out[3], int admitted_out[3]) try {
    API_LOCK;
    if (!group_out || !lens_out || !admitted_out) { set_error("uzk_test_g16_plan: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());                         // the admission depends on the calling context's tuning
    return g16_plan_test(ctx(), n_vars, n_inputs, n_constraints, group_out, lens_out, admitted_out);
} catch (...) { return uzk::on_exception("uzk_test_g16_plan"); }

int uzk_test_g2_kat(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!a || !b || !out)) { set_error("uzk_test_g2_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (op < 0 || (op > 5 && op < 10) || op > 14) { set_error("uzk_test_g2_kat: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return g2_op_device(ctx(), op, a, b, out, n);
} catch (...) { return uzk::on_exception("uzk_test_g2_kat"); }

int uzk_test_l29_kat(int field, int op, uint32_t param, const uint32_t* in, uint32_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!in || !out)) { set_error("uzk_test_l29_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (field < 0 || field > 1 || op < 0 || op > 22) { set_error("uzk_test_l29_kat: bad field/op"); return UZK_ERR_PARAMETER; }
    if (op == 20 && param > 5) { set_error("uzk_test_l29_kat: sub_off takes offsets 0 .. 5"); return UZK_ERR_PARAMETER; }
    if (op == 21 && !l29_sig_runnable(field, param)) { set_error("uzk_test_l29_kat: not a sub / to_wire / canon signature of this field"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return l29_op_device(ctx(), field, op, param, in, out, n);
} catch (...) { return uzk::on_exception("uzk_test_l29_kat"); }
int uzk_test_p29_kat(int op, const uint32_t* in, uint32_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!in || !out)) { set_error("uzk_test_p29_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (op < 0 || op > 3) { set_error("uzk_test_p29_kat: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return p29_op_device(ctx(), op, in, out, n);
} catch (...) { return uzk::on_exception("uzk_test_p29_kat"); }
int uzk_test_g2_raw_kat(int op, const uint32_t* in, uint32_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!in || !out)) { set_error("uzk_test_g2_raw_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (op < 0 || op > 4) { set_error("uzk_test_g2_raw_kat: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return g2_raw_op_device(ctx(), op, in, out, n);
} catch (...) { return uzk::on_exception("uzk_test_g2_raw_kat"); }
int uzk_test_fq12_raw_kat(int op, const uint32_t* in, uint32_t* out, size_t n) try {
    API_LOCK;
    if (n > (1u << 20) || (n > 0 && (!in || !out))) { set_error("uzk_test_fq12_raw_kat: null pointer or more than 2^20 elements"); return UZK_ERR_PARAMETER; }
    if (op < 0 || op > 12) { set_error("uzk_test_fq12_raw_kat: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return pairing_raw_kat_device(ctx(), op, in, out, (uint32_t)n);
} catch (...) { return uzk::on_exception("uzk_test_fq12_raw_kat"); }
int uzk_test_miller_step_raw(int op, const uint32_t* in, uint32_t* out, size_t n) try {
    API_LOCK;
    if (n > (1u << 20) || (n > 0 && (!in || !out))) { set_error("uzk_test_miller_step_raw: null pointer or more than 2^20 records"); return UZK_ERR_PARAMETER; }
    if (op < 0 || op > 1) { set_error("uzk_test_miller_step_raw: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return pairing_raw_step_device(ctx(), op, in, out, (uint32_t)n);
} catch (...) { return uzk::on_exception("uzk_test_miller_step_raw"); }
int uzk_test_ed_raw_kat(int op, const uint32_t* in, uint32_t* out, size_t n) try {
    API_LOCK;
    if (n > 0 && (!in || !out)) { set_error("uzk_test_ed_raw_kat: null pointer"); return UZK_ERR_PARAMETER; }
    if (op < 0 || op > 6) { set_error("uzk_test_ed_raw_kat: bad op"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return ed_raw_op_device(ctx(), op, in, out, n);
} catch (...) { return uzk::on_exception("uzk_test_ed_raw_kat"); }
int uzk_test_lanes(int op, const void* const* d_polys, const uint64_t* lane_strides, uint32_t count, const uint32_t* lens, const uint32_t* pts,
                   const uint64_t* args, uint32_t lanes, uint64_t len, uint64_t* out, int* kernel) try {
    API_LOCK;
    if (op < 0 || op > 1 || count == 0 || lanes == 0 || !kernel) { set_error("uzk_test_lanes: bad op / count / lanes"); return UZK_ERR_PARAMETER; }
    if (!d_polys || !lane_strides || !lens || !args || !out || (op == 1 && !pts)) { set_error("uzk_test_lanes: null pointer"); return UZK_ERR_PARAMETER; }
    for (uint32_t k = 0; k < count; ++k)
        if (!d_polys[k] || (op == 1 && pts[k] > 1)) { set_error("uzk_test_lanes: null polynomial or point index > 1"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    return lanes_test(ctx(), op, d_polys, lane_strides, count, lens, pts, as_fp(args), lanes, len, reinterpret_cast<Fp*>(out), kernel);
} catch (...) { return uzk::on_exception("uzk_test_lanes"); }
// uzk_ntt_fr_batch_strided_device (forward) with ntt_run's in_len, which only the prover passes (prover.cpp derive_cosets, round 3)
int uzk_test_ntt_in_len(const void* d_in, uint64_t in_stride, void* d_out, uint64_t out_stride, uint64_t n, uint32_t batch,
                        const uint64_t* coset_shift_mont, uint64_t in_len) try {
    API_LOCK;
    if (!domain_supported(n)) {
        set_error("no evaluation domain of size %llu (need 2^k, k <= %d, or 3 * 2^k, k <= %d)", (unsigned long long)n, UZK_NTT_MAX_LOG2, UZK_NTT_MAX_LOG2_MIXED);
        return UZK_ERR_FFT;
    }
    if (!d_in || !d_out) { set_error("uzk_test_ntt_in_len: null pointer"); return UZK_ERR_PARAMETER; }
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(ntt_run(c, static_cast<const Fp*>(d_in), static_cast<Fp*>(d_out), n, false,
                    coset_shift_mont ? as_fp(coset_shift_mont) : nullptr, batch, in_stride, out_stride, in_len));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_test_ntt_in_len"); }

/* ---- measurement -------------------------------------------------------------------------- */
int uzk_profile_enable(int on) try {
    API_LOCK;
    UZK_TRY(require_ready());
    Ctx& c = ctx();
    UZK_TRY(c.prof_collect());
    c.prof_on = on != 0;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_profile_enable"); }
int uzk_profile_reset(void) try {
    API_LOCK;
    Ctx& c = ctx();
    if (c.ready) UZK_TRY(c.prof_collect());
    c.prof_totals.clear();
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_profile_reset"); }
int uzk_profile_get(const char* name, double* total_ms, uint64_t* launches) try {
    API_LOCK;
    Ctx& c = ctx();
    if (!name) { set_error("uzk_profile_get: null name"); return UZK_ERR_PARAMETER; }
    if (c.ready) UZK_TRY(c.prof_collect());
    auto it = c.prof_totals.find(name);
    if (total_ms) *total_ms = (it == c.prof_totals.end()) ? 0.0 : it->second.first;
    if (launches) *launches = (it == c.prof_totals.end()) ? 0 : it->second.second;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_profile_get"); }
int uzk_profile_dump(char* buf, size_t cap) try {
    API_LOCK;
    Ctx& c = ctx();
    if (!buf || cap == 0) { set_error("uzk_profile_dump: null buffer"); return UZK_ERR_PARAMETER; }
    if (c.ready) UZK_TRY(c.prof_collect());
    size_t off = 0;
    buf[0] = 0;
    for (auto& kv : c.prof_totals) {
        int w = snprintf(buf + off, cap - off, "%s %llu %.6f\n", kv.first.c_str(),
                         (unsigned long long)kv.second.second, kv.second.first);
        if (w < 0 || (size_t)w >= cap - off) break;
        off += (size_t)w;
    }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_profile_dump"); }
int uzk_sync(void) try {
    API_LOCK;
    UZK_TRY(require_ready());
    UZK_HIP(hipStreamSynchronize(ctx().stream));
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_sync"); }
void* uzk_stream(void) {
    API_LOCK;
    if (require_ready() != UZK_OK) return nullptr;
    return ctx().stream;
}
int uzk_msm_set_window_bits(int c) try {
    API_LOCK;
    if (c != 0 && (c < 4 || c > 22)) { set_error("window bits must be 0 (auto) or 4..22"); return UZK_ERR_PARAMETER; }
    ctx().msm_window_bits = c;
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_set_window_bits"); }

int uzk_msm_plan_info(size_t n, int* window_bits, int* windows) try {
    API_LOCK;
    if (!window_bits || !windows || n == 0) { set_error("uzk_msm_plan_info: bad arguments"); return UZK_ERR_PARAMETER; }
    msm_plan_info(ctx(), n, window_bits, windows);
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_msm_plan_info"); }

int uzk_tune(const char* key, int value) try {
    API_LOCK;
    if (!key) { set_error("uzk_tune: null key"); return UZK_ERR_PARAMETER; }
    Ctx& c = ctx();
    if (!std::strcmp(key, "msm_no_precompute")) c.tune_no_precompute = value;
    else if (!std::strcmp(key, "msm_stream_log")) c.tune_stream_log = (value >= -1 && value <= 26) ? value : 0;
    else if (!std::strcmp(key, "msm_stream_min_log")) c.tune_stream_min_log = (value >= 4 && value <= 26) ? value : 22;
    else if (!std::strcmp(key, "msm_chunk_log")) c.tune_chunk_log = (value >= 8 && value <= 26) ? value : 26;
    else if (!std::strcmp(key, "msm_small")) c.tune_small = value ? 1 : 0;
    else if (!std::strcmp(key, "msm_seg_sort")) c.tune_seg_sort = value;
    else if (!std::strcmp(key, "msm_taper")) c.tune_msm_taper = (value >= 0 && value <= 2) ? value : 1;
    else if (!std::strcmp(key, "ntt_tile")) c.tune_ntt_tile = (value == 1024 || value == 2048) ? value : 0;
    else if (!std::strcmp(key, "ntt_two_pass")) c.tune_ntt_two_pass = value ? 1 : 0;
    else if (!std::strcmp(key, "arith29")) c.tune_arith29 = value & 7;
    else if (!std::strcmp(key, "verify_transcript")) c.tune_verify_transcript = (value == 1 || value == 2) ? value : 0;
    else { set_error("uzk_tune: unknown key %s", key); return UZK_ERR_PARAMETER; }
    return UZK_OK;
} catch (...) { return uzk::on_exception("uzk_tune"); }

}  // extern "C"
