// Anemoi-Jive on the device, batched one lane per item (anemoi29.hpp has the permutation and the sponge).
//
//   anemoi_permute   one lane per state (x0 x1 y0 y1): one permutation
//   anemoi_sponge    one lane per input of `len` elements: the whole sponge of eval_variable_length_hash (out_len == 0: one output) or
//                    eval_stream_cipher (out_len outputs), P = uzk_anemoi_permutations(len, out_len) permutations one after the other;
//                    with a trace every permutation's 64 elements go to the item's P x 64 block as they are computed
//
// A permutation is 28 fifth roots of ~340 dependent products each, two chains side by side in a lane: the latency of a call is
// P permutations whatever the batch, until the chip is full.  No shared memory, no scratch, 64 lanes per workgroup.  The host splits
// a batch whose buffers would pass kAnemoiChunkBytes into launches over slices of the items.  tests/anemoi_ref.py is the
// restatement on Python integers.
#include "anemoi29.hpp"
#include "ctx.hpp"
#include "handles.hpp"

namespace uzk {

constexpr uint32_t kAnemoiBlock = 64;
constexpr size_t kAnemoiChunkBytes = (size_t)1 << 30;               // device buffers of one launch (inputs, outputs, trace)

__global__ __launch_bounds__(kAnemoiBlock) void anemoi_permute_kernel(const Fp* __restrict__ in, Fp* __restrict__ out, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kAnemoiBlock + threadIdx.x;
    if (i >= n) return;
    const Fp* w = in + 4 * (size_t)i;
    anemoi::State s;
    s.x0 = anemoi::ld(w[0]); s.x1 = anemoi::ld(w[1]); s.y0 = anemoi::ld(w[2]); s.y1 = anemoi::ld(w[3]);
    anemoi::permute(&s, nullptr);
    anemoi::put4(out + 4 * (size_t)i, s);
#endif
}

__global__ __launch_bounds__(kAnemoiBlock) void anemoi_sponge_kernel(const Fp* __restrict__ in, uint32_t len, uint32_t out_len, Fp* __restrict__ out,
                                                                      Fp* __restrict__ trace, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kAnemoiBlock + threadIdx.x;
    if (i >= n) return;
    const Fp* w = in + (size_t)len * i;
    const uint32_t outs = out_len ? out_len : 1, perms = anemoi_permutations(len, out_len);
    anemoi::sponge([w](uint32_t k) { return w[k]; }, len, out_len, out + (size_t)outs * i,
                   trace ? trace + (size_t)i * perms * kAnemoiTraceElems : nullptr);
#endif
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static unsigned an_grid(size_t lanes) { return (unsigned)((lanes + kAnemoiBlock - 1) / kAnemoiBlock); }
// items per launch: all of them, or as many whole workgroups as keep the launch's buffers below kAnemoiChunkBytes
static size_t an_chunk(size_t n, size_t item_bytes) {
    size_t fit = kAnemoiChunkBytes / item_bytes;
    if (fit >= n) return n;
    if (fit > kAnemoiBlock) fit -= fit % kAnemoiBlock;
    return fit ? fit : 1;
}

int anemoi_permute_run(Ctx& c, const Fp* states, size_t n, Fp* out) {
    const size_t item = 4 * sizeof(Fp), chunk = an_chunk(n, 2 * item);
    WsCarver cv;
    const auto a_in = cv.array<Fp>(chunk * 4), a_out = cv.array<Fp>(chunk * 4);
    UZK_TRY(cv.reserve(c.ed_ws));
    Fp *d_in = cv(a_in), *d_out = cv(a_out);
    for (size_t first = 0; first < n; first += chunk) {
        const size_t count = n - first < chunk ? n - first : chunk;
        UZK_HIP(hipMemcpyAsync(d_in, states + 4 * first, count * item, hipMemcpyHostToDevice, c.stream));
        UZK_LAUNCH(c, "anemoi_permute", anemoi_permute_kernel, dim3(an_grid(count)), dim3(kAnemoiBlock), 0, c.stream, d_in, d_out, (uint32_t)count);
        UZK_HIP(hipMemcpyAsync(out + 4 * first, d_out, count * item, hipMemcpyDeviceToHost, c.stream));
    }
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// out_len == 0: the hash (one output per item); trace_out: null or n x P x 64 elements
int anemoi_sponge_run(Ctx& c, const Fp* inputs, uint32_t len, size_t n, uint32_t out_len, Fp* out, Fp* trace_out) {
    const uint32_t outs = out_len ? out_len : 1, perms = anemoi_permutations(len, out_len);
    const size_t in_item = (size_t)len * sizeof(Fp), out_item = (size_t)outs * sizeof(Fp);
    const size_t tr_item = trace_out ? (size_t)perms * kAnemoiTraceElems * sizeof(Fp) : 0;
    const size_t chunk = an_chunk(n, in_item + out_item + tr_item);
    WsCarver cv;
    const auto a_in = cv.array<Fp>(chunk * len), a_out = cv.array<Fp>(chunk * outs), a_tr = cv.array<Fp>(chunk * (tr_item / sizeof(Fp)));
    UZK_TRY(cv.reserve(c.ed_ws));
    Fp *d_in = cv(a_in), *d_out = cv(a_out), *d_tr = trace_out ? cv(a_tr) : nullptr;
    for (size_t first = 0; first < n; first += chunk) {
        const size_t count = n - first < chunk ? n - first : chunk;
        if (len) UZK_HIP(hipMemcpyAsync(d_in, inputs + first * len, count * in_item, hipMemcpyHostToDevice, c.stream));
        UZK_LAUNCH(c, trace_out ? "anemoi_sponge_trace" : "anemoi_sponge", anemoi_sponge_kernel, dim3(an_grid(count)), dim3(kAnemoiBlock), 0, c.stream, d_in, len, out_len, d_out, d_tr, (uint32_t)count);
        UZK_HIP(hipMemcpyAsync(out + first * outs, d_out, count * out_item, hipMemcpyDeviceToHost, c.stream));
        if (trace_out)
            UZK_HIP(hipMemcpyAsync(reinterpret_cast<char*>(trace_out) + first * tr_item, d_tr, count * tr_item, hipMemcpyDeviceToHost, c.stream));
    }
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int anemoi_sponge_device(Ctx& c, const Fp* d_inputs, uint32_t len, uint32_t n, uint32_t out_len, Fp* d_out, Fp* d_trace) {
    UZK_LAUNCH(c, d_trace ? "anemoi_sponge_trace" : "anemoi_sponge", anemoi_sponge_kernel, dim3(an_grid(n)), dim3(kAnemoiBlock), 0, c.stream, d_inputs, len, out_len, d_out, d_trace, n);
    return UZK_OK;
}

}  // namespace uzk
