// zmatchmaking's circuit on the device (include/uzkge_gpu.h, "the matchmaking circuit"): the evaluation vectors of its tables and the
// witnesses of `batch` matches, from the compact layout of matchcs.hpp and the two Anemoi traces anemoi_sponge_device leaves in HBM.
//   cs_tables    per row: 9 q (small signed integers into Fr), 5 s (one product k[w] omega^i each), qb, 4 q_prk    19 stores of 32 B
//   mcs_steps    one wave of 64 lanes per match.  Lane i (1 <= i < N) takes stream output i - 1 out of Montgomery form and divides its
//                eight 32-bit words by i + 1 <= 64.  Then LANE j HOLDS POSITION j of the running output vector as an index into the
//                inputs, in a register, and the N - 1 steps run one after the other: step i exchanges positions i and rem_i.  The only
//                traffic between positions is two __shfl reads per step, which take every lane's value BEFORE any lane assigns its own,
//                so there is no memory cell two lanes could race on.  The vector before every step goes out as a row of 64 bytes
//   mcs_values   per (match, variable): the variable's definition in Fr -- a load, a small integer, or an input picked through a row
//                of the step kernel's index table.  No sum is formed: a running sum of one-hot bits is rem < count, a running sum of
//                the products is the picked input or zero
//   cs_gather    per (match, wire, row): extended[w][row] = value[wiring[w][row]]; the 2 N + 2 items behind them: the public inputs
// Every launch but mcs_steps moves 32-byte elements and does next to no arithmetic; mcs_steps is N - 1 dependent steps of two
// cross-lane reads and a 64-byte store.  A match's cost is its 18 (N = 50) serial Anemoi permutations, not these.
#include "matchcs_dev.hpp"

namespace uzk {

#if defined(__HIP_DEVICE_COMPILE__)
// Long division of a plain 256-bit integer by m, 2 <= m <= 64, sixteen bits at a time from the top: the running remainder stays
// below m, so every partial dividend is below 2^22 and every partial quotient below 2^16.  Returns the remainder.
__device__ __forceinline__ uint32_t mcs_divrem(const Fp& plain, uint32_t m, Fp* quot) {
    uint32_t rem = 0;
#pragma unroll
    for (int w = 7; w >= 0; --w) {
        const uint32_t hi = rem << 16 | plain.v[w] >> 16;
        const uint32_t qh = hi / m;
        rem = hi - qh * m;
        const uint32_t lo = rem << 16 | (plain.v[w] & 0xffffu);
        const uint32_t ql = lo / m;
        rem = lo - ql * m;
        quot->v[w] = qh << 16 | ql;
    }
    return rem;
}
#endif

// one wave per match; every lane runs to the end (the shuffles read all 64)
__global__ __launch_bounds__(kMcsLanes) void mcs_steps_kernel(McsWitnessArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lane = threadIdx.x, match = blockIdx.x, N = a.players;
    uint32_t my_rem = 0;
    if (lane >= 1 && lane < N) {
        Fp q;
        my_rem = mcs_divrem(Fr::from_mont(a.stream_out[(size_t)match * (N - 1) + (lane - 1)]), lane + 1, &q);
        a.quot[(size_t)match * kMcsLanes + lane] = Fr::to_mont(q);
    }
    a.rem[(size_t)match * kMcsLanes + lane] = (uint8_t)my_rem;
    uint8_t* state = a.state + (size_t)match * (N + 1) * kMcsLanes;
    uint32_t idx = lane;                                           // position `lane` of the running output vector, as an index into the inputs
    for (uint32_t i = 1; i < N; ++i) {
        state[(size_t)i * kMcsLanes + lane] = (uint8_t)idx;
        const uint32_t r = (uint32_t)__shfl((int)my_rem, (int)i);  // rem_i <= i: the same in every lane
        const uint32_t at_i = (uint32_t)__shfl((int)idx, (int)i), at_r = (uint32_t)__shfl((int)idx, (int)r);
        if (lane == i) idx = at_r;                                 // the sum of the products: the output picked by the one-hot bits
        else if (lane == r) idx = at_i;                            // select(output_r, output_i, bit_r = 1); every other select keeps its own
    }
    state[(size_t)N * kMcsLanes + lane] = (uint8_t)idx;
#endif
}

__global__ __launch_bounds__(kCsBlock) void mcs_values_kernel(McsWitnessArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t v = blockIdx.x * kCsBlock + threadIdx.x, match = blockIdx.y, N = a.players;
    if (v >= a.num_vars) return;
    const uint32_t d = a.defs[v], kind = cs_def_kind(d), x = cs_def_a(d), y = cs_def_b(d);
    const Fp* in = a.inputs + (size_t)match * N;
    const uint8_t* state = a.state + (size_t)match * (N + 1) * kMcsLanes;
    // steps are x = 1 .. N - 1 in every kind that reads them (matchcs_layout.cpp; tests/cpp/matchcs_host.cpp checks every operand)
    const uint32_t rem = kind >= kMcsRem ? a.rem[(size_t)match * kMcsLanes + x] : 0;
    Fp r = Fr::zero();
    switch (kind) {
    case kMcsConst: r = cs_small((int)x); break;
    case kMcsInput: r = in[x]; break;
    case kMcsSeed: r = a.seeds[match]; break;
    case kMcsRandom: r = a.randoms[match]; break;
    case kMcsCommit: r = a.commit[match]; break;
    case kMcsHashTrace: r = a.hash_trace[((size_t)match + x) * kMcsTraceElems + y]; break;
    case kMcsStreamTrace: r = a.stream_trace[((size_t)match * a.stream_perms + x) * kMcsTraceElems + y]; break;
    case kMcsStreamOut: r = a.stream_out[(size_t)match * (N - 1) + x]; break;
    case kMcsQuot: r = a.quot[(size_t)match * kMcsLanes + x]; break;
    case kMcsRem: r = cs_small((int)rem); break;
    case kMcsBit: r = cs_bit(rem == y); break;
    case kMcsBitSum: r = cs_bit(rem < y); break;
    case kMcsProduct: if (rem == y) r = in[state[(size_t)x * kMcsLanes + y]]; break;
    case kMcsProdSum: if (rem < y) r = in[state[(size_t)x * kMcsLanes + rem]]; break;
    default: r = in[state[(size_t)(x + 1) * kMcsLanes + y]]; break;
    }
    a.values[(size_t)match * a.num_vars + v] = r;
#endif
}

__global__ __launch_bounds__(kCsBlock) void mcs_divrem_kernel(const Fp* __restrict__ values, uint32_t m, uint32_t count, Fp* __restrict__ quot,
                                                              uint32_t* __restrict__ rem) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kCsBlock + threadIdx.x;
    if (i >= count) return;
    Fp q;
    rem[i] = mcs_divrem(values[i], m, &q);
    quot[i] = q;
#endif
}

int mcs_witness_run(Ctx& c, const McsWitnessArgs& a, uint32_t batch) {
    const dim3 block(kCsBlock);
    UZK_LAUNCH(c, "mcs_steps", mcs_steps_kernel, dim3(batch), dim3(kMcsLanes), 0, c.stream, a);
    UZK_LAUNCH(c, "mcs_values", mcs_values_kernel, dim3(cs_grid(a.num_vars), batch), block, 0, c.stream, a);
    UZK_TRY(cs_gather_run(c, {a.n, a.num_vars, a.pi_count, a.wiring, a.pi_vars, a.values, a.witness, a.pi}, batch));
    return UZK_OK;
}

int mcs_divrem_run(Ctx& c, const Fp* d_values, uint32_t m, uint32_t count, Fp* d_quot, uint32_t* d_rem) {
    UZK_LAUNCH(c, "mcs_divrem", mcs_divrem_kernel, dim3(cs_grid(count)), dim3(kCsBlock), 0, c.stream, d_values, m, count, d_quot, d_rem);
    return UZK_OK;
}

}  // namespace uzk
