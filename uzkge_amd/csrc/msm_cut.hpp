// How a bucket's run of sorted points is cut into accumulation tasks (msm.hip) -- the ONE place that says so: the device's task
// scan and task fill, the last fold level and the host's workspace bounds all call these functions
// (tests/cpp/msm_cut_host.cpp checks them against each other on the CPU).
//
// A bucket of population p becomes T = ceil(p / L_b) tasks of equal length (r of q + 1 points, T - r of q).  L_b is the plan's
// task length L for most buckets.  With the taper on, the first buckets of every scan window get a shorter cut: the schedule is
// longest first, so their tasks are the grid's end, and the accumulator's drain -- the time its resident waves take to finish
// once the task list is empty -- lasts one SHORT task instead of one of L / 2 additions.  Only buckets of ordinary population
// (p <= kCutSpan * L) are cut short: a bucket that a skewed scalar set fills with thousands of points keeps the length L, its
// task count what it was, and the workspace bounds stay close to the untapered ones whatever the scalars are.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UZK_CUT_HD __host__ __device__
#else
#define UZK_CUT_HD
#endif

namespace uzk {

constexpr uint32_t kCutSpan = 2;                 // short cuts only for populations <= kCutSpan * L
constexpr uint32_t kCutMaxTasks = kCutSpan * 8;  // so a short-cut bucket never has more tasks than this
// lanes the accumulator keeps resident: 256 CUs x 4 SIMDs x 4 waves (its launch bound) x 64
constexpr uint64_t kResidentLanes = 256ull * 4 * 4 * 64;

struct MsmCut {
    uint32_t L = 0;      // task length of an ordinary bucket (16 .. 256)
    uint32_t NB = 0;     // buckets per scan window
    uint32_t n8 = 0;     // the first n8 buckets of every scan window are cut at ceil(L / 8) ...
    uint32_t n4 = 0;     // ... and the n4 behind them at ceil(L / 4)   (both 0: no taper, every bucket at L)
};

// cut length of bucket b (index inside its scan window w)
UZK_CUT_HD inline uint32_t msm_cut_len(const MsmCut& p, uint32_t w, uint32_t b) {
    (void)w;                                      // every scan window tapers alike
    if (b < p.n8) return (p.L + 7) >> 3;          // rounded up: at most 8 (4) pieces per L points, whatever L is
    if (b - p.n8 < p.n4) return (p.L + 3) >> 2;
    return p.L;
}
// is bucket b, holding pop points, cut short?
UZK_CUT_HD inline bool msm_cut_short(const MsmCut& p, uint32_t w, uint32_t b, uint32_t pop) {
    (void)w;
    return b < p.n8 + p.n4 && pop <= kCutSpan * p.L;
}
// number of tasks of bucket b holding pop points
UZK_CUT_HD inline uint32_t msm_task_count(const MsmCut& p, uint32_t w, uint32_t b, uint32_t pop) {
    if (pop == 0) return 0;
    const uint32_t Lb = msm_cut_short(p, w, b, pop) ? msm_cut_len(p, w, b) : p.L;
    return (pop + Lb - 1) / Lb;
}
// the most tasks -- partial sums -- bucket b can have when it is cut short (<= kCutMaxTasks): the task fill writes that many
// descriptors per lane, the last fold level folds that many per lane, where other buckets with as many go to a wave of their own
UZK_CUT_HD inline uint32_t msm_cut_max_tasks(const MsmCut& p, uint32_t w, uint32_t b) {
    const uint32_t Lb = msm_cut_len(p, w, b);
    return (kCutSpan * p.L + Lb - 1) / Lb;
}
// The order in which the last fold level takes the buckets: position idx of its grid -> bucket w * NB + b.  The short-cut buckets
// of ALL windows come first, the shortest cuts (most partial sums) before the others: their lanes fold a chain of up to
// msm_cut_max_tasks sums, and started where their window's turn comes that chain is the kernel's tail (0.33 instead of 0.20 ms
// at n = 2^24).  A permutation of [0, Wd * NB); the identity without a taper.
UZK_CUT_HD inline uint64_t msm_cut_order(const MsmCut& p, uint32_t Wd, uint64_t idx) {
    if (p.n8 == 0) return idx;
    const uint32_t ns = p.n8 + p.n4, rest = p.NB - ns;
    uint32_t w, b;
    if (idx < (uint64_t)Wd * p.n8) { w = (uint32_t)(idx / p.n8); b = (uint32_t)(idx % p.n8); }
    else if (idx < (uint64_t)Wd * ns) { const uint64_t i = idx - (uint64_t)Wd * p.n8; w = (uint32_t)(i / p.n4); b = p.n8 + (uint32_t)(i % p.n4); }
    else { const uint64_t i = idx - (uint64_t)Wd * ns; w = (uint32_t)(i / rest); b = ns + (uint32_t)(i % rest); }
    return (uint64_t)w * p.NB + b;
}
// Upper bound on the tasks of Wd scan windows holding `entries` points in all, for ANY populations: a short-cut bucket has at
// most kCutSpan * L / L_b tasks, every other one ceil(p / L), and sum ceil(p_b / L) <= floor(sum p_b / L) + #buckets.
inline uint64_t msm_task_bound(const MsmCut& p, uint64_t Wd, uint64_t entries) {
    return entries / p.L + Wd * p.NB + Wd * ((uint64_t)kCutSpan * 8 * p.n8 + (uint64_t)kCutSpan * 4 * p.n4);
}
// The plan's taper.  mode 0: none.  1: only where the task list is several times the resident lanes (each short length then
// gets about one task per resident lane: at n = 2^24, c = 17 the 1/32 of the buckets cut at L / 8 = 32 give 28 x 1024 x 8.5 =
// 244 k tasks, the 1/16 cut at 64 give 28 x 2048 x 4.5 = 258 k, and the two-task buckets supply the 128s by themselves; the
// top window's buckets hold 680 points each, more than kCutSpan * L, and stay as they are).  2: at any size (tests).
inline MsmCut msm_cut_plan(uint32_t L, uint32_t NB, uint64_t entries, int mode) {
    MsmCut p;
    p.L = L; p.NB = NB;
    const bool on = mode >= 2 ? NB >= 4 : (mode == 1 && NB >= 1024 && entries / L >= 3 * kResidentLanes);
    if (on) {
        p.n8 = NB / 32 ? NB / 32 : 1;
        p.n4 = 2 * p.n8;
    }
    return p;
}

}  // namespace uzk
