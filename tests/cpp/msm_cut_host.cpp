// The MSM's bucket-cutting rule (uzkge_amd/csrc/msm_cut.hpp) on the CPU: the header is plain C++ outside a HIP compile, so g++
// builds this program by itself (tests/test_msm_cut_host.py).  For plans with the taper off, automatic and forced, and for random
// and extreme populations, it checks that
//   - the pieces of every bucket (r of q + 1 points, T - r of q, as msm_bucket_fill_kernel cuts them) add up to its population;
//   - no piece is longer than the bucket's cut length, none longer than L <= 256, and its bin of the schedule's length
//     histogram (min(len, kLenBins - 1)) is inside the histogram;
//   - a short-cut bucket never has more tasks than msm_cut_max_tasks says (the last fold level relies on it);
//   - the tasks of all buckets together never exceed msm_task_bound, the host's reservation, and without a taper that bound is
//     the old entries / L + buckets;
//   - with the taper off every bucket has ceil(p / L) tasks: the schedule of before;
//   - the order in which the last fold level takes the buckets (msm_cut_order) is a permutation that puts every bucket with a
//     short cut before every other one, the shortest cuts first, and is the identity without a taper.
// Prints OK and exits 0, or says which check failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../uzkge_amd/csrc/msm_cut.hpp"

using namespace uzk;

static constexpr uint32_t kLenBins = 256;   // msm.hip

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

// one bucket: returns its task count after checking its pieces
static uint64_t check_bucket(const MsmCut& p, uint32_t w, uint32_t b, uint32_t pop) {
    const uint32_t T = msm_task_count(p, w, b, pop);
    if (pop == 0) { CHECK(T == 0, "empty bucket with %u tasks", T); return 0; }
    CHECK(T >= 1, "pop %u without a task", pop);
    const uint32_t Lb = msm_cut_len(p, w, b);
    CHECK(Lb == p.L || Lb == (p.L + 1) / 2 || Lb == (p.L + 3) / 4 || Lb == (p.L + 7) / 8, "cut length %u of L %u", Lb, p.L);
    CHECK(Lb >= 1, "cut length 0");
    const uint32_t q = pop / T, r = pop - q * T;
    uint64_t sum = 0;
    uint32_t longest = 0;
    for (uint32_t j = 0; j < T && j < 4096; ++j) {         // (every piece of a small bucket; the two lengths of a huge one below)
        const uint32_t len = q + (j < r ? 1u : 0u);
        sum += len;
        longest = len > longest ? len : longest;
    }
    if (T > 4096) { sum = (uint64_t)r * (q + 1) + (uint64_t)(T - r) * q; longest = q + (r ? 1u : 0u); }
    CHECK(sum == pop, "pieces add up to %llu, population %u", (unsigned long long)sum, pop);
    CHECK(longest <= p.L && p.L <= 256, "piece of %u, L %u", longest, p.L);
    CHECK((longest < kLenBins - 1 ? longest : kLenBins - 1) < kLenBins, "histogram bin");
    CHECK(msm_cut_short(p, w, b, pop) == (Lb != p.L && pop <= kCutSpan * p.L), "msm_cut_short");
    if (pop <= kCutSpan * p.L) {
        CHECK(longest <= Lb, "piece of %u in a bucket cut at %u", longest, Lb);
        CHECK(T <= msm_cut_max_tasks(p, w, b) && msm_cut_max_tasks(p, w, b) <= (Lb == p.L ? kCutSpan : kCutMaxTasks), "%u tasks, at most %u promised",
              T, msm_cut_max_tasks(p, w, b));
    } else {
        CHECK(T == (pop + p.L - 1) / p.L, "a large bucket is cut at L");
    }
    if (p.n8 == 0) CHECK(T == (pop + p.L - 1) / p.L, "taper off: ceil(p / L)");
    return T;
}

static void check_plan(const MsmCut& p, uint32_t Wd, std::mt19937_64& rng) {
    CHECK(p.n8 + p.n4 <= p.NB, "tapered %u + %u of %u buckets", p.n8, p.n4, p.NB);
    const uint64_t nbk = (uint64_t)Wd * p.NB;
    {   // the last fold level's order
        std::vector<uint8_t> seen(nbk, 0);
        uint32_t prev_len = 0;
        for (uint64_t idx = 0; idx < nbk; ++idx) {
            const uint64_t t = msm_cut_order(p, Wd, idx);
            CHECK(t < nbk && !seen[t], "order: position %llu -> bucket %llu", (unsigned long long)idx, (unsigned long long)t);
            seen[t] = 1;
            if (p.n8 == 0) CHECK(t == idx, "order without a taper");
            const uint32_t len = msm_cut_len(p, (uint32_t)(t / p.NB), (uint32_t)(t % p.NB));
            CHECK(len >= prev_len, "order: a cut of %u behind one of %u", len, prev_len);
            prev_len = len;
        }
    }
    std::vector<uint32_t> pop(nbk);
    auto run = [&](const char* what) {
        uint64_t entries = 0, tasks = 0;
        for (uint64_t t = 0; t < nbk; ++t) {
            entries += pop[t];
            tasks += check_bucket(p, (uint32_t)(t / p.NB), (uint32_t)(t % p.NB), pop[t]);
        }
        const uint64_t bound = msm_task_bound(p, Wd, entries);
        CHECK(tasks <= bound, "%s: %llu tasks, bound %llu (L %u NB %u n8 %u)", what, (unsigned long long)tasks,
              (unsigned long long)bound, p.L, p.NB, p.n8);
        if (p.n8 == 0) CHECK(bound == entries / p.L + nbk, "%s: the untapered bound changed", what);
    };
    const uint32_t L = p.L;
    const uint32_t edge[] = {0, 1, 2, L / 8 - 1, L / 8, L / 8 + 1, L / 4, L / 4 + 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1,
                             3 * L, 255, 256, 257, 8 * L + 1};
    // every bucket at the population that costs its cut the most tasks per point
    for (uint64_t t = 0; t < nbk; ++t) pop[t] = 1;
    run("all ones");
    for (uint64_t t = 0; t < nbk; ++t) pop[t] = msm_cut_len(p, 0, (uint32_t)(t % p.NB)) + 1;
    run("cut + 1");
    for (uint64_t t = 0; t < nbk; ++t) pop[t] = kCutSpan * L;
    run("span");
    for (uint64_t t = 0; t < nbk; ++t) pop[t] = kCutSpan * L + 1;
    run("span + 1");
    for (uint32_t e : edge) { for (uint64_t t = 0; t < nbk; ++t) pop[t] = e; run("edge"); }
    // everything in one bucket: the first (a short-cut one), the last, and the last short-cut one
    for (uint64_t at : {(uint64_t)0, nbk - 1, (uint64_t)(p.n8 + p.n4 ? p.n8 + p.n4 - 1 : 0)}) {
        for (uint64_t t = 0; t < nbk; ++t) pop[t] = 0;
        pop[at] = 0x7FFFFFFFu;
        run("one bucket");
        pop[at] = 1;
        run("one point");
    }
    for (uint64_t t = 0; t < nbk; ++t) pop[t] = 0;
    run("empty");
    // random: around the mean a plan of this L is made for, edges mixed in, a few heavy buckets
    for (int rep = 0; rep < 4; ++rep) {
        std::poisson_distribution<uint32_t> around(rep & 1 ? L : L / 4.0 + 1);
        for (uint64_t t = 0; t < nbk; ++t) {
            const uint64_t x = rng();
            pop[t] = (x & 15) == 0 ? edge[(x >> 8) % (sizeof(edge) / sizeof(edge[0]))] : ((x & 1023) == 1 ? (uint32_t)((x >> 20) % 100000) : around(rng));
        }
        run("random");
    }
}

int main() {
    std::mt19937_64 rng(20240611);
    int plans = 0, tapered = 0;
    for (uint32_t L : {16u, 24u, 64u, 100u, 200u, 256u})
        for (uint32_t NB : {1u, 2u, 4u, 8u, 32u, 128u, 1024u, 4096u, 32768u})
            for (int mode = 0; mode <= 2; ++mode)
                for (uint64_t entries : {(uint64_t)1 << 16, (uint64_t)15 << 24}) {
                    const MsmCut p = msm_cut_plan(L, NB, entries, mode);
                    CHECK(p.L == L && p.NB == NB, "plan fields");
                    if (mode == 0) CHECK(p.n8 == 0 && p.n4 == 0, "mode 0 tapers");
                    if (mode == 2 && NB >= 4) CHECK(p.n8 != 0, "mode 2 does not taper at NB %u", NB);
                    if (mode == 1 && entries == ((uint64_t)1 << 16)) CHECK(p.n8 == 0, "mode 1 tapers a small problem");
                    check_plan(p, NB >= 32768 ? 2 : 3, rng);
                    ++plans;
                    tapered += p.n8 != 0;
                }
    // the flagship plan: n = 2^24, c = 17 -- 15 windows of 2^16 buckets = 30 scan windows of 2^15, L = 256
    const MsmCut big = msm_cut_plan(256, 1u << 15, (uint64_t)15 << 24, 1);
    CHECK(big.n8 == 1024 && big.n4 == 2048, "the 2^24 plan tapers %u + %u buckets per scan window", big.n8, big.n4);
    CHECK(msm_cut_plan(256, 1u << 15, (uint64_t)13 << 20, 1).n8 == 0, "a 2^20 plan tapers");
    CHECK(tapered > 0 && tapered < plans, "plans with and without a taper");
    std::printf("%d plans (%d tapered)\nOK\n", plans, tapered);
    return 0;
}
