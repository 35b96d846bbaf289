// uzkge_amd/csrc/handles.hpp on the CPU: the handle table and the workspace carver have no HIP in them, so plain g++ builds this
// program (tests/test_handles_host.py: once plain, once under ThreadSanitizer, once under Address- and UBSanitizer).
//   handles_host            every check below; prints OK and exits 0, or says which check failed and exits 1
#include <cstdint>
#include <cstdio>
#include <set>
#include <thread>
#include <vector>

#include "../../uzkge_amd/csrc/handles.hpp"

using uzk::HandleTable;
using uzk::WsArray;
using uzk::WsCarver;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

struct Entry {
    int device = 0;
    uint64_t payload = 0;
};

static void test_handles_count_up_from_one() {
    const uint64_t tag = 5ull << 59;
    HandleTable<Entry> t(tag);
    for (uint64_t k = 1; k <= 5; ++k) CHECK(t.insert(Entry{0, k}) == (tag | k));
    Entry e;
    CHECK(t.get(tag | 3, &e) && e.payload == 3);
    CHECK(!t.get(tag | 6, &e) && !t.get(tag, &e) && !t.get(3, &e));
}

static void test_tables_refuse_each_others_handles() {
    HandleTable<Entry> a(1ull << 59), b(1ull << 58), c(7ull << 59);
    HandleTable<Entry>* all[] = {&a, &b, &c};
    uint64_t h[3];
    for (int i = 0; i < 3; ++i) h[i] = all[i]->insert(Entry{i, 100u + i});   // the counter part is 1 in all three
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Entry e;
            if (i == j) continue;
            CHECK(!all[i]->get(h[j], &e));
            CHECK(!all[i]->take(h[j], &e));
        }
    for (int i = 0; i < 3; ++i) {                                             // and every handle is still alive in its own table
        Entry e;
        CHECK(all[i]->get(h[i], &e) && e.device == i && e.payload == 100u + i);
    }
}

static void test_take_removes_once() {
    HandleTable<Entry> t(6ull << 59);
    const uint64_t h1 = t.insert(Entry{0, 11}), h2 = t.insert(Entry{1, 22});
    Entry e;
    CHECK(t.take(h1, &e) && e.payload == 11);
    CHECK(!t.get(h1, &e));
    CHECK(!t.take(h1, &e));
    CHECK(t.get(h2, &e) && e.device == 1 && e.payload == 22);
}

static void test_drain_frees_each_live_entry_once_and_the_count_goes_on() {
    const uint64_t tag = 1ull << 58;
    HandleTable<Entry> t(tag);
    uint64_t h[4];
    for (int k = 0; k < 4; ++k) h[k] = t.insert(Entry{0, (uint64_t)k});
    Entry e;
    CHECK(t.take(h[1], &e));
    std::multiset<uint64_t> freed;
    t.drain([&](const Entry& x) { freed.insert(x.payload); });
    CHECK(freed == (std::multiset<uint64_t>{0, 2, 3}));
    for (int k = 0; k < 4; ++k) CHECK(!t.get(h[k], &e));
    int again = 0;
    t.drain([&](const Entry&) { ++again; });
    CHECK(again == 0);
    CHECK(t.insert(Entry{}) == (tag | 5));
    CHECK(t.insert(Entry{}) == (tag | 6));
}

static void test_threads() {
    constexpr int kThreads = 8, kEach = 1000;
    const uint64_t tag = 7ull << 59;
    HandleTable<Entry> t(tag);
    std::vector<std::vector<uint64_t>> seen(kThreads);
    std::vector<uint64_t> freed(kThreads, 0), bad(kThreads, 0);
    std::vector<std::thread> th;
    for (int i = 0; i < kThreads; ++i)
        th.emplace_back([&, i] {
            for (int k = 0; k < kEach; ++k) {
                const uint64_t payload = (uint64_t)i * kEach + k;
                const uint64_t h = t.insert(Entry{i, payload});
                seen[i].push_back(h);
                Entry e;
                if (!t.get(h, &e) || e.payload != payload) ++bad[i];
                if (t.take(h, &e) && e.device == i && e.payload == payload) ++freed[i];   // "freeing" happens outside the table's lock
                else ++bad[i];
                if (t.take(h, &e)) ++bad[i];
            }
        });
    for (auto& x : th) x.join();
    std::set<uint64_t> unique;
    uint64_t total_freed = 0;
    for (int i = 0; i < kThreads; ++i) {
        CHECK(bad[i] == 0);
        total_freed += freed[i];
        for (uint64_t h : seen[i]) {
            CHECK((h & tag) == tag && (h ^ tag) >= 1 && (h ^ tag) <= (uint64_t)kThreads * kEach);
            unique.insert(h);
        }
    }
    CHECK(unique.size() == (size_t)kThreads * kEach);
    CHECK(total_freed == (uint64_t)kThreads * kEach);
    int left = 0;
    t.drain([&](const Entry&) { ++left; });
    CHECK(left == 0);
    CHECK(t.insert(Entry{}) == (tag | ((uint64_t)kThreads * kEach + 1)));
}

// what a DevBuf is to the carver: reserve(bytes) and p
struct FakeBuf {
    void* p = nullptr;
    size_t asked = 0;
    int calls = 0, fail = 0;
    alignas(256) static char block[1 << 16];
    int reserve(size_t bytes) {
        ++calls;
        asked = bytes;
        if (fail) return fail;
        p = block;
        return 0;
    }
};
alignas(256) char FakeBuf::block[1 << 16];

struct Rec24 {
    uint32_t w[6];
};
static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

static void test_carver_byte_sizes() {
    // arrays of 0, 1, 255, 256 and 257 bytes, a zero-length one in the middle and at the end
    const size_t sizes[] = {0, 1, 255, 0, 256, 257, 0};
    constexpr int N = sizeof sizes / sizeof sizes[0];
    WsCarver cv;
    WsArray<uint8_t> a[N];
    size_t want = 0;
    for (int i = 0; i < N; ++i) {
        a[i] = cv.array<uint8_t>(sizes[i]);
        CHECK(a[i].offset == want && a[i].count == sizes[i] && a[i].bytes() == sizes[i]);
        want += up256(sizes[i]);
        CHECK(cv.total() == want);
    }
    CHECK(want == 0 + 256 + 256 + 0 + 256 + 512 + 0);
    CHECK(a[0].offset == a[1].offset && a[3].offset == a[4].offset && a[6].offset == cv.total());   // no elements, no room
    FakeBuf buf;
    CHECK(cv.reserve(buf) == 0 && buf.calls == 1 && buf.asked == want);
    for (int i = 0; i < N; ++i) CHECK(cv(a[i]) == reinterpret_cast<uint8_t*>(FakeBuf::block + a[i].offset));
}

static void test_carver_mixed_types() {
    WsCarver cv;
    const auto a = cv.array<uint8_t>(300);      // 300 bytes -> 512
    const auto b = cv.array<uint64_t>(33);      // 264 bytes -> 512
    const auto c = cv.array<Rec24>(0);          // nothing
    const auto d = cv.array<Rec24>(32);         // 768 bytes -> 768
    const auto e = cv.array<uint32_t>(1);       // 4 bytes -> 256
    const auto f = cv.array<Rec24>(11);         // 264 bytes -> 512
    CHECK(a.offset == 0 && b.offset == 512 && c.offset == 1024 && d.offset == 1024 && e.offset == 1792 && f.offset == 2048);
    CHECK(cv.total() == 2560);
    CHECK(b.bytes() == 264 && d.bytes() == 768 && f.bytes() == 264);
    FakeBuf buf;
    CHECK(cv.reserve(buf) == 0 && buf.asked == 2560);
    char* base = FakeBuf::block;
    uint64_t* pb = cv(b);
    Rec24 *pc = cv(c), *pd = cv(d), *pf = cv(f);
    uint32_t* pe = cv(e);
    CHECK(reinterpret_cast<char*>(cv(a)) == base && reinterpret_cast<char*>(pb) == base + 512 && reinterpret_cast<char*>(pc) == base + 1024 &&
          reinterpret_cast<char*>(pd) == base + 1024 && reinterpret_cast<char*>(pe) == base + 1792 && reinterpret_cast<char*>(pf) == base + 2048);
    pb[32] = 7; pd[31].w[5] = 9; pe[0] = 1; pf[10].w[5] = 3;                   // the last element of each array lies inside its room
    CHECK(reinterpret_cast<char*>(&pb[33]) <= base + 1024 && reinterpret_cast<char*>(&pd[32]) <= base + 1792 && reinterpret_cast<char*>(&pf[11]) <= base + 2560);
    // a reserve that fails is the caller's error code, passed through
    WsCarver cv2;
    (void)cv2.array<uint32_t>(5);
    FakeBuf bad;
    bad.fail = 3;
    CHECK(cv2.reserve(bad) == 3);
}

static void test_carver_bound_to_a_block_of_its_total() {
    WsCarver cv;
    const auto a = cv.array<uint32_t>(65);      // 260 bytes -> 512
    const auto b = cv.array<uint16_t>(0);       // nothing
    const auto c = cv.array<uint8_t>(7);        // 7 bytes -> 256
    CHECK(cv.total() == 768);
    std::vector<char> block(cv.total());        // exactly the total: the sanitizers see a write past any array's room
    cv.bind(block.data());
    CHECK(reinterpret_cast<char*>(cv(a)) == block.data() && reinterpret_cast<char*>(cv(b)) == block.data() + 512 &&
          reinterpret_cast<char*>(cv(c)) == block.data() + 512);
    cv(a)[64] = 5; cv(c)[6] = 9;
    CHECK(reinterpret_cast<char*>(&cv(c)[7]) <= block.data() + cv.total());
    // a later reserve moves the carver to the buffer, as for any other carver
    FakeBuf buf;
    CHECK(cv.reserve(buf) == 0 && buf.asked == 768 && reinterpret_cast<char*>(cv(a)) == FakeBuf::block);
}

int main() {
    test_handles_count_up_from_one();
    test_tables_refuse_each_others_handles();
    test_take_removes_once();
    test_drain_frees_each_live_entry_once_and_the_count_goes_on();
    test_threads();
    test_carver_byte_sizes();
    test_carver_mixed_types();
    test_carver_bound_to_a_block_of_its_total();
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("OK\n");
    return 0;
}
