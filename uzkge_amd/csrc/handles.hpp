// The two pieces of host scaffolding every key-holding module shares: the process-wide table behind one kind of handle, and the
// carving of a grow-only block into the arrays of one call.  Plain C++17, no HIP in it: tests/cpp/handles_host.cpp builds it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>

namespace uzk {

// One kind of handle: handles are tag | 1, tag | 2, ... for the life of the process (a released handle is never issued again), so
// a handle of another kind, or a stale one, is simply unknown.  Entries are small descriptors copied in and out under the lock; the
// device memory they name is freed by the caller, outside the lock (take) or under it (drain: the process is shutting down).
template <class Entry>
class HandleTable {
  public:
    explicit HandleTable(uint64_t tag) : tag_(tag) {}
    HandleTable(const HandleTable&) = delete;
    HandleTable& operator=(const HandleTable&) = delete;

    uint64_t insert(const Entry& e) {
        std::lock_guard<std::mutex> lk(mu_);
        const uint64_t h = tag_ | next_++;
        map_[h] = e;
        return h;
    }
    bool get(uint64_t h, Entry* out) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = map_.find(h);
        if (it == map_.end()) return false;
        *out = it->second;
        return true;
    }
    // removes the entry and hands it to the caller, who frees what it names
    bool take(uint64_t h, Entry* out) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = map_.find(h);
        if (it == map_.end()) return false;
        *out = it->second;
        map_.erase(it);
        return true;
    }
    // free_fn(entry) for every live entry, then none is left; the count goes on
    template <class F>
    void drain(F&& free_fn) {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& kv : map_) free_fn(kv.second);
        map_.clear();
    }

  private:
    const uint64_t tag_;
    std::mutex mu_;
    std::map<uint64_t, Entry> map_;
    uint64_t next_ = 1;
};

// An array of a carved block: declared once, with its element type and count.
template <class T>
struct WsArray {
    size_t offset, count;
    size_t bytes() const { return count * sizeof(T); }
};

// Arrays laid one behind the other in one block, each at a multiple of kWsAlign; an array of no elements takes no room.
//     WsCarver cv;
//     const auto a = cv.array<Fp>(n), b = cv.array<uint8_t>(m);
//     UZK_TRY(cv.reserve(c.some_ws));         // one reserve of cv.total() bytes
//     Fp* d_a = cv(a);
constexpr size_t kWsAlign = 256;
class WsCarver {
  public:
    template <class T>
    WsArray<T> array(size_t count) {
        const WsArray<T> a{at_, count};
        at_ += (a.bytes() + kWsAlign - 1) & ~(kWsAlign - 1);
        return a;
    }
    size_t total() const { return at_; }
    // Buf: DevBuf (ctx.hpp) -- reserve(bytes) returns 0 or an error code, p is the block
    template <class Buf>
    int reserve(Buf& buf) {
        const int rc = buf.reserve(at_);
        if (rc == 0) base_ = static_cast<char*>(buf.p);
        return rc;
    }
    // a block of the caller's own, of exactly total() bytes, in place of a buffer that grows
    void bind(void* block) { base_ = static_cast<char*>(block); }
    template <class T>
    T* operator()(const WsArray<T>& a) const { return reinterpret_cast<T*>(base_ + a.offset); }

  private:
    size_t at_ = 0;
    char* base_ = nullptr;
};

}  // namespace uzk
