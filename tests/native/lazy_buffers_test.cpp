// csrc/lazy_buffers.hpp on the CPU: a set of lazily made buffers is all or nothing.  A counting allocator fails each
// allocation index in turn; afterwards every pointer is null, the capacity 0, nothing is live, and the next call starts
// over.  Stand-alone; built with AddressSanitizer + UBSan (a leak or a double free ends the run).
#include "../../vectorlite_amd/csrc/lazy_buffers.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>

namespace {
int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++failures;                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
        }                                                   \
    } while (0)

constexpr int OOM = 7;

struct FakeMem {
    int allocs = 0, releases = 0;
    int fail_at = -1;                // the allocation (counted from 0 since the last arm()) that fails
    int since_arm = 0;
    std::map<void*, bool> live;      // pointer -> pinned
    void arm(int index)
    {
        fail_at = index;
        since_arm = 0;
    }
    int alloc(void** p, size_t bytes, bool pinned)
    {
        if (since_arm++ == fail_at) {
            *p = reinterpret_cast<void*>(0x1);  // garbage the helper must not keep
            return OOM;
        }
        ++allocs;
        *p = std::malloc(bytes ? bytes : 1);
        live[*p] = pinned;
        return 0;
    }
    void release(void* p, bool pinned)
    {
        auto it = live.find(p);
        EXPECT(it != live.end(), "released a pointer that is not live");
        if (it == live.end()) return;
        EXPECT(it->second == pinned, "released as the other kind of memory");
        live.erase(it);
        std::free(p);
        ++releases;
    }
};

struct Four {  // a fixed set of mixed types and kinds
    uint32_t* ctr = nullptr;
    uint32_t* h_ctr = nullptr;
    double* h_scores = nullptr;
    uint64_t* keys = nullptr;
    bool all_null() const { return !ctr && !h_ctr && !h_scores && !keys; }
    bool all_set() const { return ctr && h_ctr && h_scores && keys; }
};
int ensure_four(FakeMem& mem, Four& b)
{
    return vl::ensure_set(mem, {vl::dev_buf(b.ctr, 4), vl::pinned_buf(b.h_ctr, 4), vl::pinned_buf(b.h_scores, 64), vl::dev_buf(b.keys, 64)});
}

struct Pair {
    uint64_t* keys = nullptr;
    uint32_t* pos = nullptr;
    size_t cap = 0;
};
int grow_pair(FakeMem& mem, Pair& b, size_t need)
{
    return vl::grow(mem, b.cap, need, {vl::dev_buf(b.keys, need), vl::dev_buf(b.pos, need)});
}

void fixed_set()
{
    for (int fail = 0; fail < 4; ++fail) {
        FakeMem mem;
        Four b;
        mem.arm(fail);
        EXPECT(ensure_four(mem, b) == OOM, "set: allocation %d failing is reported", fail);
        EXPECT(b.all_null(), "set: every pointer is null after allocation %d failed", fail);
        EXPECT(mem.live.empty() && mem.allocs == fail && mem.releases == fail, "set: what was obtained before %d went back", fail);
        mem.arm(-1);
        EXPECT(ensure_four(mem, b) == 0 && b.all_set(), "set: the retry after %d succeeds", fail);
        EXPECT(mem.live.size() == 4 && mem.allocs == fail + 4, "set: the retry made all four");
        EXPECT(mem.live.at(b.ctr) == false && mem.live.at(b.h_ctr) == true && mem.live.at(b.h_scores) == true &&
                   mem.live.at(b.keys) == false, "set: each member came from its kind of memory");
        b.h_scores[63] = 1.0;  // the sizes are the elements asked for (ASan)
        b.keys[63] = 1;
        const Four before = b;
        EXPECT(ensure_four(mem, b) == 0 && mem.allocs == fail + 4 && mem.releases == fail, "set: a second call allocates nothing");
        EXPECT(b.ctr == before.ctr && b.keys == before.keys, "set: a second call keeps the buffers");
        for (auto& e : std::map<void*, bool>(mem.live)) mem.release(e.first, e.second);
    }
}

void empty_flag_member()
{
    FakeMem mem;
    Four b;
    const int rc = vl::ensure_set(mem, {vl::dev_buf(b.ctr, 0), vl::pinned_buf(b.h_ctr, 4)});
    EXPECT(rc == vl::LAZY_BAD_SET && mem.allocs == 0 && b.all_null(), "set: an empty first member cannot be the flag: refused, nothing made");
}

void grown_pair()
{
    for (int fail = 0; fail < 2; ++fail) {
        FakeMem mem;
        Pair b;
        EXPECT(grow_pair(mem, b, 0) == 0 && mem.allocs == 0 && !b.keys && b.cap == 0, "pair: nothing is needed, nothing is made");
        mem.arm(fail);
        EXPECT(grow_pair(mem, b, 100) == OOM, "pair: allocation %d failing is reported", fail);
        EXPECT(!b.keys && !b.pos && b.cap == 0, "pair: null pointers and no capacity after allocation %d failed", fail);
        EXPECT(mem.live.empty() && mem.releases == fail, "pair: what was obtained before %d went back", fail);
        mem.arm(-1);
        EXPECT(grow_pair(mem, b, 100) == 0 && b.keys && b.pos && b.cap == 100, "pair: the retry after %d succeeds", fail);
        b.keys[99] = 1;
        b.pos[99] = 1;
        const int allocs = mem.allocs, releases = mem.releases;
        EXPECT(grow_pair(mem, b, 100) == 0 && grow_pair(mem, b, 7) == 0 && mem.allocs == allocs && mem.releases == releases,
               "pair: the same need, or a smaller one, allocates nothing");
        EXPECT(grow_pair(mem, b, 101) == 0 && b.cap == 101, "pair: a larger need is served");
        // (release() fails the run on a pointer that is not live: two releases are the two old buffers, once each)
        EXPECT(mem.releases == releases + 2 && mem.allocs == allocs + 2, "pair: the old buffers went exactly once");
        EXPECT(mem.live.size() == 2 && mem.live.count(b.keys) && mem.live.count(b.pos), "pair: the two new buffers are what is live");
        b.keys[100] = 1;
        // growth that fails while buffers are held: they are gone too, and the next call starts over
        mem.arm(fail);
        EXPECT(grow_pair(mem, b, 1000) == OOM && !b.keys && !b.pos && b.cap == 0 && mem.live.empty(),
               "pair: failed growth (allocation %d) leaves an empty pair", fail);
        mem.arm(-1);
        EXPECT(grow_pair(mem, b, 5) == 0 && b.cap == 5 && mem.live.size() == 2, "pair: ... from which a small need is served");
        mem.release(b.keys, false);
        mem.release(b.pos, false);
    }
}
}  // namespace

int main()
{
    fixed_set();
    empty_flag_member();
    grown_pair();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("lazy buffers ok\n");
    return 0;
}
