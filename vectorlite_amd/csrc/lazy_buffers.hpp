// lazy_buffers.hpp -- scratch buffers made on first use or regrown on demand, all or nothing.
//
// A lazily made set of buffers is safe only if a failed allocation leaves it looking untouched: every pointer null, the
// capacity 0, nothing leaked.  The next call then starts over, instead of finding a "made" flag beside null pointers.
// Both helpers below keep that promise.  They know nothing about the memory they hand out; `mem` is any object with
//     int  alloc(void** p, size_t bytes, bool pinned)    0 on success, else the status the helper returns
//     void release(void* p, bool pinned)
// flat_index.cpp passes device and pinned-host allocation, tests/native/lazy_buffers_test.cpp a counting fake.
#pragma once

#include <cstddef>
#include <initializer_list>

namespace vl {

struct BufReq {  // one buffer of a set: where its pointer is kept, its size, device memory or pinned host memory
    void** slot;
    size_t bytes;
    bool pinned;
};
template <typename T>
BufReq dev_buf(T*& p, size_t count)
{
    return {reinterpret_cast<void**>(&p), count * sizeof(T), false};
}
template <typename T>
BufReq pinned_buf(T*& p, size_t count)
{
    return {reinterpret_cast<void**>(&p), count * sizeof(T), true};
}

namespace lazy_detail {
template <typename Mem>
void drop(Mem& mem, std::initializer_list<BufReq> set)
{
    for (const BufReq& r : set) {
        if (*r.slot) mem.release(*r.slot, r.pinned);
        *r.slot = nullptr;
    }
}
template <typename Mem>
int obtain(Mem& mem, std::initializer_list<BufReq> set)  // every slot is null on entry
{
    for (const BufReq& r : set) {
        const int rc = mem.alloc(r.slot, r.bytes, r.pinned);
        if (rc != 0) {
            *r.slot = nullptr;
            drop(mem, set);  // what was obtained so far; the slots behind the failed one are still null
            return rc;
        }
    }
    return 0;
}
}  // namespace lazy_detail

// A fixed set made on first use.  Its first member doubles as the "already made" flag, which is sound because the set is
// all or nothing -- and because that member is never empty: a 0-byte allocation may stay null, the set would be made
// again on every call and its other members leaked.  Such a set is refused.
constexpr int LAZY_BAD_SET = 8;  // (the library's invalid-argument status)
template <typename Mem>
int ensure_set(Mem&& mem, std::initializer_list<BufReq> set)
{
    if (set.size() == 0 || set.begin()->bytes == 0) return LAZY_BAD_SET;
    if (*set.begin()->slot) return 0;
    return lazy_detail::obtain(mem, set);
}

// Buffers that share one capacity, `set` sized for `need`: nothing to do while cap >= need; otherwise the old buffers
// go, cap = 0, all are made anew, cap = need.
template <typename Mem, typename Cap>
int grow(Mem&& mem, Cap& cap, size_t need, std::initializer_list<BufReq> set)
{
    if (cap >= need) return 0;
    lazy_detail::drop(mem, set);
    cap = 0;
    const int rc = lazy_detail::obtain(mem, set);
    if (rc == 0) cap = need;
    return rc;
}

}  // namespace vl
