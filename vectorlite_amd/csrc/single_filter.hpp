// single_filter.hpp -- which slab a single-query search streams first, and the auto mode's switch-off rule.  Pure host
// code (no HIP): tests/native/single_filter_test.cpp checks the parsing and the window / probe rule on the CPU;
// flat_index.cpp applies it per handle.
#pragma once

#include <stdint.h>
#include <string.h>

#include <atomic>

namespace vl {

// vl_index_set_single_filter modes: 0 the f32 slab only, 1 the bf16 copy first always, 2 auto (new handles)
constexpr int FILTER_F32 = 0, FILTER_BF16 = 1, FILTER_AUTO = 2;

// VL_SINGLE_FILTER=f32|bf16|auto -> mode; anything else (or unset) -> dflt
inline int parse_single_filter(const char* s, int dflt)
{
    if (!s) return dflt;
    if (strcmp(s, "f32") == 0) return FILTER_F32;
    if (strcmp(s, "bf16") == 0) return FILTER_BF16;
    if (strcmp(s, "auto") == 0) return FILTER_AUTO;
    return dflt;
}

// The auto mode looks at the last WINDOW outcomes of the bf16 filter only (one bit each, 1 = not certified): it is off
// while more than MAX_FAILS of them (a third) failed, and while off every PROBE_EVERY-th eligible search tries it again,
// so a bad streak (a dense neighbourhood, planted duplicates) pauses it and certifying queries bring it back.  Cost
// bounds: on, a streak of uncertifiable queries pays the extra bf16 pass at most MAX_FAILS + 1 times in a row; off, one
// search in PROBE_EVERY pays it.  The counters race benignly between threads: a lost update moves a decision by one
// search, never an answer.
struct AutoFilterWindow {
    static constexpr int WINDOW = 64;
    static constexpr int MAX_FAILS = 21;
    static constexpr int PROBE_EVERY = 16;
    std::atomic<uint64_t> hist{0}, skips{0};

    void reset()
    {
        hist.store(0, std::memory_order_relaxed);
        skips.store(0, std::memory_order_relaxed);
    }
    bool on() const { return __builtin_popcountll(hist.load(std::memory_order_relaxed)) <= MAX_FAILS; }
    // does this search try the bf16 filter
    bool want()
    {
        if (on()) return true;
        return (skips.fetch_add(1, std::memory_order_relaxed) + 1) % PROBE_EVERY == 0;
    }
    void record(bool certified)
    {
        uint64_t h = hist.load(std::memory_order_relaxed);
        while (!hist.compare_exchange_weak(h, (h << 1) | (certified ? 0u : 1u), std::memory_order_relaxed)) {
        }
    }
};

}  // namespace vl
