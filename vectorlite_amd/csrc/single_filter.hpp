// single_filter.hpp -- which slab a single-query search streams first, and the auto mode's switch-off rule.  Pure host
// code (no HIP): tests/native/single_filter_test.cpp checks the parsing and the window / probe rule on the CPU;
// flat_index.cpp applies it per handle.
#pragma once

#include <stdint.h>
#include <string.h>

#include <atomic>

namespace vl {

// vl_index_set_single_filter modes: 0 the f32 slab only, 1 the bf16 copy first always, 2 auto (new handles), 3 the int8
// copy first always
constexpr int FILTER_F32 = 0, FILTER_BF16 = 1, FILTER_AUTO = 2, FILTER_I8 = 3;

// VL_SINGLE_FILTER=f32|bf16|auto|i8 -> mode; anything else (or unset) -> dflt
inline int parse_single_filter(const char* s, int dflt)
{
    if (!s) return dflt;
    if (strcmp(s, "f32") == 0) return FILTER_F32;
    if (strcmp(s, "bf16") == 0) return FILTER_BF16;
    if (strcmp(s, "auto") == 0) return FILTER_AUTO;
    if (strcmp(s, "i8") == 0) return FILTER_I8;
    return dflt;
}

// The auto mode looks at the last WINDOW outcomes of one filter stage only (each stage of the ladder has its own window) (one bit each, 1 = not certified): it is off
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
    // does this search try the stage
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

// Mode 1 / mode 3's one-way rule: a stage asked for explicitly switches itself off for good once more than a third of
// 64 or more tries failed to certify.
inline bool forced_stage_on(uint64_t tries, uint64_t fails) { return !(tries >= 64 && fails * 3 > tries); }

// Does a single search run the filter stage `stage` (FILTER_I8 or FILTER_BF16) before the f32 scan?  The ladder is
// int8, then bf16, then f32; a stage runs when its copy supports the query (ok: the (dim, metric), nothing skipping it --
// an MFMA straggler skips both -- and, in auto, the copy not known to be unallocatable) and
//   - the mode asks for exactly this stage: then `forced()` (forced_stage_on of its counters) decides;
//   - auto: the f32 slab is at least the stage's floor, and then `window()` (its AutoFilterWindow's want()) decides --
//     consulted only past the floor, so a probe is never spent on a stage that could not run.
// The stages are asked in ladder order and the bf16 one only after the int8 one failed to certify.
template <class Forced, class Window>
inline bool ladder_stage(int stage, int mode, bool ok, uint64_t slab_bytes, uint64_t min_bytes, Forced forced, Window window)
{
    if (!ok) return false;
    if (mode == stage) return forced();
    if (mode != FILTER_AUTO) return false;
    return slab_bytes >= min_bytes && window();
}

}  // namespace vl
