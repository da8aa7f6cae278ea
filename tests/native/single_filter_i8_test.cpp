// single_filter.hpp's int8 additions on the CPU: VL_SINGLE_FILTER=i8 parsing, the one-way rule of modes 1 and 3, and
// ladder_stage -- which stages of int8 -> bf16 -> f32 a single search runs in each mode, with the floors and windows.
#include "../../vectorlite_amd/csrc/single_filter.hpp"

#include <stdio.h>

using namespace vl;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
            ++fails;                                                \
        }                                                           \
    } while (0)

int main()
{
    CHECK(parse_single_filter("i8", FILTER_AUTO) == FILTER_I8);
    CHECK(parse_single_filter("I8", FILTER_AUTO) == FILTER_AUTO);
    CHECK(parse_single_filter("int8", FILTER_AUTO) == FILTER_AUTO);
    CHECK(parse_single_filter("3", FILTER_F32) == FILTER_F32);

    CHECK(forced_stage_on(0, 0));
    CHECK(forced_stage_on(63, 63));   // fewer than 64 tries: on whatever they did
    CHECK(forced_stage_on(64, 21));
    CHECK(!forced_stage_on(64, 22));  // more than a third of 64 failed: off for good
    CHECK(!forced_stage_on(300, 101));

    const uint64_t MB = 1ull << 20, i8_floor = 1024 * MB, bf16_floor = 512 * MB;
    int forced_calls = 0, window_calls = 0;
    auto stage = [&](int st, int mode, bool ok, uint64_t bytes, bool forced_on, bool window_on) {
        const uint64_t floor = st == FILTER_I8 ? i8_floor : bf16_floor;
        return ladder_stage(st, mode, ok, bytes, floor, [&] { ++forced_calls; return forced_on; },
                            [&] { ++window_calls; return window_on; });
    };
    // mode 3: the int8 stage at any size, under its one-way rule; never the bf16 stage
    CHECK(stage(FILTER_I8, FILTER_I8, true, 1, true, false));
    CHECK(!stage(FILTER_I8, FILTER_I8, true, 1, false, true));
    CHECK(!stage(FILTER_I8, FILTER_I8, false, 1 << 30, true, true));
    CHECK(!stage(FILTER_BF16, FILTER_I8, true, 1ull << 40, true, true));
    // mode 1: the bf16 stage only
    CHECK(stage(FILTER_BF16, FILTER_BF16, true, 1, true, false));
    CHECK(!stage(FILTER_I8, FILTER_BF16, true, 1ull << 40, true, true));
    // mode 0: neither
    CHECK(!stage(FILTER_I8, FILTER_F32, true, 1ull << 40, true, true));
    CHECK(!stage(FILTER_BF16, FILTER_F32, true, 1ull << 40, true, true));
    // auto: each stage past its own floor, then its window decides
    forced_calls = window_calls = 0;
    CHECK(!stage(FILTER_I8, FILTER_AUTO, true, i8_floor - 1, true, true));  // between the floors: no int8 ...
    CHECK(stage(FILTER_BF16, FILTER_AUTO, true, i8_floor - 1, true, true));  // ... but bf16
    CHECK(!stage(FILTER_BF16, FILTER_AUTO, true, bf16_floor - 1, true, true));
    CHECK(window_calls == 1);  // below a floor the window (and its probe counter) is not consulted
    CHECK(stage(FILTER_I8, FILTER_AUTO, true, i8_floor, false, true));
    CHECK(!stage(FILTER_I8, FILTER_AUTO, true, i8_floor, true, false));  // paused window
    CHECK(!stage(FILTER_I8, FILTER_AUTO, false, 1ull << 40, true, true)); // unsupported / unallocatable
    CHECK(forced_calls == 0);  // auto never applies the one-way rule

    // auto, the two windows are independent: a streak of uncertifiable queries fails both stages; each pauses on its
    // own rule, each probes every PROBE_EVERY-th eligible search
    AutoFilterWindow wi, wb;
    int i8_runs = 0, bf16_runs = 0;
    for (int s = 0; s < 200; ++s) {
        if (wi.want()) {
            ++i8_runs;
            wi.record(false);
        }
        if (wb.want()) {
            ++bf16_runs;
            wb.record(false);
        }
    }
    CHECK(i8_runs == AutoFilterWindow::MAX_FAILS + 1 + (200 - AutoFilterWindow::MAX_FAILS - 1) / AutoFilterWindow::PROBE_EVERY);
    CHECK(bf16_runs == i8_runs);
    // int8 certifies again: its window recovers while the bf16 one (never asked: the int8 stage answered) stays paused
    int back = -1;
    for (int s = 0; s < 64 * AutoFilterWindow::PROBE_EVERY + 16 && back < 0; ++s)
        if (wi.want()) {
            wi.record(true);
            if (wi.on()) back = s;
        }
    CHECK(back >= 0);
    CHECK(wi.on());
    CHECK(!wb.on());

    if (fails) return 1;
    printf("passed single_filter i8 checks\n");
    return 0;
}
