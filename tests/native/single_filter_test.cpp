// single_filter.hpp on the CPU: VL_SINGLE_FILTER parsing, and the auto mode's window / probe rule -- a bad streak pauses
// the bf16 filter within a bounded number of searches, costs one search in PROBE_EVERY while paused, and certifying
// queries bring it back.
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

// n searches whose bf16 try certifies (ok) or not; returns how many of them tried the filter
static int run(AutoFilterWindow& w, int n, bool ok)
{
    int tried = 0;
    for (int i = 0; i < n; ++i)
        if (w.want()) {
            ++tried;
            w.record(ok);
        }
    return tried;
}

int main()
{
    CHECK(parse_single_filter(nullptr, FILTER_AUTO) == FILTER_AUTO);
    CHECK(parse_single_filter("f32", FILTER_AUTO) == FILTER_F32);
    CHECK(parse_single_filter("bf16", FILTER_AUTO) == FILTER_BF16);
    CHECK(parse_single_filter("auto", FILTER_F32) == FILTER_AUTO);
    CHECK(parse_single_filter("", FILTER_AUTO) == FILTER_AUTO);
    CHECK(parse_single_filter("BF16", FILTER_AUTO) == FILTER_AUTO);
    CHECK(parse_single_filter("1", FILTER_AUTO) == FILTER_AUTO);

    AutoFilterWindow w;
    CHECK(w.on());
    CHECK(run(w, 1000, true) == 1000);  // certifying queries: always on
    // a streak of uncertifiable queries: on for at most MAX_FAILS + 1 of them, then paused
    int tried = run(w, AutoFilterWindow::MAX_FAILS + 1, false);
    CHECK(tried == AutoFilterWindow::MAX_FAILS + 1);
    CHECK(!w.on());
    // paused: one try in PROBE_EVERY searches, whatever the length of the streak
    tried = run(w, 160 * AutoFilterWindow::PROBE_EVERY, false);
    CHECK(tried == 160);
    CHECK(!w.on());
    // certifying queries again: back on within WINDOW probes
    int n = 0;
    while (!w.on() && n < 2 * AutoFilterWindow::WINDOW * AutoFilterWindow::PROBE_EVERY) {
        run(w, 1, true);
        ++n;
    }
    CHECK(w.on());
    CHECK(n <= AutoFilterWindow::WINDOW * AutoFilterWindow::PROBE_EVERY);
    CHECK(run(w, 100, true) == 100);
    // a mixed stream that certifies 3 queries in 4 stays on
    w.reset();
    for (int i = 0; i < 4000; ++i) {
        CHECK(w.want());
        w.record(i % 4 != 0);
    }
    // a fresh window after reset() (set_single_filter)
    w.reset();
    run(w, 200, false);
    CHECK(!w.on());
    w.reset();
    CHECK(w.on());
    printf("%s single_filter checks\n", fails ? "FAILED" : "passed");
    return fails ? 1 : 0;
}
