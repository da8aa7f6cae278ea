// subset_batch_plan_test.cpp -- csrc/subset_batch_plan.hpp on the CPU: invariants P1-P6 on random job mixes and on the
// named examples.  Built and run (AddressSanitizer + UBSan) by tests/test_subset_batch_plan_cpu.py.
#include "../../vectorlite_amd/csrc/subset_batch_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace vl;

namespace {
int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            if (++g_failed > 20) std::exit(1);            \
        }                                                 \
    } while (0)

// the buffer constants of kernels.hpp, restated (no HIP here)
constexpr uint32_t MAX_JOBS = 512, MERGE_QUERIES = 8, MAX_GRID = 2048;
constexpr uint64_t PARTIAL_LISTS = 8ull * 2048;

SubsetBatchLimits limits(uint32_t resident) { return {resident, MAX_JOBS, PARTIAL_LISTS, MERGE_QUERIES, MAX_GRID}; }

void check_plan(const std::vector<SubsetJob>& jobs, const SubsetBatchLimits& lim, const SubsetBatchPlan& p, const char* what)
{
    std::vector<int> seen(jobs.size(), 0);
    for (uint32_t j : p.single) {
        CHECK(j < jobs.size(), "%s", what);
        seen[j]++;
    }
    for (size_t i = 1; i < p.single.size(); ++i) CHECK(p.single[i - 1] < p.single[i], "%s: single list order", what);
    for (const SubsetLaunch& L : p.launches) {
        const uint64_t c = L.jobs.size();
        CHECK(c >= 2, "%s: P5, a launch of %llu jobs", what, (unsigned long long)c);
        CHECK(c <= lim.max_jobs, "%s: P2 jobs", what);
        CHECK(L.gx >= 1 && (uint64_t)L.gx * c <= lim.partial_lists, "%s: P2 gx %u x %llu", what, L.gx, (unsigned long long)c);
        if (c > lim.merge_queries) CHECK(L.gx <= 64, "%s: P3 gx %u with %llu jobs", what, L.gx, (unsigned long long)c);
        else CHECK(L.gx <= std::min<uint32_t>(lim.max_grid, std::max<uint32_t>(1, lim.resident / (uint32_t)c)), "%s: P3 gx %u", what, L.gx);
        uint64_t busy = 0;
        bool cut = false;
        for (size_t i = 0; i < c; ++i) {
            const uint32_t j = L.jobs[i];
            CHECK(j < jobs.size(), "%s", what);
            if (j >= jobs.size()) continue;
            seen[j]++;
            if (i) CHECK(L.jobs[i - 1] < j, "%s: P1 order inside a launch", what);
            CHECK(jobs[j].fast && jobs[j].m > 0, "%s: job %u may not be batched", what, j);
            busy += std::min<uint32_t>(jobs[j].need, L.gx);
            cut = cut || jobs[j].need > L.gx;
        }
        CHECK(!cut || busy >= lim.resident, "%s: P4 busy %llu of %u at gx %u, %llu jobs", what, (unsigned long long)busy, lim.resident,
              L.gx, (unsigned long long)c);
    }
    for (size_t j = 0; j < jobs.size(); ++j)
        CHECK(seen[j] == (jobs[j].m > 0 ? 1 : 0), "%s: P1 job %zu appears %d times (m = %llu)", what, j, seen[j],
              (unsigned long long)jobs[j].m);
    // P6
    const SubsetBatchPlan again = subset_batch_plan(jobs, lim);
    CHECK(again.single == p.single && again.launches.size() == p.launches.size(), "%s: P6", what);
    for (size_t i = 0; i < p.launches.size() && i < again.launches.size(); ++i)
        CHECK(again.launches[i].jobs == p.launches[i].jobs && again.launches[i].gx == p.launches[i].gx, "%s: P6 launch %zu", what, i);
}

std::vector<SubsetJob> uniform_jobs(size_t n, uint64_t m, int g, int u)
{
    return std::vector<SubsetJob>(n, SubsetJob{m, true, subset_job_need(m, g, u)});
}
}  // namespace

int main()
{
    // the default shapes' (G, U) of VL_SCAN_VARIANTS, and the generic kernel's (G, 1)
    static const int shapes[][2] = {{8, 3}, {8, 2}, {8, 1}, {16, 1}, {1, 1}, {2, 1}, {4, 1}, {32, 1}, {64, 1}};
    static const size_t nqs[] = {1, 2, 8, 9, 512, 513, 5000};
    static const uint64_t ms[] = {0, 1, 63, 64, 65, 2048, 100000, 10000000};
    std::mt19937_64 rng(20240611);
    size_t plans = 0;
    for (const auto& sh : shapes)
        for (size_t nq : nqs)
            for (int rep = 0; rep < 6; ++rep) {
                const uint32_t resident = rep == 0 ? 256 : rep == 1 ? 2048 : 256 + (uint32_t)(rng() % 1793);
                // mixes: everything at random, mostly small with a few whole-index jobs, mostly large
                const int mix = rep % 3;
                std::vector<SubsetJob> jobs(nq);
                for (SubsetJob& j : jobs) {
                    uint64_t m = ms[rng() % 8];
                    if (mix == 1 && rng() % 16) m = ms[1 + rng() % 5];
                    if (mix == 2 && rng() % 4) m = ms[6 + rng() % 2];
                    j.m = m;
                    j.fast = rng() % 8 != 0;
                    j.need = subset_job_need(m, sh[0], sh[1]);
                }
                const SubsetBatchLimits lim = limits(resident);
                check_plan(jobs, lim, subset_batch_plan(jobs, lim), "sweep");
                ++plans;
            }

    {   // nine whole-index filters: launches of 8 or fewer, each filling the resident set (never 9 x 64 workgroups)
        const auto jobs = uniform_jobs(9, 10000000, 8, 1);
        const SubsetBatchLimits lim = limits(1024);
        const SubsetBatchPlan p = subset_batch_plan(jobs, lim);
        check_plan(jobs, lim, p, "9 x 1e7");
        CHECK(!p.launches.empty(), "9 x 1e7: no launch");
        size_t in_launches = 0;
        for (const SubsetLaunch& L : p.launches) {
            CHECK(L.jobs.size() <= 8, "9 x 1e7: a launch of %zu", L.jobs.size());
            CHECK((uint64_t)L.gx * L.jobs.size() >= lim.resident, "9 x 1e7: %u x %zu workgroups", L.gx, L.jobs.size());
            in_launches += L.jobs.size();
        }
        CHECK(in_launches + p.single.size() == 9 && in_launches >= 8, "9 x 1e7: %zu batched", in_launches);
        ++plans;
    }
    {   // 256 filters of 10^4 rows: one launch at the finalize kernel's 64 lists
        const auto jobs = uniform_jobs(256, 10000, 8, 1);
        const SubsetBatchLimits lim = limits(1024);
        const SubsetBatchPlan p = subset_batch_plan(jobs, lim);
        check_plan(jobs, lim, p, "256 x 1e4");
        CHECK(p.launches.size() == 1 && p.single.empty(), "256 x 1e4: %zu launches", p.launches.size());
        if (p.launches.size() == 1) CHECK(p.launches[0].gx == 64 && p.launches[0].jobs.size() == 256, "256 x 1e4: gx %u", p.launches[0].gx);
        ++plans;
    }
    {   // 256 filters of 100 rows: one launch, nobody cut
        const auto jobs = uniform_jobs(256, 100, 8, 1);
        const SubsetBatchLimits lim = limits(1024);
        const SubsetBatchPlan p = subset_batch_plan(jobs, lim);
        check_plan(jobs, lim, p, "256 x 100");
        CHECK(p.launches.size() == 1 && p.single.empty(), "256 x 100: %zu launches", p.launches.size());
        if (p.launches.size() == 1) CHECK(p.launches[0].gx >= jobs[0].need, "256 x 100: gx %u cuts need %u", p.launches[0].gx, jobs[0].need);
        ++plans;
    }
    {   // one job: the single list
        const auto jobs = uniform_jobs(1, 5000, 8, 1);
        const SubsetBatchLimits lim = limits(1024);
        const SubsetBatchPlan p = subset_batch_plan(jobs, lim);
        check_plan(jobs, lim, p, "one job");
        CHECK(p.launches.empty() && p.single.size() == 1, "one job");
        ++plans;
    }
    {   // 513 small jobs: two launches of equal share, nothing single
        const auto jobs = uniform_jobs(513, 200, 8, 1);
        const SubsetBatchLimits lim = limits(1024);
        const SubsetBatchPlan p = subset_batch_plan(jobs, lim);
        check_plan(jobs, lim, p, "513 x 200");
        CHECK(p.launches.size() == 2 && p.single.empty(), "513 x 200: %zu launches, %zu single", p.launches.size(), p.single.size());
        ++plans;
    }
    {   // three whole-index filters among twenty small ones: the small ones share a launch that cuts nobody
        std::vector<SubsetJob> jobs = uniform_jobs(23, 50, 4, 2);
        for (size_t j : {0u, 11u, 22u}) jobs[j] = {200000, true, subset_job_need(200000, 4, 2)};
        const SubsetBatchLimits lim = limits(1792);
        const SubsetBatchPlan p = subset_batch_plan(jobs, lim);
        check_plan(jobs, lim, p, "3 big + 20 small");
        bool small_together = false;
        for (const SubsetLaunch& L : p.launches) small_together = small_together || L.jobs.size() == 20;
        CHECK(small_together, "3 big + 20 small: the small jobs do not share one launch");
        ++plans;
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("%zu plans checked\n", plans);
    return 0;
}
