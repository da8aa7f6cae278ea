// subset_batch_plan.hpp -- which (query, filter) jobs of a filtered batch share a launch of k_scan_subset_jobs, and on how
// many workgroups per job.  Pure host arithmetic (no HIP): tests/native/subset_batch_plan_test.cpp checks the invariants
// below on the CPU; flat_index.cpp (search_batch_filters) fills the jobs and launches what this returns.
//
//   P1  every job with m > 0 is in exactly one launch or in the single list; inside a launch the jobs are in query order
//   P2  a launch holds at most max_jobs jobs, gx >= 1, gx * jobs <= partial_lists
//   P3  a launch of more than merge_queries jobs has gx <= 64 (its lists reach the finalize kernel without a merge level:
//       the merge scratch holds merge_queries queries); a smaller one may use up to min(max_grid, resident / jobs)
//   P4  no launch leaves the machine idle because of a cap: a job is cut when need > gx, and in every launch either no job
//       is cut or sum(min(need, gx)) >= resident
//   P5  a launch of one job is not a launch: that job goes to the single list
//   P6  the plan is a function of its arguments
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace vl {

struct SubsetJob {
    uint64_t m;     // rows of the job's filter
    bool fast;      // may take the fast path (search_subset's conditions)
    uint32_t need;  // workgroups a lone subset scan of m rows would use before its resident cap (subset_job_need)
};

struct SubsetBatchLimits {
    uint32_t resident;       // workgroups of the scan kernel that are resident at once (what scan_grid caps at)
    uint32_t max_jobs;       // K3_PIPE_QUERIES: jobs staged, launched and synchronised together
    uint64_t partial_lists;  // PARTIALS32_LISTS: lists the partial-list buffer holds
    uint32_t merge_queries;  // SCAN_BATCH_QB: queries the merge scratch behind the lists holds
    uint32_t max_grid;       // SCAN_BATCH_MAX_GRID
};

struct SubsetLaunch {
    std::vector<uint32_t> jobs;  // job numbers, ascending
    uint32_t gx;                 // workgroups per job: the grid is (gx, jobs.size())
};

struct SubsetBatchPlan {
    std::vector<SubsetLaunch> launches;
    std::vector<uint32_t> single;  // jobs left to the single filtered search, ascending
};

// scan_grid's block count for m rows at (lanes per row g, row groups in flight u), before any cap
inline uint32_t subset_job_need(uint64_t m, int g, int u)
{
    const uint64_t rps = 64 / (uint64_t)g;
    const uint64_t steps = (m + rps - 1) / rps;
    const uint64_t per_block = 4ull * (uint64_t)u;
    const uint64_t blocks = (steps + per_block - 1) / per_block;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 0xFFFFFFFFull);
}

namespace subset_plan_detail {
inline uint32_t grid_for(const std::vector<SubsetJob>& jobs, const std::vector<uint32_t>& set, const SubsetBatchLimits& lim)
{
    const uint64_t c = set.size();
    uint64_t gx = 1;
    for (uint32_t j : set) gx = std::max<uint64_t>(gx, jobs[j].need);  // more than the widest job can use helps nobody
    gx = std::min<uint64_t>(gx, lim.partial_lists / c);
    if (c > lim.merge_queries) gx = std::min<uint64_t>(gx, 64);
    else gx = std::min<uint64_t>(gx, std::min<uint64_t>(lim.max_grid, lim.resident / c));
    return (uint32_t)std::max<uint64_t>(gx, 1);
}

// Jobs that the shared width cuts while the launch as a whole would not fill the machine are taken out and planned among
// themselves (fewer jobs: a wider grid each); what stays is cut by nothing.  A set in which every job is cut and that
// still does not fill the machine (more than merge_queries jobs at 64 workgroups each, or resident / jobs rounding
// down) is shortened from the front.
inline void plan_set(const std::vector<SubsetJob>& jobs, std::vector<uint32_t> set, const SubsetBatchLimits& lim, SubsetBatchPlan* p)
{
    while (!set.empty()) {
        if (set.size() == 1) {
            p->single.push_back(set[0]);
            return;
        }
        const uint32_t gx = grid_for(jobs, set, lim);
        uint64_t busy = 0;
        std::vector<uint32_t> cut, whole;
        for (uint32_t j : set) {
            busy += std::min<uint32_t>(jobs[j].need, gx);
            (jobs[j].need > gx ? cut : whole).push_back(j);
        }
        if (cut.empty() || busy >= lim.resident) {
            p->launches.push_back({std::move(set), gx});
            return;
        }
        if (!whole.empty()) {
            plan_set(jobs, std::move(whole), lim, p);
            set = std::move(cut);
        } else if (set.size() > lim.merge_queries) {
            std::vector<uint32_t> head(set.begin(), set.begin() + lim.merge_queries);
            set.erase(set.begin(), set.begin() + lim.merge_queries);
            plan_set(jobs, std::move(head), lim, p);
        } else {
            p->single.push_back(set[0]);
            set.erase(set.begin());
        }
    }
}
}  // namespace subset_plan_detail

inline SubsetBatchPlan subset_batch_plan(const std::vector<SubsetJob>& jobs, const SubsetBatchLimits& lim)
{
    SubsetBatchPlan p;
    std::vector<uint32_t> fast;
    for (uint32_t j = 0; j < (uint32_t)jobs.size(); ++j) {
        if (jobs[j].m == 0) continue;  // answered empty
        if (jobs[j].fast) fast.push_back(j);
        else p.single.push_back(j);
    }
    // the fewest launches max_jobs allows, in equal shares (513 jobs: 257 + 256, not 512 and one left over)
    const uint64_t n = fast.size(), cap = std::max<uint32_t>(lim.max_jobs, 1);
    const uint64_t parts = (n + cap - 1) / cap;
    for (uint64_t i = 0; i < parts; ++i) {
        const uint64_t lo = n * i / parts, hi = n * (i + 1) / parts;
        subset_plan_detail::plan_set(jobs, std::vector<uint32_t>(fast.begin() + lo, fast.begin() + hi), lim, &p);
    }
    std::sort(p.single.begin(), p.single.end());
    return p;
}

}  // namespace vl
