// group_plan.hpp -- the host half of a group table (vl_index_groups_create).
//
// The caller hands over (id, group key) pairs in any order.  The plan sorts them by id, drops exact repeats, rejects an id
// that carries two different keys, and numbers the distinct keys densely: the device works with u32 group numbers (one slot
// of best[] / first[] per number), the keys come back only with the answer.  Plain C++ with no HIP in it: it builds with a
// host compiler alone (tests/native/group_plan_test.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace vl {

constexpr uint32_t GROUP_NONE = 0xFFFFFFFFu;  // group_of_row[] of a row whose id the table does not hold

struct GroupPlan {
    std::vector<uint64_t> ids;    // sorted, unique
    std::vector<uint32_t> dense;  // dense[i]: the group number of ids[i], < keys.size()
    std::vector<uint64_t> keys;   // group number -> the caller's key, ascending
};

// false: some id carries two different keys (*conflict_id names the smallest such id) or there are 2^32 - 1 pairs or more;
// the plan is left empty.
inline bool group_plan_build(const uint64_t* ids, const uint64_t* group_keys, uint64_t n, GroupPlan* plan,
                             uint64_t* conflict_id = nullptr)
{
    plan->ids.clear();
    plan->dense.clear();
    plan->keys.clear();
    if (n >= (uint64_t)GROUP_NONE) return false;
    std::vector<std::pair<uint64_t, uint64_t>> pairs(n);
    for (uint64_t i = 0; i < n; ++i) pairs[i] = {ids[i], group_keys[i]};
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    for (size_t i = 1; i < pairs.size(); ++i)
        if (pairs[i].first == pairs[i - 1].first) {  // exact repeats are gone: the same id with another key
            if (conflict_id) *conflict_id = pairs[i].first;
            return false;
        }
    plan->keys.reserve(pairs.size());
    for (const auto& p : pairs) plan->keys.push_back(p.second);
    std::sort(plan->keys.begin(), plan->keys.end());
    plan->keys.erase(std::unique(plan->keys.begin(), plan->keys.end()), plan->keys.end());
    plan->ids.resize(pairs.size());
    plan->dense.resize(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) {
        plan->ids[i] = pairs[i].first;
        plan->dense[i] = (uint32_t)(std::lower_bound(plan->keys.begin(), plan->keys.end(), pairs[i].second) - plan->keys.begin());
    }
    return true;
}

}  // namespace vl
