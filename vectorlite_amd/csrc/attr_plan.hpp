// attr_plan.hpp -- the host half of an attribute column (vl_index_attr_create / vl_index_attr_set).
//
// The caller hands over (id, int64 value) pairs in any order.  The plan sorts them by id, drops exact repeats and rejects an
// id that carries two different values within one call.  attr_plan_merge upserts a second batch of pairs into a plan: an id
// already held takes the new value, other ids are added; it writes into a plan of its own, so a refusal leaves the column
// as it was.  Plain C++ with no device code in it: it builds with a host compiler alone (tests/native/attr_plan_test.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace vl {

constexpr uint64_t ATTR_MAX_PAIRS = 0xFFFFFFFFull;  // a column holds fewer pairs than this (u32 lower bounds on the device)

enum : int { ATTR_PLAN_OK = 0, ATTR_PLAN_CONFLICT = 1, ATTR_PLAN_TOO_MANY = 2 };

struct AttrPlan {
    std::vector<uint64_t> ids;    // sorted, unique
    std::vector<int64_t> values;  // values[i]: the value of ids[i]
};

// ATTR_PLAN_CONFLICT: some id carries two different values (*conflict_id names the smallest such id); ATTR_PLAN_TOO_MANY:
// max_pairs pairs or more.  Either way the plan is left empty.
inline int attr_plan_build(const uint64_t* ids, const int64_t* values, uint64_t n, AttrPlan* plan, uint64_t* conflict_id = nullptr,
                           uint64_t max_pairs = ATTR_MAX_PAIRS)
{
    plan->ids.clear();
    plan->values.clear();
    if (n >= max_pairs) return ATTR_PLAN_TOO_MANY;
    std::vector<std::pair<uint64_t, int64_t>> pairs(n);
    for (uint64_t i = 0; i < n; ++i) pairs[i] = {ids[i], values[i]};
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    for (size_t i = 1; i < pairs.size(); ++i)
        if (pairs[i].first == pairs[i - 1].first) {  // exact repeats are gone: the same id with another value
            if (conflict_id) *conflict_id = pairs[i].first;
            return ATTR_PLAN_CONFLICT;
        }
    plan->ids.resize(pairs.size());
    plan->values.resize(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) {
        plan->ids[i] = pairs[i].first;
        plan->values[i] = pairs[i].second;
    }
    return ATTR_PLAN_OK;
}

// *out = cur with the n pairs upserted.  The pairs obey attr_plan_build's rules among themselves; the merged column holds
// fewer than max_pairs pairs.  On a refusal *out is left empty and cur, which is only read, stands.
inline int attr_plan_merge(const AttrPlan& cur, const uint64_t* ids, const int64_t* values, uint64_t n, AttrPlan* out,
                           uint64_t* conflict_id = nullptr, uint64_t max_pairs = ATTR_MAX_PAIRS)
{
    AttrPlan upd;
    out->ids.clear();
    out->values.clear();
    const int rc = attr_plan_build(ids, values, n, &upd, conflict_id, max_pairs);
    if (rc != ATTR_PLAN_OK) return rc;
    AttrPlan merged;
    merged.ids.reserve(cur.ids.size() + upd.ids.size());
    merged.values.reserve(cur.ids.size() + upd.ids.size());
    size_t a = 0, b = 0;
    while (a < cur.ids.size() || b < upd.ids.size()) {
        const bool take_new = a == cur.ids.size() || (b < upd.ids.size() && upd.ids[b] <= cur.ids[a]);
        if (take_new) {
            if (a < cur.ids.size() && cur.ids[a] == upd.ids[b]) ++a;  // an id already held takes the new value
            merged.ids.push_back(upd.ids[b]);
            merged.values.push_back(upd.values[b]);
            ++b;
        } else {
            merged.ids.push_back(cur.ids[a]);
            merged.values.push_back(cur.values[a]);
            ++a;
        }
    }
    if (merged.ids.size() >= max_pairs) return ATTR_PLAN_TOO_MANY;
    *out = std::move(merged);
    return ATTR_PLAN_OK;
}

}  // namespace vl
