// The host half of an attribute column (csrc/attr_plan.hpp) on the CPU: the pairs sorted by id, exact repeats dropped,
// conflicting repeats rejected with the smallest such id named, the upsert of vl_index_attr_set against a std::map
// restatement, and the size limit.  Stand-alone; built with AddressSanitizer + UBSan.
#include "../../vectorlite_amd/csrc/attr_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>

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

using Map = std::map<uint64_t, int64_t>;

// id -> value of one call's pairs; false (and *bad = the smallest offending id) when an id carries two values
bool pairs_to_map(const std::vector<uint64_t>& ids, const std::vector<int64_t>& vals, Map* out, uint64_t* bad)
{
    out->clear();
    bool conflict = false;
    for (size_t i = 0; i < ids.size(); ++i) {
        auto it = out->find(ids[i]);
        if (it == out->end()) (*out)[ids[i]] = vals[i];
        else if (it->second != vals[i]) {
            if (!conflict || ids[i] < *bad) *bad = ids[i];
            conflict = true;
        }
    }
    return !conflict;
}

bool same(const vl::AttrPlan& p, const Map& m)
{
    if (p.ids.size() != m.size() || p.values.size() != m.size()) return false;
    size_t i = 0;
    for (const auto& kv : m) {  // ascending ids
        if (p.ids[i] != kv.first || p.values[i] != kv.second) return false;
        ++i;
    }
    return true;
}

void check_build(const std::vector<uint64_t>& ids, const std::vector<int64_t>& vals, const char* what)
{
    Map m;
    uint64_t want_bad = 0, bad = 0;
    const bool ok = pairs_to_map(ids, vals, &m, &want_bad);
    vl::AttrPlan p;
    const int rc = vl::attr_plan_build(ids.data(), vals.data(), ids.size(), &p, &bad);
    EXPECT((rc == vl::ATTR_PLAN_OK) == ok, "%s: rc = %d, conflict = %d", what, rc, (int)!ok);
    if (!ok) {
        EXPECT(rc == vl::ATTR_PLAN_CONFLICT, "%s: a conflict is reported as one (%d)", what, rc);
        EXPECT(bad == want_bad, "%s: names id %llu, want the smallest, %llu", what, (unsigned long long)bad, (unsigned long long)want_bad);
        EXPECT(p.ids.empty() && p.values.empty(), "%s: a rejected plan is empty", what);
        return;
    }
    EXPECT(same(p, m), "%s: the plan is the map", what);
}
}  // namespace

int main()
{
    const int64_t I64_MIN = std::numeric_limits<int64_t>::min(), I64_MAX = std::numeric_limits<int64_t>::max();
    // sort and dedup
    {
        const std::vector<uint64_t> ids = {30, 10, 20, 10, 40, ~0ull, 0};
        const std::vector<int64_t> vals = {-7, 9, I64_MIN, 9, I64_MAX, 0, -1};
        vl::AttrPlan p;
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), ids.size(), &p) == vl::ATTR_PLAN_OK, "plain build");
        EXPECT((p.ids == std::vector<uint64_t>{0, 10, 20, 30, 40, ~0ull}), "ids sorted, the exact repeat dropped");
        EXPECT((p.values == std::vector<int64_t>{-1, 9, I64_MIN, -7, I64_MAX, 0}), "values follow their ids");
        check_build(ids, vals, "plain");
    }
    // conflicts: the smallest conflicting id is named, whatever the order
    {
        const std::vector<uint64_t> ids = {9, 6, 5, 9, 6, 5};
        const std::vector<int64_t> vals = {1, 2, 3, 4, 5, 3};
        vl::AttrPlan p;
        uint64_t bad = 0;
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), 6, &p, &bad) == vl::ATTR_PLAN_CONFLICT, "conflict rejected");
        EXPECT(bad == 6, "the smallest conflicting id is named (%llu)", (unsigned long long)bad);
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), 6, &p) == vl::ATTR_PLAN_CONFLICT, "rejected without an out pointer");
        EXPECT(p.ids.empty(), "a rejected plan is empty");
        check_build(ids, vals, "two conflicts");
    }
    // n = 0 and the size limit (decided before a pair is read)
    {
        vl::AttrPlan p;
        p.ids.push_back(1);
        EXPECT(vl::attr_plan_build(nullptr, nullptr, 0, &p) == vl::ATTR_PLAN_OK && p.ids.empty() && p.values.empty(), "n = 0 builds empty");
        EXPECT(vl::attr_plan_build(nullptr, nullptr, 0xFFFFFFFFull, &p) == vl::ATTR_PLAN_TOO_MANY, "2^32 - 1 pairs refused");
        EXPECT(vl::attr_plan_build(nullptr, nullptr, ~0ull, &p) == vl::ATTR_PLAN_TOO_MANY, "2^64 - 1 pairs refused");
        EXPECT(vl::ATTR_MAX_PAIRS == 0xFFFFFFFFull, "the limit is 2^32 - 1");
        const std::vector<uint64_t> ids = {1, 2, 3, 3};
        const std::vector<int64_t> vals = {1, 2, 3, 3};
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), 3, &p, nullptr, 4) == vl::ATTR_PLAN_OK, "3 pairs under a limit of 4");
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), 4, &p, nullptr, 4) == vl::ATTR_PLAN_TOO_MANY, "4 pairs at a limit of 4");
        // the merged size counts, not the batch's
        vl::AttrPlan cur, out;
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), 3, &cur) == vl::ATTR_PLAN_OK, "base");
        const std::vector<uint64_t> more = {3, 4};
        const std::vector<int64_t> mv = {30, 40};
        EXPECT(vl::attr_plan_merge(cur, more.data(), mv.data(), 1, &out, nullptr, 4) == vl::ATTR_PLAN_OK && out.ids.size() == 3, "a replacement does not grow the column");
        EXPECT(vl::attr_plan_merge(cur, more.data(), mv.data(), 2, &out, nullptr, 4) == vl::ATTR_PLAN_TOO_MANY, "the merged column reaches the limit");
        EXPECT(out.ids.empty() && cur.ids.size() == 3 && cur.values[2] == 3, "the refusal leaves the column as it was");
    }
    // merge: replace, add, a conflict within the call, a refusal leaves the plan untouched
    {
        const std::vector<uint64_t> ids = {10, 20, 30};
        const std::vector<int64_t> vals = {1, 2, 3};
        vl::AttrPlan cur, out;
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), 3, &cur) == vl::ATTR_PLAN_OK, "base");
        const std::vector<uint64_t> u = {20, 5, 35, 20, ~0ull};
        const std::vector<int64_t> uv = {-2, 50, I64_MIN, -2, I64_MAX};
        EXPECT(vl::attr_plan_merge(cur, u.data(), uv.data(), u.size(), &out) == vl::ATTR_PLAN_OK, "merge");
        EXPECT((out.ids == std::vector<uint64_t>{5, 10, 20, 30, 35, ~0ull}), "ids merged in order");
        EXPECT((out.values == std::vector<int64_t>{50, 1, -2, 3, I64_MIN, I64_MAX}), "an id already held takes the new value");
        EXPECT((cur.ids == ids && cur.values == vals), "the source plan is only read");
        const std::vector<uint64_t> c = {40, 20, 40, 20};
        const std::vector<int64_t> cv = {1, 7, 2, 8};
        uint64_t bad = 0;
        EXPECT(vl::attr_plan_merge(cur, c.data(), cv.data(), 4, &out, &bad) == vl::ATTR_PLAN_CONFLICT && bad == 20, "a conflict within the call names id 20 (%llu)", (unsigned long long)bad);
        EXPECT(out.ids.empty() && cur.ids == ids && cur.values == vals, "the refusal leaves the column as it was");
        // a value that differs from the HELD one is no conflict: it replaces
        const std::vector<uint64_t> r = {30};
        const std::vector<int64_t> rv = {-3};
        EXPECT(vl::attr_plan_merge(cur, r.data(), rv.data(), 1, &out) == vl::ATTR_PLAN_OK && out.values[2] == -3, "replace alone");
        EXPECT(vl::attr_plan_merge(cur, nullptr, nullptr, 0, &out) == vl::ATTR_PLAN_OK && out.ids == ids && out.values == vals, "an empty batch copies");
        vl::AttrPlan empty;
        EXPECT(vl::attr_plan_merge(empty, u.data(), uv.data(), u.size(), &out) == vl::ATTR_PLAN_OK && out.ids.size() == 4, "into an empty column");
    }
    // random streams of builds and merges against the map
    std::mt19937_64 rng(20241021);
    for (int round = 0; round < 40; ++round) {
        const size_t n = 1 + rng() % 2000;
        const uint64_t id_space = 1 + rng() % (2 * n);
        std::vector<uint64_t> ids(n);
        std::vector<int64_t> vals(n);
        for (size_t i = 0; i < n; ++i) {
            ids[i] = rng() % id_space;
            vals[i] = (int64_t)(ids[i] * 0x9E3779B97F4A7C15ull) >> (rng() % 2 ? 0 : 40);  // a function of the id and a coin: some conflicts
        }
        if (round % 2 == 0)
            for (size_t i = 0; i < n; ++i) vals[i] = (int64_t)(ids[i] * 0x9E3779B97F4A7C15ull);  // repeats agree
        check_build(ids, vals, "random");
        Map held;
        uint64_t dummy = 0;
        vl::AttrPlan cur;
        if (!pairs_to_map(ids, vals, &held, &dummy)) continue;
        EXPECT(vl::attr_plan_build(ids.data(), vals.data(), n, &cur) == vl::ATTR_PLAN_OK, "random base");
        for (int step = 0; step < 6; ++step) {
            const size_t k = rng() % 300;
            std::vector<uint64_t> u(k);
            std::vector<int64_t> uv(k);
            for (size_t i = 0; i < k; ++i) {
                u[i] = rng() % (id_space + 50);
                uv[i] = (int64_t)(u[i] + (uint64_t)step) * (step % 3 == 2 && i % 97 == 0 ? (int64_t)i : 1);
            }
            Map upd;
            uint64_t want_bad = 0, bad = 0;
            const bool ok = pairs_to_map(u, uv, &upd, &want_bad);
            vl::AttrPlan out;
            const int rc = vl::attr_plan_merge(cur, u.data(), uv.data(), k, &out, &bad);
            EXPECT((rc == vl::ATTR_PLAN_OK) == ok, "random merge: rc = %d, conflict = %d", rc, (int)!ok);
            if (!ok) {
                EXPECT(bad == want_bad && out.ids.empty() && same(cur, held), "random merge: a refusal names the smallest id and changes nothing");
                continue;
            }
            for (const auto& kv : upd) held[kv.first] = kv.second;
            EXPECT(same(out, held), "random merge: the merged plan is the map");
            cur = out;
        }
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("attr plan ok\n");
    return 0;
}
