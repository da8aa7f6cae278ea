// The host half of a group table (csrc/group_plan.hpp) on the CPU: the pairs sorted by id, the distinct keys numbered
// densely in ascending key order, conflicting repeats rejected.  Stand-alone; built with AddressSanitizer + UBSan.
#include "../../vectorlite_amd/csrc/group_plan.hpp"

#include <cstdio>
#include <cstdlib>
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

// the plan restated with std::map: id -> key, then key -> rank among the distinct keys
void check_against_map(const std::vector<uint64_t>& ids, const std::vector<uint64_t>& keys, const char* what)
{
    std::map<uint64_t, uint64_t> by_id;
    bool conflict = false;
    for (size_t i = 0; i < ids.size(); ++i) {
        auto it = by_id.find(ids[i]);
        if (it == by_id.end()) by_id[ids[i]] = keys[i];
        else if (it->second != keys[i]) conflict = true;
    }
    vl::GroupPlan plan;
    uint64_t bad = 0;
    const bool ok = vl::group_plan_build(ids.data(), keys.data(), ids.size(), &plan, &bad);
    EXPECT(ok == !conflict, "%s: built = %d, conflict = %d", what, (int)ok, (int)conflict);
    if (!ok) {
        EXPECT(plan.ids.empty() && plan.dense.empty() && plan.keys.empty(), "%s: a rejected plan is empty", what);
        return;
    }
    std::map<uint64_t, uint32_t> rank;
    for (const auto& kv : by_id) rank[kv.second] = 0;
    uint32_t r = 0;
    for (auto& kv : rank) kv.second = r++;
    EXPECT(plan.ids.size() == by_id.size() && plan.dense.size() == by_id.size(), "%s: %zu ids, want %zu", what, plan.ids.size(), by_id.size());
    EXPECT(plan.keys.size() == rank.size(), "%s: %zu distinct keys, want %zu", what, plan.keys.size(), rank.size());
    size_t i = 0;
    for (const auto& kv : by_id) {  // std::map iterates in ascending id order
        if (i >= plan.ids.size()) break;
        EXPECT(plan.ids[i] == kv.first, "%s: ids[%zu]", what, i);
        EXPECT(plan.dense[i] == rank[kv.second], "%s: dense[%zu] = %u, want %u", what, i, plan.dense[i], rank[kv.second]);
        EXPECT(plan.dense[i] < plan.keys.size() && plan.keys[plan.dense[i]] == kv.second, "%s: keys[dense[%zu]]", what, i);
        ++i;
    }
    for (size_t j = 1; j < plan.ids.size(); ++j) EXPECT(plan.ids[j - 1] < plan.ids[j], "%s: ids ascend strictly at %zu", what, j);
    for (size_t j = 1; j < plan.keys.size(); ++j) EXPECT(plan.keys[j - 1] < plan.keys[j], "%s: keys ascend strictly at %zu", what, j);
}
}  // namespace

int main()
{
    // sorted pairs out of unsorted input
    {
        const std::vector<uint64_t> ids = {30, 10, 20, 40}, keys = {7, 9, 7, 8};
        vl::GroupPlan p;
        EXPECT(vl::group_plan_build(ids.data(), keys.data(), 4, &p), "plain build");
        EXPECT((p.ids == std::vector<uint64_t>{10, 20, 30, 40}), "ids sorted");
        EXPECT((p.keys == std::vector<uint64_t>{7, 8, 9}), "keys distinct, ascending");
        EXPECT((p.dense == std::vector<uint32_t>{2, 0, 0, 1}), "dense numbers follow the sorted ids");
        check_against_map(ids, keys, "plain");
    }
    // random input with repeats: same-key repeats only, then with conflicts mixed in
    std::mt19937_64 rng(20240607);
    for (int round = 0; round < 40; ++round) {
        const size_t n = 1 + rng() % 3000;
        const uint64_t id_space = 1 + rng() % (2 * n), key_space = 1 + rng() % 200;
        std::vector<uint64_t> ids(n), keys(n);
        for (size_t i = 0; i < n; ++i) {
            ids[i] = rng() % id_space;
            keys[i] = (ids[i] * 0x9E3779B97F4A7C15ull >> 17) % key_space;  // a function of the id: repeats agree
        }
        check_against_map(ids, keys, "random, repeats agree");
        if (round % 2) {
            const size_t a = rng() % n;
            ids.push_back(ids[a]);
            keys.push_back(keys[a] + 1);  // the same id with another key
            check_against_map(ids, keys, "random, one conflict");
        }
    }
    // a conflicting repeat is rejected and named; a same-key repeat is accepted
    {
        const std::vector<uint64_t> ids = {5, 6, 5, 9, 6}, keys = {1, 2, 1, 3, 4};
        vl::GroupPlan p;
        uint64_t bad = 0;
        EXPECT(!vl::group_plan_build(ids.data(), keys.data(), 5, &p, &bad), "conflict rejected");
        EXPECT(bad == 6, "the conflicting id is named (%llu)", (unsigned long long)bad);
        EXPECT(!vl::group_plan_build(ids.data(), keys.data(), 5, &p), "conflict rejected without an out pointer");
        const std::vector<uint64_t> ids2 = {5, 6, 5, 5}, keys2 = {1, 2, 1, 1};
        EXPECT(vl::group_plan_build(ids2.data(), keys2.data(), 4, &p), "same-key repeats accepted");
        EXPECT(p.ids.size() == 2 && p.keys.size() == 2, "repeats collapse");
    }
    // n = 0
    {
        vl::GroupPlan p;
        p.ids.push_back(1);
        EXPECT(vl::group_plan_build(nullptr, nullptr, 0, &p), "n = 0 builds");
        EXPECT(p.ids.empty() && p.dense.empty() && p.keys.empty(), "n = 0 is empty");
    }
    // keys 0 and 2^64 - 1, ids 0 and 2^64 - 1
    {
        const std::vector<uint64_t> ids = {~0ull, 0, 17}, keys = {0, ~0ull, 0};
        vl::GroupPlan p;
        EXPECT(vl::group_plan_build(ids.data(), keys.data(), 3, &p), "extreme keys build");
        EXPECT((p.ids == std::vector<uint64_t>{0, 17, ~0ull}), "extreme ids sorted");
        EXPECT((p.keys == std::vector<uint64_t>{0, ~0ull}), "extreme keys kept");
        EXPECT((p.dense == std::vector<uint32_t>{1, 0, 0}), "extreme keys numbered");
        check_against_map(ids, keys, "extremes");
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("group plan ok\n");
    return 0;
}
