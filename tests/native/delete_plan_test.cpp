// CPU check of csrc/delete_plan.hpp: the launch plan of a bulk delete over a sweep of index sizes, bounce capacities and removed
// sets.  Invariants: the segments tile the destinations [r_0, n - m) exactly once, ascending; a direct segment's destinations
// end at or before its first source; a bounced segment fits the bounce; the recorded shifts are the true ones.  Every plan is
// then executed on a host array, the rows of one launch applied in forward, reverse and shuffled order (a launch's workgroups
// run in any order: that is the adversary of the hazard rule), and the outcome must equal std::remove_if.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../vectorlite_amd/csrc/delete_plan.hpp"

namespace {

std::string g_case;
uint64_t g_n, g_cap;

#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            std::printf("FAILED %s  (%s, n %llu, bounce rows %llu)\n", #c, g_case.c_str(), (unsigned long long)g_n,   \
                        (unsigned long long)g_cap);                                                                    \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

enum Order { FORWARD, REVERSE, SHUFFLED };

// runs the plan on `rows` as the device would: a direct launch writes in place, its rows in the given order; a bounced
// segment is gathered (same orders) and copied down
void execute(std::vector<uint32_t>& rows, const std::vector<vl::DeleteSegment>& plan, const std::vector<uint32_t>& keys,
             uint64_t cap, Order order, std::mt19937_64& rng)
{
    std::vector<uint32_t> bounce(cap, 0xDEADBEEFu);
    for (const vl::DeleteSegment& s : plan) {
        std::vector<uint64_t> ds(s.dst_end - s.dst_begin);
        std::iota(ds.begin(), ds.end(), s.dst_begin);
        if (order == REVERSE) std::reverse(ds.begin(), ds.end());
        if (order == SHUFFLED) std::shuffle(ds.begin(), ds.end(), rng);
        for (uint64_t d : ds) {
            const uint32_t v = rows[d + vl::delete_shift(keys, d)];
            if (s.direct) rows[d] = v;
            else bounce[d - s.dst_begin] = v;
        }
        if (!s.direct) std::copy(bounce.begin(), bounce.begin() + (s.dst_end - s.dst_begin), rows.begin() + s.dst_begin);
    }
}

int check_one(const std::string& name, uint64_t n, const std::vector<uint64_t>& removed, uint64_t cap, long* plans,
              long* n_direct, long* n_bounced)
{
    g_case = name;
    g_n = n;
    g_cap = cap;
    const uint64_t m = removed.size();
    const std::vector<uint32_t> keys = vl::delete_keys(removed);
    const std::vector<vl::DeleteSegment> plan = vl::delete_plan(n, keys, cap);
    // the shift is what the definition says: removed rows in front of the source
    for (uint64_t d = 0; d < n - m; d += std::max<uint64_t>(1, (n - m) / 97)) {
        const uint64_t s = d + vl::delete_shift(keys, d);
        CHECK(s < n && !std::binary_search(removed.begin(), removed.end(), s));
        CHECK((uint64_t)(std::lower_bound(removed.begin(), removed.end(), s) - removed.begin()) == s - d);
    }
    if (m == 0 || m == n) {
        CHECK(plan.empty());
    } else {
        // tiles [r_0, n - m) exactly once, ascending
        uint64_t at = removed[0];
        for (const vl::DeleteSegment& s : plan) {
            CHECK(s.dst_begin == at && s.dst_end > s.dst_begin);
            at = s.dst_end;
            CHECK(s.shift_begin == vl::delete_shift(keys, s.dst_begin) && s.shift_begin >= 1);
            CHECK(s.shift_end == vl::delete_shift(keys, s.dst_end - 1) && s.shift_end >= s.shift_begin);
            if (s.direct) CHECK(s.dst_end <= s.dst_begin + s.shift_begin);  // destination end <= source start
            else CHECK(s.dst_end - s.dst_begin <= cap);                     // fits the bounce
            if (s.dst_end - s.dst_begin <= s.shift_begin) CHECK(s.direct);  // never two copies where one is safe
            ++(s.direct ? *n_direct : *n_bounced);
        }
        CHECK(at == n - m);
        if (removed[0] == n - m) CHECK(plan.empty());  // only a tail went: nothing moves
    }
    // execution against std::remove_if
    std::vector<uint32_t> want(n);
    for (uint64_t i = 0; i < n; ++i) want[i] = (uint32_t)(i * 2654435761u + 12345u);
    const std::vector<uint32_t> orig = want;
    {
        size_t ri = 0, w = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (ri < removed.size() && removed[ri] == i) ++ri;
            else want[w++] = orig[i];
        }
        want.resize(w);
        std::vector<uint32_t> lib = orig;  // the same through the standard algorithm
        std::vector<uint8_t> gone(n, 0);
        for (uint64_t r : removed) gone[r] = 1;
        size_t idx = 0;
        lib.erase(std::remove_if(lib.begin(), lib.end(), [&](uint32_t) { return gone[idx++] != 0; }), lib.end());
        CHECK(lib == want);
    }
    std::mt19937_64 rng(n * 1000003 + cap);
    for (Order o : {FORWARD, REVERSE, SHUFFLED}) {
        std::vector<uint32_t> rows = orig;
        execute(rows, plan, keys, cap, o, rng);
        rows.resize(n - m);
        CHECK(rows == want);
    }
    ++*plans;
    return 0;
}

std::vector<uint64_t> random_set(uint64_t n, double frac, uint64_t seed)
{
    std::vector<uint64_t> all(n);
    std::iota(all.begin(), all.end(), 0);
    std::mt19937_64 rng(seed);
    std::shuffle(all.begin(), all.end(), rng);
    all.resize((size_t)std::min<double>((double)n, std::max(1.0, frac * (double)n)));
    std::sort(all.begin(), all.end());
    return all;
}

}  // namespace

int main()
{
    long plans = 0, n_direct = 0, n_bounced = 0;
    const uint64_t sizes[] = {1, 2, 3, 17, 64, 257, 1000, 3000, 4099};
    const uint64_t caps[] = {1, 2, 3, 7, 20, 64, 333, 1024, 5000, 1u << 20};
    for (uint64_t n : sizes)
        for (uint64_t cap : caps) {
            std::vector<std::pair<std::string, std::vector<uint64_t>>> sets;
            sets.push_back({"none", {}});
            sets.push_back({"first", {0}});
            sets.push_back({"last", {n - 1}});
            sets.push_back({"middle", {n / 2}});
            {
                std::vector<uint64_t> r;
                for (uint64_t i = 0; i < n; i += 2) r.push_back(i);
                sets.push_back({"every other (even)", r});
                r.clear();
                for (uint64_t i = 1; i < n; i += 2) r.push_back(i);
                sets.push_back({"every other (odd)", r});
            }
            {
                std::vector<uint64_t> r;
                for (uint64_t i = n / 5; i < n / 5 + std::max<uint64_t>(1, n / 3); ++i) r.push_back(i);
                sets.push_back({"one long run", r});
                r.clear();
                for (uint64_t i = 0; i < n / 2; ++i) r.push_back(i);
                sets.push_back({"front half", r});
                r.clear();
                for (uint64_t i = 0; i < n; ++i) r.push_back(i);
                sets.push_back({"all", r});
            }
            for (double f : {0.01, 0.10, 0.50, 0.99})
                sets.push_back({"random " + std::to_string(f), random_set(n, f, (uint64_t)(f * 100) + n)});
            for (auto& s : sets) {
                if (!s.second.empty() && s.second.back() >= n) continue;
                if (check_one(s.first, n, s.second, cap, &plans, &n_direct, &n_bounced)) return 1;
            }
            // named shapes
            g_n = n;
            g_cap = cap;
            if (n >= 3) {
                // one hole at row 0: every row moves up by one, so no launch of two rows or more may write in place -- all
                // bounce, in chunks of the bounce's size.  (A segment of ONE row -- the bounce holds one row, or one row is
                // left over at the end -- has no second row to race with: b - a <= shift(a) = 1 holds and it moves in place.)
                g_case = "hole at row 0";
                const auto plan = vl::delete_plan(n, vl::delete_keys({0}), cap);
                CHECK(plan.size() == (n - 1 + cap - 1) / cap);
                for (const auto& s : plan) {
                    CHECK(s.dst_end - s.dst_begin <= cap);
                    CHECK(s.direct == (s.dst_end - s.dst_begin == 1));
                }
            }
            if (n >= 2 && n % 2 == 0) {
                // n/2 removals at the front: everything is direct, in one launch, whatever the bounce holds
                g_case = "front half";
                std::vector<uint64_t> r;
                for (uint64_t i = 0; i < n / 2; ++i) r.push_back(i);
                const auto plan = vl::delete_plan(n, vl::delete_keys(r), cap);
                CHECK(plan.size() == 1 && plan[0].direct && plan[0].dst_begin == 0 && plan[0].dst_end == n / 2);
            }
        }
    if (n_direct == 0 || n_bounced == 0) {
        std::printf("FAILED: the sweep must see both kinds of segment (%ld direct, %ld bounced)\n", n_direct, n_bounced);
        return 1;
    }
    std::printf("%ld plans checked (%ld direct launches, %ld bounced segments)\n", plans, n_direct, n_bounced);
    return 0;
}
