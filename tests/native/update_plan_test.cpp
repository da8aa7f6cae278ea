// update_plan_test.cpp -- csrc/update_plan.hpp on the CPU (tests/test_update_plan_cpu.py builds this with AddressSanitizer and
// UBSan).  Random position -> id tables, some with duplicate-id rows; id lists with repeats and absent ids; both values of
// insert_missing.  Every plan is applied to a host mirror (one f64 "value" per row: the list index it came from) and must
// leave exactly what the sequential loop `contains(id) ? update(first row with id) : (insert_missing ? add : fail)` leaves;
// positions strictly ascending, one per distinct position; chunks tile the positions and fit the staging size; a refusal
// names the loop's failing id and plans nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../vectorlite_amd/csrc/update_plan.hpp"

namespace {

struct Mirror {
    std::vector<uint64_t> ids;
    std::vector<double> val;
};

[[noreturn]] void fail(const char* what, int trial)
{
    std::fprintf(stderr, "FAIL (trial %d): %s\n", trial, what);
    std::exit(1);
}

// the contract, literally; false + *bad: the loop's failure (the mirror is then discarded by the caller)
bool run_loop(Mirror& mi, const std::vector<uint64_t>& ids, bool insert_missing, uint64_t* bad)
{
    for (size_t i = 0; i < ids.size(); ++i) {
        size_t p = 0;
        while (p < mi.ids.size() && mi.ids[p] != ids[i]) ++p;
        if (p < mi.ids.size()) {
            mi.val[p] = 1000.0 + (double)i;
        } else if (insert_missing) {
            mi.ids.push_back(ids[i]);
            mi.val.push_back(1000.0 + (double)i);
        } else {
            *bad = ids[i];
            return false;
        }
    }
    return true;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240607);
    uint64_t plans = 0, refusals = 0, appended = 0, chunk_checks = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        const uint64_t rows = rng() % 4 == 0 ? rng() % 4 : rng() % 300;
        const uint64_t id_space = 1 + rng() % (rows + 40);  // small spaces: duplicate-id rows in the table
        Mirror before;
        for (uint64_t p = 0; p < rows; ++p) {
            uint64_t id = rng() % id_space;
            if (rng() % 97 == 0) id = ~0ull;  // the largest id is an id like any other
            before.ids.push_back(id);
            before.val.push_back((double)p);
        }
        const uint64_t n = rng() % 5 == 0 ? rng() % 3 : rng() % 200;
        const int flavour = (int)(rng() % 3);  // 0: listed ids mostly present, 1: a mix, 2: mostly absent
        std::vector<uint64_t> ids;
        for (uint64_t i = 0; i < n; ++i) {
            const bool present = rows && (flavour == 0 ? rng() % 50 != 0 : flavour == 1 ? rng() % 2 : rng() % 8 == 0);
            uint64_t id = present ? before.ids[rng() % rows] : id_space + rng() % 30;
            if (!ids.empty() && rng() % 6 == 0) id = ids[rng() % ids.size()];  // repeats
            if (rng() % 211 == 0) id = ~0ull;
            ids.push_back(id);
        }
        for (int im = 0; im < 2; ++im) {
            const bool insert_missing = im != 0;
            Mirror want = before;
            uint64_t bad = 0;
            const bool ok = run_loop(want, ids, insert_missing, &bad);
            const vl::UpdatePlan plan = vl::update_plan(before.ids.data(), rows, ids.data(), n, insert_missing);
            ++plans;
            if (!ok) {
                ++refusals;
                if (!plan.refused) fail("the loop fails but the plan does not refuse", trial);
                if (plan.missing_id != bad) fail("the refusal names another id than the loop's", trial);
                if (!plan.pos.empty() || !plan.src.empty() || !plan.append_ids.empty() || !plan.append_src.empty())
                    fail("a refusal left something planned", trial);
                continue;
            }
            if (plan.refused) fail("the plan refuses a list the loop accepts", trial);
            if (plan.pos.size() != plan.src.size() || plan.append_ids.size() != plan.append_src.size())
                fail("list lengths differ", trial);
            for (size_t j = 0; j < plan.pos.size(); ++j) {
                if (plan.pos[j] >= rows) fail("a position beyond the table", trial);
                if (j && plan.pos[j] <= plan.pos[j - 1]) fail("positions not strictly ascending", trial);
                if (plan.src[j] >= n) fail("a source beyond the list", trial);
            }
            Mirror got = before;
            for (size_t j = 0; j < plan.pos.size(); ++j) got.val[plan.pos[j]] = 1000.0 + (double)plan.src[j];
            for (size_t j = 0; j < plan.append_ids.size(); ++j) {
                if (plan.append_src[j] >= n) fail("an appended source beyond the list", trial);
                got.ids.push_back(plan.append_ids[j]);
                got.val.push_back(1000.0 + (double)plan.append_src[j]);
            }
            appended += plan.append_ids.size();
            if (got.ids != want.ids) fail("ids differ from the sequential loop's", trial);
            if (got.val != want.val) fail("values differ from the sequential loop's", trial);
            if (!insert_missing && !plan.append_ids.empty()) fail("rows appended without insert_missing", trial);

            // the staging cut: for a few dims and buffer sizes, chunks tile [0, m) in order and fit the buffer
            const uint64_t m = plan.pos.size();
            const uint64_t dims[] = {1, 3, 64, 100, 384};
            for (uint64_t dim : dims) {
                const uint64_t sizes[] = {0, 1, dim * 8, 2 * (dim * 8 + 5) + 48 + 1, 5000, 1ull << 20};
                for (uint64_t bytes : sizes) {
                    const uint64_t sr = vl::update_stage_rows(bytes, dim);
                    if (sr < 1) fail("a staging buffer of no rows", trial);
                    if (sr > 1 && vl::update_stage_bytes(sr, dim) > bytes) fail("the staged rows do not fit the buffer", trial);
                    if (vl::update_stage_pos_offset(sr, dim) < sr * dim * 8 || vl::update_stage_pos_offset(sr, dim) % 16 ||
                        vl::update_stage_flag_offset(sr, dim) < vl::update_stage_pos_offset(sr, dim) + sr * 4 ||
                        vl::update_stage_bytes(sr, dim) < vl::update_stage_flag_offset(sr, dim) + sr)
                        fail("the staging arrays overlap", trial);
                    uint64_t at = 0;
                    for (const auto& c : vl::update_chunks(m, sr)) {
                        if (c.first != at || c.second <= c.first || c.second - c.first > sr) fail("a chunk is out of place or too long", trial);
                        at = c.second;
                    }
                    if (at != m) fail("the chunks do not cover the positions", trial);
                    ++chunk_checks;
                }
            }
            if (vl::update_stage_rows(2 * (384 * 8 + 5) + 48 + 1, 384) != 2) fail("the two-row staging size does not hold two rows", trial);
        }
    }
    if (refusals < 100 || appended < 1000) fail("the generator did not reach refusals and appends", -1);
    std::printf("%llu plans checked (%llu refusals, %llu rows appended, %llu staging cuts)\n", (unsigned long long)plans,
                (unsigned long long)refusals, (unsigned long long)appended, (unsigned long long)chunk_checks);
    return 0;
}
