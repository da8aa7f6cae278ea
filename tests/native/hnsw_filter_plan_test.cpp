// vectorlite_amd/csrc/hnsw_filter_plan.hpp on the CPU (stand-alone, run under ASan + UBSan by
// tests/test_hnsw_filter_plan_cpu.py): the route and the list capacity of an id-filtered HNSW search at every boundary.
//   - n_pass = 0 (exact, zero candidates) and n_pass = 1;
//   - ef_walk from ef, from min(k, n_pass) and from the opt-in floor; ef_walk = 512 walks, 513 does not;
//   - both sides of ef_walk * n_nodes > 256 * n_pass;
//   - cap at each step of 64 / 128 / 256 / 512, from ef_walk alone and from ceil(2 * ef_walk * n_nodes / n_pass);
//   - products beyond 2^64; and a sweep of a small domain against the rule restated in plain 64-bit arithmetic.
#include "../../vectorlite_amd/csrc/hnsw_filter_plan.hpp"

#include <cstdio>

namespace {
int failures = 0;

void expect(const char* what, uint64_t k, uint32_t ef, uint32_t min_beam, uint64_t n, uint64_t n_pass, int route, uint32_t cap,
            uint64_t max_candidates, uint64_t ef_walk)
{
    const vl::HnswFilterPlan p = vl::hnsw_filter_plan(k, ef, min_beam, n, n_pass);
    const bool ok = p.route == route && (route == 1 || p.cap == cap) && p.max_candidates == max_candidates && p.ef_walk == ef_walk;
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: route %d cap %u max_candidates %llu ef_walk %llu\n", what, p.route, p.cap,
                    (unsigned long long)p.max_candidates, (unsigned long long)p.ef_walk);
    }
}
}  // namespace

int main()
{
    // n_pass 0 and 1
    expect("no passing node", 10, 32, 0, 1000, 0, 1, 0, 0, 32);
    expect("one passing node of one", 10, 0, 0, 1, 1, 0, 64, 1, 1);
    expect("one passing node of 256, strict beam", 10, 0, 0, 256, 1, 0, 512, 1, 1);  // 1 * 256 > 256 * 1 is false
    expect("one passing node of 257, strict beam", 10, 0, 0, 257, 1, 1, 0, 1, 1);
    expect("k = 0", 0, 0, 0, 100, 50, 1, 0, 0, 0);
    // where ef_walk comes from
    expect("ef below min(k, n_pass)", 40, 10, 0, 1000, 1000, 0, 128, 40, 40);
    expect("ef above min(k, n_pass)", 10, 100, 0, 1000, 1000, 0, 256, 10, 100);
    expect("the floor counts only without ef", 10, 0, 32, 1000, 1000, 0, 64, 10, 32);
    expect("an explicit ef ignores the floor", 10, 12, 32, 1000, 1000, 0, 64, 10, 12);
    expect("n_pass caps the candidates", 100, 0, 0, 1000, 7, 1, 0, 7, 7);  // 7 * 1000 > 256 * 7
    // 512 / 513
    expect("ef_walk 512", 512, 0, 0, 4096, 4096, 1, 0, 512, 512);       // 512 * 4096 > 256 * 4096: all-pass still too wide
    expect("ef 512 all-pass", 10, 512, 0, 4096, 4096, 1, 0, 10, 512);
    expect("ef_walk 513", 513, 0, 0, 4096, 4096, 1, 0, 513, 513);
    expect("ef_walk 256 all-pass walks", 10, 256, 0, 4096, 4096, 0, 512, 10, 256);
    expect("ef_walk 257 all-pass does not", 10, 257, 0, 4096, 4096, 1, 0, 10, 257);
    // both sides of the 256 rule: ef 32, n 8000 -> n_pass >= 1000 walks
    expect("on the boundary", 10, 32, 0, 8000, 1000, 0, 512, 10, 32);
    expect("one below the boundary", 10, 32, 0, 8000, 999, 1, 0, 10, 32);
    // cap steps: need = max(ef, ceil(2 ef n / n_pass))
    expect("cap 64 from the ratio", 10, 32, 0, 1000, 1000, 0, 64, 10, 32);      // 64
    expect("cap 128 one past 64", 10, 32, 0, 1000, 999, 0, 128, 10, 32);        // ceil(64000 / 999) = 65
    expect("cap 128 at 128", 10, 32, 0, 1000, 500, 0, 128, 10, 32);
    expect("cap 256 one past 128", 10, 32, 0, 1000, 499, 0, 256, 10, 32);
    expect("cap 256 at 256", 10, 32, 0, 1000, 250, 0, 256, 10, 32);
    expect("cap 512 one past 256", 10, 32, 0, 1000, 249, 0, 512, 10, 32);
    expect("cap 512 at 512", 10, 32, 0, 1000, 125, 0, 512, 10, 32);
    expect("past 512 is the exact route", 10, 32, 0, 1000, 124, 1, 0, 10, 32);
    expect("cap 64 at ef 1", 1, 1, 0, 3000, 3000, 0, 64, 1, 1);
    // products beyond 2^64: ef_walk * n_nodes = 512 * 2^62 = 2^71
    const uint64_t big = 1ull << 62;
    expect("2^71 against 2^70: walk", 10, 256, 0, big, big, 0, 512, 10, 256);
    expect("2^71 against 2^70 + 2^62: exact", 10, 257, 0, big, big, 1, 0, 10, 257);
    expect("n_pass = n / 2 at 2^62", 10, 128, 0, big, big / 2, 0, 512, 10, 128);
    expect("n_pass = n / 2 - 1 at 2^62", 10, 128, 0, big, big / 2 - 1, 1, 0, 10, 128);
    expect("all 64-bit ones", ~0ull, 0, 0, ~0ull, ~0ull, 1, 0, ~0ull, ~0ull);
    expect("n at 2^64 - 1, ef 1", 1, 1, 0, ~0ull, ~0ull, 0, 64, 1, 1);
    expect("n at 2^64 - 1, a 256th passes", 1, 1, 0, ~0ull, (~0ull) / 256 + 1, 0, 512, 1, 1);
    expect("n at 2^64 - 1, just under a 256th", 1, 1, 0, ~0ull, (~0ull) / 256, 1, 0, 1, 1);

    // a small domain against the rule restated in plain 64-bit arithmetic (nothing wraps at these sizes)
    for (uint64_t n = 1; n <= 600 && !failures; n += 7)
        for (uint64_t np = 0; np <= n; np += (n > 40 ? n / 13 : 1))
            for (uint32_t ef = 0; ef <= 520; ef += 13)
                for (uint64_t k = 0; k <= 20; k += 5) {
                    const vl::HnswFilterPlan p = vl::hnsw_filter_plan(k, ef, 3, n, np);
                    const uint64_t mc = k < np ? k : np;
                    const uint64_t fl = ef ? ef : 3;
                    const uint64_t ew = mc > fl ? mc : fl;
                    int route = 0;
                    uint32_t cap = 0;
                    if (np == 0 || ew > 512 || ew * n > 256 * np) route = 1;
                    else {
                        uint64_t need = (2 * ew * n + np - 1) / np;
                        if (need < ew) need = ew;
                        cap = need <= 64 ? 64 : need <= 128 ? 128 : need <= 256 ? 256 : 512;
                    }
                    if (p.route != route || (route == 0 && p.cap != cap) || p.max_candidates != mc || p.ef_walk != ew) {
                        ++failures;
                        std::printf("FAIL sweep n %llu n_pass %llu ef %u k %llu\n", (unsigned long long)n, (unsigned long long)np, ef,
                                    (unsigned long long)k);
                    }
                }
    if (failures) return 1;
    std::printf("hnsw filter plan ok\n");
    return 0;
}
