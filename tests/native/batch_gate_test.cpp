// csrc/batch_gate.hpp on the CPU (host compiler, ASan + UBSan): over every combination of small domains of the gate's
// inputs, each route's function against that route's condition, restated independently below as one flat expression over
// the index's own names (force_path, n_out_of_domain, mf_env, mfma_min, ...).
#include "../../vectorlite_amd/csrc/batch_gate.hpp"

#include <cstdio>

using namespace vl;

namespace {
constexpr uint64_t MFMA_MIN_ROWS = 8192, KFAST_MAX = 60;  // the limits flat_index.cpp passes (any values serve the comparison)
long failures = 0, checked = 0;
// (`g`, the gate under test, is the enclosing loop's; `extra` names what the site reads beside it)
#define EXPECT_SAME(site, extra, got, want)                                                                                  \
    do {                                                                                                                     \
        ++checked;                                                                                                           \
        if ((got) != (want) && ++failures < 20)                                                                              \
            printf("FAIL %s: got %d, want %d at forced %d, out_of_domain %llu, dim %llu, rows %llu, nq %llu, k_eff %llu, "   \
                   "env_off %d, supported %d, rows_kernel %d, min_batch %llu, extra %llu\n",                                 \
                   site, (int)(got), (int)(want), g.forced_path, (unsigned long long)g.out_of_domain,                        \
                   (unsigned long long)g.dim, (unsigned long long)g.rows, (unsigned long long)g.nq,                          \
                   (unsigned long long)g.k_eff, (int)g.env_off, (int)g.scan_supported, (int)g.rows_kernel,                   \
                   (unsigned long long)g.lim.min_batch, (unsigned long long)(extra));                                        \
    } while (0)
}  // namespace

int main()
{
    const uint64_t rows_v[] = {0, MFMA_MIN_ROWS - 1, MFMA_MIN_ROWS, MFMA_MIN_ROWS + 1, 0x7FFFFFFEull, 0x7FFFFFFFull, 0x80000000ull};
    const uint64_t dim_v[] = {0, 1, 384};
    const uint64_t k_v[] = {1, KFAST_MAX - 1, KFAST_MAX, KFAST_MAX + 1};
    const uint64_t ks_v[] = {1, 10, (1ull << 31) / 3, (1ull << 31) / 2, 1ull << 31};
    for (int force_path = 0; force_path < 2; ++force_path)
    for (uint64_t n_out_of_domain = 0; n_out_of_domain < 2; ++n_out_of_domain)
    for (uint64_t dim_ : dim_v)
    for (uint64_t n : rows_v)
    for (uint64_t nq = 0; nq < 4; ++nq)
    for (uint64_t mfma_min = 2; mfma_min < 4; ++mfma_min)
    for (uint64_t k_eff : k_v)
    for (int env_off = 0; env_off < 2; ++env_off)
    for (int supported = 0; supported < 2; ++supported)
    for (int rows_kernel = 0; rows_kernel < 2; ++rows_kernel) {
        const char* mf_env = env_off ? "0" : nullptr;
        const BatchGate g{force_path, n_out_of_domain, dim_, n, nq, k_eff, env_off != 0, supported != 0, rows_kernel != 0,
                          {MFMA_MIN_ROWS, mfma_min, KFAST_MAX, 2048}};
        // search_batch_locked: `batchable`, then the MFMA condition
        const bool batchable = nq > 1 && force_path == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain == 0;
        const bool mfma_on = !(mf_env && mf_env[0] == '0');
        EXPECT_SAME("search_batch_locked", 0, gate_topk(g), batchable && mfma_on && nq >= mfma_min && n >= MFMA_MIN_ROWS && supported);
        // search_batch_device
        const bool direct = nq > 1 && force_path == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain == 0 &&
                            !(mf_env && mf_env[0] == '0') && nq >= mfma_min && n >= MFMA_MIN_ROWS && supported;
        EXPECT_SAME("search_batch_device", 0, gate_topk(g), direct);
        // search_batch_to_record
        for (uint64_t ks : ks_v)
            EXPECT_SAME("search_batch_to_record", ks, gate_record(g, ks),
                        nq > 1 && force_path == 0 && k_eff <= (uint64_t)KFAST_MAX && n_out_of_domain == 0 &&
                            !(mf_env && mf_env[0] == '0') && nq >= mfma_min && n >= MFMA_MIN_ROWS && supported && nq * ks < (1ull << 31));
        // search_batch_filters, masked block: shp.index_ok
        const bool may_batch = force_path == 0 && n_out_of_domain == 0 && dim_ != 0;
        EXPECT_SAME("search_batch_filters", 0, gate_masked_index(g), may_batch && !(mf_env && mf_env[0] == '0') && supported && rows_kernel);
        // search_mmr_batch and search_grouped_batch: shp.index.index_ok
        const bool tail_ok = force_path == 0 && n_out_of_domain == 0 && dim_ != 0 && !(mf_env && mf_env[0] == '0') && supported;
        EXPECT_SAME("search_mmr_batch", 0, gate_tail_index(g), tail_ok);
        EXPECT_SAME("search_grouped_batch", 0, gate_tail_index(g), tail_ok);
        // search_range_batch (nq = nq_run)
        for (int f = 0; f < 2; ++f)
            EXPECT_SAME("search_range_batch", f, gate_range(g, f != 0),
                        !f && nq >= mfma_min && force_path == 0 && n_out_of_domain == 0 && !(mf_env && mf_env[0] == '0') && supported &&
                            rows_kernel);
        // similarity_join
        for (int join_route = 0; join_route < 3; ++join_route)
        for (int metric = 0; metric < 4; ++metric)
        for (int join_rows = 0; join_rows < 2; ++join_rows)
            EXPECT_SAME("similarity_join", join_route * 100 + metric * 10 + join_rows, gate_join(g, join_route == 1, metric == 0, join_rows != 0),
                        join_route != 1 && metric == 0 && force_path == 0 && n_out_of_domain == 0 && !(mf_env && mf_env[0] == '0') &&
                            join_rows && n < 0x7FFFFFFFull);
    }
    printf("%ld gate decisions checked, %ld failures\n", checked, failures);
    return failures ? 1 : 0;
}
