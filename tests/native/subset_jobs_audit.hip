// Audit of the lists k_scan_subset_jobs writes (test tool, not shipped; driven by tests/test_gpu_subset_jobs_audit.py).
// Ingests one case, runs ONE launch of the jobs scan with the given gx over the case's (query, position list) jobs, merges
// each job's gx lists with the library's k_merge_lists and writes one 64-entry list per job; then, per job, the list of
// k_scan_subset launched alone on the same position list and query, merged the same way.  Every check is made by the
// Python test.
//
//   subset_jobs_audit <case file> <output file>
//
// case file (little endian): u32 magic 'VLSJ', u32 n_metrics, u32 metrics[4], u32 n, u32 dim, u32 nq, u32 n_jobs, u32 gx,
//                            u32 pool_len, f64 rows[n][dim], f64 queries[nq][dim], u32 pool[pool_len],
//                            u32 job[n_jobs][3] = (query, offset into pool, m)
// output file, one block per metric: u32 magic, u32 metric, u32 n_jobs, u32 gx, u32 variant, u32 lone_variant,
//                            f32 key[n_jobs][64], u32 pos[n_jobs][64], f32 lone_key[n_jobs][64], u32 lone_pos[n_jobs][64]
// Status only on stdout; exit status 0 = every stage ran.
#include "../../vectorlite_amd/csrc/kernels.hip"

#include <cstdio>
#include <vector>

using namespace vl;

namespace {

constexpr uint32_t MAGIC = 0x4a534c56u;  // "VLSJ"

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

// n_q groups of n_lists sorted lists (group stride `stride` entries) -> one sorted list per group at out[q * KP], through
// the library's merge level k_merge_lists (at least one pass, so the output is always compact)
void merge_to_one(hipStream_t s, const Cand32* lists, int n_lists, size_t stride, int n_q, Cand32* buf0, Cand32* buf1, Cand32* out)
{
    Cand32* bufs[2] = {buf0, buf1};
    int ping = 0;
    do {
        const int blocks = (n_lists + 63) / 64;
        Cand32* dst = blocks == 1 ? out : bufs[ping];
        hipLaunchKernelGGL((k_merge_lists<float, Cand32>), dim3(blocks, n_q), dim3(1024), 0, s, lists, n_lists, stride, dst,
                           (size_t)blocks * KP);
        CK(hipGetLastError());
        lists = dst;
        stride = (size_t)blocks * KP;
        n_lists = blocks;
        ping ^= 1;
    } while (n_lists > 1);
}

template <typename T>
T* dalloc(size_t count, int fill = 0)
{
    T* p = nullptr;
    CK(hipMalloc(&p, count * sizeof(T) + 256));
    CK(hipMemset(p, fill, count * sizeof(T) + 256));
    return p;
}

void wr(FILE* f, const void* p, size_t bytes)
{
    if (bytes && fwrite(p, 1, bytes, f) != bytes) {
        printf("FAIL short write\n");
        exit(1);
    }
}

void write_lists(FILE* f, const Cand32* d_lists, size_t n_lists)
{
    std::vector<Cand32> lists(n_lists * KP);
    CK(hipMemcpy(lists.data(), d_lists, lists.size() * sizeof(Cand32), hipMemcpyDeviceToHost));
    std::vector<float> keys(lists.size());
    std::vector<uint32_t> pos(lists.size());
    for (size_t i = 0; i < lists.size(); ++i) {
        keys[i] = lists[i].key;
        pos[i] = lists[i].pos;
    }
    wr(f, keys.data(), keys.size() * 4);
    wr(f, pos.data(), pos.size() * 4);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: subset_jobs_audit <case> <out>\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) {
        printf("FAIL cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t hdr[12];
    if (fread(hdr, 4, 12, fi) != 12 || hdr[0] != MAGIC) {
        printf("FAIL bad case header\n");
        return 2;
    }
    const uint32_t n_metrics = hdr[1], n32 = hdr[6], dim = hdr[7], nq = hdr[8], n_jobs = hdr[9], gx = hdr[10], pool_len = hdr[11];
    const uint64_t n = n32;
    if (n_metrics < 1 || n_metrics > 4 || n == 0 || dim == 0 || nq == 0 || n_jobs == 0 || n_jobs > (uint32_t)SCAN_BATCH_MAX_QUERIES ||
        gx == 0 || (uint64_t)gx * n_jobs > PARTIALS32_LISTS || pool_len == 0) {
        printf("FAIL bad case parameters\n");
        return 2;
    }
    std::vector<double> rows(n * dim), qs((size_t)nq * dim);
    std::vector<uint32_t> pool(pool_len), jobs3((size_t)n_jobs * 3);
    if (fread(rows.data(), 8, rows.size(), fi) != rows.size() || fread(qs.data(), 8, qs.size(), fi) != qs.size() ||
        fread(pool.data(), 4, pool.size(), fi) != pool.size() || fread(jobs3.data(), 4, jobs3.size(), fi) != jobs3.size()) {
        printf("FAIL short case file\n");
        return 2;
    }
    fclose(fi);
    // nothing the kernels index with may leave its array: positions below n, job segments inside the pool, queries below nq
    for (uint32_t p : pool)
        if (p >= n32) {
            printf("FAIL position %u past the last row\n", p);
            return 2;
        }
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (jobs3[3 * j] >= nq || jobs3[3 * j + 2] == 0 || (uint64_t)jobs3[3 * j + 1] + jobs3[3 * j + 2] > pool_len) {
            printf("FAIL job %u outside its arrays\n", j);
            return 2;
        }

    const uint32_t ld = (dim + 3u) & ~3u;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    double* d_master = dalloc<double>(n * dim);
    CK(hipMemcpy(d_master, rows.data(), n * dim * 8, hipMemcpyHostToDevice));
    // rows past n are filled with 0x40 bytes (f32 ~3.0), so a scan that lets a row past the end through gives it a large key
    const uint64_t n_alloc = n + 128;
    float* d_slab = dalloc<float>(n_alloc * ld, 0x40);
    float* d_inv = dalloc<float>(n_alloc, 0x40);
    uint8_t* d_flags = dalloc<uint8_t>(n_alloc);
    IngestStats* d_stats = dalloc<IngestStats>(1);
    CK(launch_ingest(s, d_master, d_slab, d_inv, d_flags, d_stats, n, dim, ld));
    IngestStats st{};
    CK(hipMemcpyAsync(&st, d_stats, sizeof st, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (st.n_out_of_domain) {
        printf("FAIL %u rows outside the fast-path domain\n", st.n_out_of_domain);
        return 3;
    }

    uint32_t* d_pool = dalloc<uint32_t>(pool_len);
    CK(hipMemcpy(d_pool, pool.data(), (size_t)pool_len * 4, hipMemcpyHostToDevice));
    // the launch's staging: [n_jobs, dim] queries, then the job table
    std::vector<double> jq((size_t)n_jobs * dim);
    std::vector<SubsetJobDev> table(n_jobs);
    for (uint32_t j = 0; j < n_jobs; ++j) {
        memcpy(jq.data() + (size_t)j * dim, qs.data() + (size_t)jobs3[3 * j] * dim, (size_t)dim * 8);
        table[j].plist = d_pool + jobs3[3 * j + 1];
        table[j].m = jobs3[3 * j + 2];
        table[j].k = table[j].m < 10 ? table[j].m : 10;
    }
    double* d_jq = dalloc<double>(jq.size());
    CK(hipMemcpy(d_jq, jq.data(), jq.size() * 8, hipMemcpyHostToDevice));
    SubsetJobDev* d_table = dalloc<SubsetJobDev>(n_jobs);
    CK(hipMemcpy(d_table, table.data(), table.size() * sizeof(SubsetJobDev), hipMemcpyHostToDevice));

    Cand32* d_part = dalloc<Cand32>(PARTIALS32_ENTRIES);
    Cand32* d_m0 = dalloc<Cand32>((size_t)SCAN_BATCH_QB * SCAN_MAX_GRID);  // a merge level: <= 64 lists of 64 out of 4096, <= 8 jobs
    Cand32* d_m1 = dalloc<Cand32>((size_t)SCAN_BATCH_QB * SCAN_MAX_GRID);
    Cand32* d_lists = dalloc<Cand32>((size_t)n_jobs * KP);
    Cand32* d_lone = dalloc<Cand32>((size_t)n_jobs * KP);
    if (gx > 64 && n_jobs > (uint32_t)SCAN_BATCH_QB) {
        printf("FAIL more than %d jobs take at most 64 lists each\n", SCAN_BATCH_QB);
        return 2;
    }

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) {
        printf("FAIL cannot open %s\n", argv[2]);
        return 2;
    }
    for (uint32_t mi = 0; mi < n_metrics; ++mi) {
        const int metric = (int)hdr[2 + mi];
        ScanPlan plan{};
        CK(launch_scan_subset_jobs(s, metric, d_slab, d_inv, d_table, n_jobs, gx, d_jq, dim, ld, d_part, &plan));
        merge_to_one(s, d_part, (int)gx, (size_t)gx * KP, (int)n_jobs, d_m0, d_m1, d_lists);
        CK(hipStreamSynchronize(s));
        // the yardstick: k_scan_subset alone on each job, its query the way the library hands it over at this stride
        ScanPlan lone{};
        std::vector<float> q32(ld, 0.0f);
        const bool qarg = scan_subset_takes_qarg(ld);
        for (uint32_t j = 0; j < n_jobs; ++j) {
            for (uint32_t c = 0; c < dim; ++c) q32[c] = (float)jq[(size_t)j * dim + c];
            CK(launch_scan_subset(s, metric, d_slab, d_inv, table[j].plist, table[j].m, d_jq + (size_t)j * dim, dim, ld, d_part, &lone,
                                  qarg ? q32.data() : nullptr));
            merge_to_one(s, d_part, lone.grid, (size_t)lone.grid * KP, 1, d_m0, d_m1, d_lone + (size_t)j * KP);
            CK(hipStreamSynchronize(s));  // q32 and the partials are reused by the next job
        }
        const uint32_t oh[6] = {MAGIC, (uint32_t)metric, n_jobs, gx, (uint32_t)plan.variant, (uint32_t)lone.variant};
        wr(fo, oh, sizeof oh);
        write_lists(fo, d_lists, n_jobs);
        write_lists(fo, d_lone, n_jobs);
        printf("metric %d: %u jobs on %u workgroups each, variant %d\n", metric, n_jobs, gx, plan.variant);
    }
    fclose(fo);
    printf("audit ok\n");
    return 0;
}
