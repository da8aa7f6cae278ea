// Audit of the candidate filters against the exactness bound (test tool, not shipped; driven by
// tests/test_gpu_filter_audit.py).  Runs the library's own stages on one case and writes, per metric and query, the filter's
// 64-entry candidate list, the shipped bound_for_key<METRIC> evaluated on the device for the list's 64th key and for every
// listed key, and the reference f64 score of every row.  Every check is made by the Python test.
//
//   filter_audit <case file> <output file>
//
// case file (little endian): u32 magic 'VLFA', u32 filter, u32 n_metrics, u32 metrics[4], u32 n, u32 dim, u32 nq,
//                            f64 rows[n][dim], f64 queries[nq][dim]
// output file, one block per metric: u32 magic, u32 metric, u32 nq, u32 n, u32 ld, u32 info[4], f64 R, f64 in_extra,
//                            f64 Q[nq], f32 key[nq][64], u32 pos[nq][64], f64 B_t64[nq], f64 B_key[nq][64], f64 exact[nq][n]
// Status only on stdout; exit status 0 = every stage ran.
#include "../../vectorlite_amd/csrc/kernels.hip"
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"

#include <cstdio>
#include <vector>

using namespace vl;

namespace {

enum Filter : uint32_t { F32_QARG = 0, F32_Q64 = 1, F32_BATCH = 2, BF16_SINGLE = 3, MFMA_BATCH = 4 };
constexpr uint32_t MAGIC = 0x41464c56u;  // "VLFA"

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

// B(t64) of every list and B(key) of every entry, with the library's own bound function
template <int METRIC>
__global__ void k_audit_bounds(const Cand32* __restrict__ lists, uint32_t nq, uint32_t ld, double R,
                               const double* __restrict__ q_norms, double in_extra, double* __restrict__ b_t64,
                               double* __restrict__ b_key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * (uint32_t)KP) return;
    const uint32_t q = i / KP;
    b_key[i] = bound_for_key<METRIC>(lists[i].key, ld, R, q_norms[q], in_extra);
    if (i % KP == 0) b_t64[q] = bound_for_key<METRIC>(lists[(size_t)q * KP + KP - 1].key, ld, R, q_norms[q], in_extra);
}

// nq groups of n_lists sorted lists (query stride `stride` entries) -> one sorted list per query at out[q * KP], through the
// library's merge level k_merge_lists (at least one pass, so the output is always compact)
void merge_to_one(hipStream_t s, const Cand32* lists, int n_lists, size_t stride, int nq, Cand32* buf0, Cand32* buf1,
                  Cand32* out)
{
    Cand32* bufs[2] = {buf0, buf1};
    int ping = 0;
    do {
        const int blocks = (n_lists + 63) / 64;
        Cand32* dst = blocks == 1 ? out : bufs[ping];
        hipLaunchKernelGGL((k_merge_lists<float, Cand32>), dim3(blocks, nq), dim3(1024), 0, s, lists, n_lists, stride, dst,
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

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: filter_audit <case> <out>\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) {
        printf("FAIL cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t hdr[10];
    if (fread(hdr, 4, 10, fi) != 10 || hdr[0] != MAGIC) {
        printf("FAIL bad case header\n");
        return 2;
    }
    const uint32_t filter = hdr[1], n_metrics = hdr[2], n32 = hdr[7], dim = hdr[8], nq = hdr[9];
    const uint64_t n = n32;
    if (filter > MFMA_BATCH || n_metrics < 1 || n_metrics > 4 || n == 0 || dim == 0 || nq == 0 || nq > MFMA_MAX_BATCH) {
        printf("FAIL bad case parameters\n");
        return 2;
    }
    std::vector<double> rows(n * dim), qs((size_t)nq * dim + nq);
    if (fread(rows.data(), 8, rows.size(), fi) != rows.size() || fread(qs.data(), 8, (size_t)nq * dim, fi) != (size_t)nq * dim) {
        printf("FAIL short case file\n");
        return 2;
    }
    fclose(fi);
    // query norms: sequential sum of squares, as the host stages a single query (flat_index.cpp)
    for (uint32_t q = 0; q < nq; ++q) {
        double ss = 0.0;
        for (uint32_t c = 0; c < dim; ++c) ss += qs[(size_t)q * dim + c] * qs[(size_t)q * dim + c];
        qs[(size_t)nq * dim + q] = sqrt(ss);
    }

    const uint32_t ld = (dim + 3u) & ~3u;  // the slab stride, and the n of every bound (rank_check_emit)
    const uint32_t ldb = mfma_ldb(dim);
    // every per-row buffer is allocated in whole 64-row tiles plus one more tile; the rows past n are filled with
    // 0x40 bytes (f32 / bf16 ~3.0), so a filter that lets a row past the end through gives it a large key
    const uint64_t n_alloc = (n + 2 * MFMA_TILE_ROWS - 1) / MFMA_TILE_ROWS * MFMA_TILE_ROWS;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    double* d_master = dalloc<double>(n * dim);
    CK(hipMemcpy(d_master, rows.data(), n * dim * 8, hipMemcpyHostToDevice));
    double* d_q = dalloc<double>(qs.size());
    CK(hipMemcpy(d_q, qs.data(), qs.size() * 8, hipMemcpyHostToDevice));
    const double* d_qn = d_q + (size_t)nq * dim;

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
    double R;
    memcpy(&R, &st.max_norm_bits, 8);

    void* d_slab16 = nullptr;
    float* d_nrm16 = nullptr;
    float* d_sqn16 = nullptr;
    const bool frag = filter == MFMA_BATCH && mfma_rows_kernel(dim);
    if (filter == BF16_SINGLE || filter == MFMA_BATCH) {
        d_slab16 = dalloc<uint16_t>(n_alloc * ldb, 0x40);
        d_nrm16 = dalloc<float>(n_alloc, 0x40);
        d_sqn16 = dalloc<float>(n_alloc, 0x40);
        if (frag) CK(launch_rows_bf16_frag(s, d_master, 0, n, dim, d_slab16, d_nrm16, d_sqn16));
        else CK(launch_rows_bf16(s, d_master, n, dim, d_slab16, d_nrm16, d_sqn16));
    }

    const size_t part_entries = PARTIALS32_ENTRIES;
    Cand32* d_part = dalloc<Cand32>(part_entries);
    Cand32* d_m0 = dalloc<Cand32>((size_t)nq * SCAN_MAX_GRID);  // merge levels: <= 64 lists of 64 per query out of 4096
    Cand32* d_m1 = dalloc<Cand32>((size_t)nq * SCAN_MAX_GRID);
    Cand32* d_lists = dalloc<Cand32>((size_t)nq * KP);
    double* d_bt = dalloc<double>(nq);
    double* d_bk = dalloc<double>((size_t)nq * KP);
    double* d_exact = dalloc<double>(n * nq);
    uint32_t* d_nan = dalloc<uint32_t>(1);
    MfmaScratch w;
    if (filter == MFMA_BATCH) {
        w.nq_cap = nq;
        w.nq_pad_cap = nq + 256;
        w.q_bf16 = dalloc<uint16_t>((size_t)w.nq_pad_cap * ldb);
        w.gmax = dalloc<int>((size_t)w.nq_pad_cap * MFMA_GROUPS);
        w.thr = dalloc<float>(w.nq_pad_cap);
        w.cand = dalloc<Cand32>((size_t)w.nq_pad_cap * MFMA_CAND_CAP);
        w.cnt = dalloc<uint32_t>(w.nq_pad_cap);
    }

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) {
        printf("FAIL cannot open %s\n", argv[2]);
        return 2;
    }
    for (uint32_t mi = 0; mi < n_metrics; ++mi) {
        const int metric = (int)hdr[3 + mi];
        uint32_t info[4] = {0, 0, 0, 0};
        double in_extra = 0.0;
        if (filter == F32_QARG || filter == F32_Q64) {
            if (filter == F32_QARG && !scan_takes_qarg(ld)) {
                printf("FAIL stride %u has no kernel-argument query\n", ld);
                return 2;
            }
            std::vector<float> q32(ld, 0.0f);
            for (uint32_t q = 0; q < nq; ++q) {
                for (uint32_t c = 0; c < dim; ++c) q32[c] = (float)qs[(size_t)q * dim + c];
                ScanPlan plan{};
                CK(launch_scan(s, metric, d_slab, d_inv, d_q + (size_t)q * dim, n, dim, ld, d_part, &plan,
                               filter == F32_QARG ? q32.data() : nullptr));
                merge_to_one(s, d_part, plan.grid, (size_t)plan.grid * KP, 1, d_m0, d_m1, d_lists + (size_t)q * KP);
                info[0] = (uint32_t)plan.grid;
                info[1] = (uint32_t)plan.variant;
                CK(hipStreamSynchronize(s));  // q32 and the partials are reused by the next query
            }
        } else if (filter == F32_BATCH) {
            if (!scan_batch_supported(ld) || nq > (uint32_t)SCAN_BATCH_MAX_QUERIES) {
                printf("FAIL no batch scan for stride %u / %u queries\n", ld, nq);
                return 2;
            }
            ScanPlan plan{};
            CK(launch_scan_batch(s, metric, d_slab, d_inv, d_q, nq, n, dim, ld, d_part, &plan));
            merge_to_one(s, d_part, plan.grid, (size_t)plan.grid * KP, (int)nq, d_m0, d_m1, d_lists);
            info[0] = (uint32_t)plan.grid;
            // lanes per row of the shape that ran: the first one of the library's list whose G * VPL is the stride
#define VL_AUDIT_G(G, VPL) \
    if (info[1] == 0 && (uint32_t)(G * VPL) == ld / 4) info[1] = G;
            VL_BATCH_SHAPES(VL_AUDIT_G)
#undef VL_AUDIT_G
        } else if (filter == BF16_SINGLE) {
            if (!scan_bf16_supported(dim, metric)) {
                printf("FAIL no bf16 scan for dim %u metric %d\n", dim, metric);
                return 2;
            }
            in_extra = IN_EXTRA_BF16_SINGLE;
            for (uint32_t q = 0; q < nq; ++q) {
                int grid = 0;
                CK(launch_scan_bf16(s, metric, d_slab16, d_nrm16, d_sqn16, d_q + (size_t)q * dim, n, dim, d_part, &grid));
                merge_to_one(s, d_part, grid, (size_t)grid * KP, 1, d_m0, d_m1, d_lists + (size_t)q * KP);
                info[0] = (uint32_t)grid;
                CK(hipStreamSynchronize(s));
            }
        } else {
            if (!mfma_scan_supported(dim, metric) || n < MFMA_MIN_ROWS) {
                printf("FAIL no MFMA filter for dim %u metric %d rows %llu\n", dim, metric, (unsigned long long)n);
                return 2;
            }
            in_extra = IN_EXTRA_MFMA;
            // the filter's q64 layout: [nq, dim] queries followed by their [nq] norms
            MfmaLaunchInfo li;
            CK(launch_mfma_candidates(s, metric, d_slab16, d_nrm16, d_sqn16, d_q, nq, n, dim, w, d_lists, &li));
            info[0] = (uint32_t)li.ksteps;
            info[1] = (uint32_t)li.chunks;
            info[2] = (uint32_t)li.stages;
            info[3] = frag ? 1u : 0u;
        }
        CK(dispatch_metric(metric, [&](auto M) -> hipError_t {
            constexpr int MM = decltype(M)::value;
            hipLaunchKernelGGL((k_audit_bounds<MM>), dim3((nq * KP + 255) / 256), dim3(256), 0, s, d_lists, nq, ld, R, d_qn,
                               in_extra, d_bt, d_bk);
            return hipGetLastError();
        }));
        for (uint32_t q = 0; q < nq; ++q)
            CK(launch_exact_scan(s, metric, d_master, d_q + (size_t)q * dim, n, dim, d_exact + (size_t)q * n, d_nan));
        CK(hipStreamSynchronize(s));

        std::vector<Cand32> lists((size_t)nq * KP);
        std::vector<double> bt(nq), bk((size_t)nq * KP), exact(n * nq);
        CK(hipMemcpy(lists.data(), d_lists, lists.size() * sizeof(Cand32), hipMemcpyDeviceToHost));
        CK(hipMemcpy(bt.data(), d_bt, nq * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(bk.data(), d_bk, bk.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(exact.data(), d_exact, exact.size() * 8, hipMemcpyDeviceToHost));
        std::vector<float> keys(lists.size());
        std::vector<uint32_t> pos(lists.size());
        for (size_t i = 0; i < lists.size(); ++i) {
            keys[i] = lists[i].key;
            pos[i] = lists[i].pos;
        }
        const uint32_t oh[9] = {MAGIC, (uint32_t)metric, nq, n32, ld, info[0], info[1], info[2], info[3]};
        wr(fo, oh, sizeof oh);
        wr(fo, &R, 8);
        wr(fo, &in_extra, 8);
        wr(fo, qs.data() + (size_t)nq * dim, (size_t)nq * 8);
        wr(fo, keys.data(), keys.size() * 4);
        wr(fo, pos.data(), pos.size() * 4);
        wr(fo, bt.data(), bt.size() * 8);
        wr(fo, bk.data(), bk.size() * 8);
        wr(fo, exact.data(), exact.size() * 8);
        printf("metric %d: %u queries, info %u %u %u %u\n", metric, nq, info[0], info[1], info[2], info[3]);
    }
    fclose(fo);
    printf("audit ok\n");
    return 0;
}
