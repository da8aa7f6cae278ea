// Audit of the 64-entry candidate lists launch_mfma_candidates_masked writes (test tool, not shipped; driven by
// tests/test_gpu_masked_mfma_audit.py).  From outside a list that lost a row is invisible: the certificate refuses it and
// the fallback repairs the answer.  Here the lists themselves are dumped.  One data set (rows, queries, one keep bitmap
// per query) and a sequence of runs on it:
//   kind 0  the masked filter: launch_mfma_candidates_masked with the table of the queries' bitmaps;
//   kind 1  the yardstick: the UNMASKED launch_mfma_candidates on a second slab that holds only the rows bitmap `mask`
//           keeps (converted from the gathered f64 rows: the conversion is per row, and a row's key does not depend on
//           its position); the positions it reports are positions in that slab.
// Every check is made by the Python test.
//
//   masked_mfma_audit <case file> <output file>
//
// case file (little endian): u32 magic 'VLMM', u32 n, u32 dim, u32 nq_all, u32 n_runs, u32 runs[n_runs][5] = (kind, metric,
//                            nq, stages, mask), f64 rows[n][dim], f64 queries[nq_all][dim], f64 norms[nq_all],
//                            u64 masks[nq_all][(n + 63) / 64]
// output file, one block per run: u32 magic, u32 rows of the slab that was scanned, u32 cnt[nq], then nq x 64 x (f32 key,
//                            u32 pos)
// A run uses the first nq queries; VL_MFMA_STAGES is set to `stages` for its launch (the launcher reads it per launch).
// Status only on stdout; exit status 0 and a last line "audit ok" = every run ran.
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace vl;

namespace {

constexpr uint32_t MAGIC = 0x4d4d4c56u;  // "VLMM"

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

template <typename T>
T* dalloc(size_t count)
{
    T* p = nullptr;
    CK(hipMalloc(&p, count * sizeof(T) + 256));
    CK(hipMemset(p, 0, count * sizeof(T) + 256));
    return p;
}

void rd(FILE* f, void* p, size_t bytes)
{
    if (bytes && fread(p, 1, bytes, f) != bytes) {
        printf("FAIL short read\n");
        exit(1);
    }
}

void wr(FILE* f, const void* p, size_t bytes)
{
    if (bytes && fwrite(p, 1, bytes, f) != bytes) {
        printf("FAIL short write\n");
        exit(1);
    }
}

// the fragment-major bf16 slab of `n` rows and its two per-row arrays, allocated in whole tiles
struct Slab {
    void* bf16 = nullptr;
    float* norm = nullptr;
    float* sqnorm = nullptr;
    uint32_t n = 0;
};

Slab make_slab(hipStream_t s, const std::vector<double>& rows, uint32_t n, uint32_t dim)
{
    Slab sl;
    sl.n = n;
    const uint32_t ldb = mfma_ldb(dim);
    const size_t n_alloc = ((size_t)n + MFMA_TILE_ROWS - 1) / MFMA_TILE_ROWS * MFMA_TILE_ROWS;
    double* d_rows = dalloc<double>((size_t)n * dim);
    CK(hipMemcpy(d_rows, rows.data(), (size_t)n * dim * sizeof(double), hipMemcpyHostToDevice));
    sl.bf16 = dalloc<unsigned char>(n_alloc * ldb * 2);
    sl.norm = dalloc<float>(n_alloc);
    sl.sqnorm = dalloc<float>(n_alloc);
    CK(launch_rows_bf16_frag(s, d_rows, 0, n, dim, sl.bf16, sl.norm, sl.sqnorm));
    CK(hipStreamSynchronize(s));
    CK(hipFree(d_rows));
    return sl;
}

void free_slab(Slab& sl)
{
    CK(hipFree(sl.bf16));
    CK(hipFree(sl.norm));
    CK(hipFree(sl.sqnorm));
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: masked_mfma_audit <case file> <output file>\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        printf("FAIL cannot open the files\n");
        return 2;
    }
    uint32_t head[5];
    rd(in, head, sizeof(head));
    const uint32_t n = head[1], dim = head[2], nq_all = head[3], n_runs = head[4];
    if (head[0] != MAGIC || n == 0 || dim == 0 || nq_all == 0 || nq_all > (uint32_t)MFMA_MAX_BATCH || !mfma_rows_kernel(dim)) {
        printf("FAIL bad case header\n");
        return 2;
    }
    std::vector<uint32_t> runs((size_t)n_runs * 5);
    rd(in, runs.data(), runs.size() * sizeof(uint32_t));
    const size_t words = ((size_t)n + 63) / 64;
    std::vector<double> rows((size_t)n * dim), q64((size_t)nq_all * (dim + 1));
    std::vector<unsigned long long> masks((size_t)nq_all * words);
    rd(in, rows.data(), rows.size() * sizeof(double));
    rd(in, q64.data(), (size_t)nq_all * dim * sizeof(double));
    std::vector<double> norms(nq_all);
    rd(in, norms.data(), nq_all * sizeof(double));
    rd(in, masks.data(), masks.size() * sizeof(unsigned long long));
    fclose(in);

    hipStream_t s;
    CK(hipStreamCreate(&s));
    Slab full = make_slab(s, rows, n, dim);
    const uint32_t ldb = mfma_ldb(dim);
    const size_t nq_pad = (size_t)nq_all + 256;
    MfmaScratch w;
    w.q_bf16 = dalloc<unsigned char>(nq_pad * ldb * 2);
    w.gmax = dalloc<int>((size_t)nq_all * MFMA_GROUPS);
    w.thr = dalloc<float>(nq_all);
    w.cand = dalloc<Cand32>((size_t)nq_all * MFMA_CAND_CAP);
    w.cnt = dalloc<uint32_t>(nq_pad);
    w.nq_cap = nq_all;
    w.nq_pad_cap = (uint32_t)nq_pad;
    double* d_q64 = dalloc<double>((size_t)nq_all * (dim + 1));
    Cand32* d_lists = dalloc<Cand32>((size_t)nq_all * KP);
    unsigned long long* d_masks = dalloc<unsigned long long>(masks.size());
    CK(hipMemcpy(d_masks, masks.data(), masks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    std::vector<const unsigned long long*> h_table(nq_all);
    for (uint32_t q = 0; q < nq_all; ++q) h_table[q] = d_masks + (size_t)q * words;
    const unsigned long long** d_table = dalloc<const unsigned long long*>(nq_all);
    CK(hipMemcpy(d_table, h_table.data(), nq_all * sizeof(void*), hipMemcpyHostToDevice));

    std::vector<Cand32> lists((size_t)nq_all * KP);
    std::vector<uint32_t> cnt(nq_all);
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t kind = runs[r * 5], metric = runs[r * 5 + 1], nq = runs[r * 5 + 2], stages = runs[r * 5 + 3], mask = runs[r * 5 + 4];
        if (kind > 1 || nq == 0 || nq > nq_all || mask >= nq_all) {
            printf("FAIL bad run %u\n", r);
            return 2;
        }
        setenv("VL_MFMA_STAGES", std::to_string(stages).c_str(), 1);
        // this run's queries: the first nq, their norms behind them
        std::vector<double> stage((size_t)nq * (dim + 1));
        memcpy(stage.data(), q64.data(), (size_t)nq * dim * sizeof(double));
        memcpy(stage.data() + (size_t)nq * dim, norms.data(), nq * sizeof(double));
        CK(hipMemcpyAsync(d_q64, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice, s));
        CK(hipMemsetAsync(d_lists, 0xEE, (size_t)nq_all * KP * sizeof(Cand32), s));
        uint32_t scanned = n;
        if (kind == 0) {
            CK(launch_mfma_candidates_masked(s, (int)metric, full.bf16, full.norm, full.sqnorm, d_q64, nq, n, dim, w, d_table, d_lists));
        } else {
            std::vector<double> kept;
            uint32_t m = 0;
            const unsigned long long* bm = masks.data() + (size_t)mask * words;
            for (uint32_t p = 0; p < n; ++p)
                if ((bm[p >> 6] >> (p & 63)) & 1ull) {
                    kept.insert(kept.end(), rows.begin() + (size_t)p * dim, rows.begin() + (size_t)(p + 1) * dim);
                    ++m;
                }
            if (m == 0) {
                printf("FAIL run %u: the yardstick needs rows\n", r);
                return 2;
            }
            Slab part = make_slab(s, kept, m, dim);
            CK(launch_mfma_candidates(s, (int)metric, part.bf16, part.norm, part.sqnorm, d_q64, nq, m, dim, w, d_lists));
            CK(hipStreamSynchronize(s));
            free_slab(part);
            scanned = m;
        }
        CK(hipMemcpyAsync(lists.data(), d_lists, (size_t)nq * KP * sizeof(Cand32), hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(cnt.data(), w.cnt, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        const uint32_t bh[2] = {MAGIC, scanned};
        wr(out, bh, sizeof(bh));
        wr(out, cnt.data(), nq * sizeof(uint32_t));
        wr(out, lists.data(), (size_t)nq * KP * sizeof(Cand32));
        printf("run %u: kind %u metric %u nq %u stages %u rows %u\n", r, kind, metric, nq, stages, scanned);
    }
    fclose(out);
    printf("audit ok\n");
    return 0;
}
