// Audit of the batched range search's device stages (test tool, not shipped; driven by
// tests/test_gpu_range_batch_audit.py).  Hands the fixed-threshold MFMA pass (launch_rows_bf16_frag +
// launch_mfma_range_candidates) and the tail behind it (launch_range_batch_tail) their inputs directly and writes every
// byte they could have written: each buffer is prefilled with 0xA5 bytes and followed by GUARD bytes of the same
// pattern, and is dumped whole.  Every check is made by the Python test.
//
//   range_batch_audit <case file> <output file>
//   range_batch_audit thr <metric> <ldb> <R bits> <Q bits> <min_score bits> <in_extra bits> [the same six again ...]
//       host only: one line "<RangeKeys code> <thr bits>" per set -- range_key_threshold(metric, ldb, R, Q, min_score,
//       in_extra, &thr).  f64 arguments and the f32 result are hexadecimal bit patterns.
//
// case file (little endian): u32 magic 'VLRB', u32 n_cases, then per case
//   u32 kind (0 pass, 1 tail, 2 chain), n_metrics, metrics[4], n, dim, nq, cap, emit_cap, n_thr, grid, stream, flags, 0
//       grid > 0: VL_MFMA_GRID for this case; stream == 0: VL_MFMA_STREAM_LOADS=0; flags: 1 = dump the exact scores,
//       2 = dump the bounds
//   f64 rows[n][dim], f64 queries[nq][dim], then per metric
//       pass:  u32 thr[n_thr][nq] (f32 bits)
//       tail:  u32 cand_pos[nq][cap], u32 cnt[nq], f64 min_scores[nq]
//       chain: f64 min_scores[nq]   (thr from range_key_threshold with IN_EXTRA_MFMA, as search_range_batch_mfma)
// output file, per case and metric:
//   u32 magic, kind, metric, nq, nq_pad, n, ldb, cap, emit_cap, n_thr, flags, out_n; f64 R; f64 Q[nq]
//   pass / chain, per threshold vector: u32 ksteps, chunks, grid_x, stages; u32 thr[nq]; u32 staged[nq];
//       cnt[nq_pad] + guard; Cand32 cand[nq][cap] + guard; with flag 2: f64 B(key)[nq][cap], f64 B(pred(thr))[nq]
//   with flag 1: f64 exact[nq][n]
//   tail / chain: ctr[nq][4] + guard, u32 out_pos[out_n] + guard, f64 out_scores[out_n] + guard,
//       f64 sv_score[nq][RBATCH_SEG] + guard, u32 sv_pos[nq][RBATCH_SEG] + guard
// Status only on stdout; the last line is "audit ok".
#include "../../vectorlite_amd/csrc/kernels.hip"
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"

#include <cstdio>
#include <vector>

using namespace vl;

namespace {

constexpr uint32_t MAGIC = 0x42524c56u;  // "VLRB"
constexpr size_t GUARD = 256;            // bytes behind every dumped buffer
constexpr int PATTERN = 0xA5;
enum Kind : uint32_t { PASS = 0, TAIL = 1, CHAIN = 2 };

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

// B(key) of every buffer entry and B(pred(thr)) of every query, with the library's own bound function
template <int METRIC>
__global__ void k_audit_bounds(const Cand32* __restrict__ cand, const float* __restrict__ pred, uint32_t nq, uint32_t cap,
                               uint32_t ldb, double R, const double* __restrict__ q_norms, double in_extra,
                               double* __restrict__ b_key, double* __restrict__ b_pred)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)nq * cap) return;
    const uint32_t q = (uint32_t)(i / cap);
    b_key[i] = bound_for_key<METRIC>(cand[i].key, ldb, R, q_norms[q], in_extra);
    if (i % cap == 0) b_pred[q] = bound_for_key<METRIC>(pred[q], ldb, R, q_norms[q], in_extra);
}

std::vector<void*> g_live;  // freed after every case

template <typename T>
T* dalloc(size_t count, int fill = PATTERN)  // count entries of `fill` bytes and the guard behind them
{
    T* p = nullptr;
    CK(hipMalloc(&p, count * sizeof(T) + GUARD));
    CK(hipMemset(p, fill, count * sizeof(T)));
    CK(hipMemset(reinterpret_cast<unsigned char*>(p) + count * sizeof(T), PATTERN, GUARD));
    g_live.push_back(p);
    return p;
}

template <typename T>
T* upload(const T* host, size_t count)
{
    T* p = dalloc<T>(count ? count : 1);
    if (count) CK(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

void wr(FILE* f, const void* p, size_t bytes)
{
    if (bytes && fwrite(p, 1, bytes, f) != bytes) {
        printf("FAIL short write\n");
        exit(1);
    }
}

template <typename T>
void rd(FILE* f, std::vector<T>& v, size_t count)
{
    v.resize(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        printf("FAIL short case file\n");
        exit(2);
    }
}

uint64_t hex64(const char* s) { return strtoull(s, nullptr, 16); }
double as_f64(uint64_t b)
{
    double d;
    memcpy(&d, &b, 8);
    return d;
}
uint32_t f32_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

int thr_main(int argc, char** argv)
{
    if (argc < 8 || (argc - 2) % 6 != 0) {
        printf("usage: range_batch_audit thr <metric> <ldb> <R bits> <Q bits> <min_score bits> <in_extra bits> ...\n");
        return 2;
    }
    for (int a = 2; a + 6 <= argc; a += 6) {
        float thr = 0.0f;
        const RangeKeys r = range_key_threshold(atoi(argv[a]), (uint32_t)atoi(argv[a + 1]), as_f64(hex64(argv[a + 2])),
                                                as_f64(hex64(argv[a + 3])), as_f64(hex64(argv[a + 4])), as_f64(hex64(argv[a + 5])),
                                                &thr);
        printf("%d %08x\n", (int)r, f32_bits(thr));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && strcmp(argv[1], "thr") == 0) return thr_main(argc, argv);
    if (argc != 3) {
        printf("usage: range_batch_audit <case> <out>\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    uint32_t top[2];
    if (!fi || !fo || fread(top, 4, 2, fi) != 2 || top[0] != MAGIC) {
        printf("FAIL cannot open the files, or bad case header\n");
        return 2;
    }
    hipStream_t s;
    CK(hipStreamCreate(&s));
    for (uint32_t ci = 0; ci < top[1]; ++ci) {
        std::vector<uint32_t> hdr;
        rd(fi, hdr, 16);
        const uint32_t kind = hdr[0], n_metrics = hdr[1], n32 = hdr[6], dim = hdr[7], nq = hdr[8], cap = hdr[9], emit_cap = hdr[10];
        const uint32_t n_thr = kind == CHAIN ? 1u : hdr[11], grid = hdr[12], stream = hdr[13], flags = hdr[14];
        const uint64_t n = n32;
        if (kind > CHAIN || n_metrics < 1 || n_metrics > 4 || n == 0 || dim == 0 || nq == 0 || nq > (uint32_t)MFMA_MAX_BATCH ||
            cap == 0 || cap > (uint32_t)MFMA_CAND_CAP || emit_cap > RBATCH_SEG || (kind == PASS && n_thr == 0)) {
            printf("FAIL bad parameters in case %u\n", ci);
            return 2;
        }
        if (grid) setenv("VL_MFMA_GRID", std::to_string(grid).c_str(), 1);
        else unsetenv("VL_MFMA_GRID");
        if (stream) unsetenv("VL_MFMA_STREAM_LOADS");
        else setenv("VL_MFMA_STREAM_LOADS", "0", 1);
        std::vector<double> rows, qs, qn(nq);
        rd(fi, rows, n * dim);
        rd(fi, qs, (size_t)nq * dim);
        // query norms: sequential sum of squares, as the host stages a query (stage_query, flat_index.cpp)
        for (uint32_t q = 0; q < nq; ++q) {
            double ss = 0.0;
            for (uint32_t c = 0; c < dim; ++c) ss += qs[(size_t)q * dim + c] * qs[(size_t)q * dim + c];
            qn[q] = sqrt(ss);
        }
        const double* d_master = upload(rows.data(), rows.size());
        const double* d_q = upload(qs.data(), qs.size());
        const double* d_qn = upload(qn.data(), qn.size());

        const uint32_t ldb = mfma_ldb(dim);
        uint32_t nq_pad = nq;
        double R = 0.0;
        void* d_slab16 = nullptr;
        float *d_nrm16 = nullptr, *d_sqn16 = nullptr;
        if (kind != TAIL) {
            if (!mfma_scan_supported(dim, COSINE) || !mfma_rows_kernel(dim)) {
                printf("FAIL no row-stationary MFMA kernel for dim %u\n", dim);
                return 2;
            }
            // R as search_range_batch_mfma takes it: the largest row norm of launch_ingest's stats
            const uint32_t ld = (dim + 3u) & ~3u;
            const uint64_t n_alloc = (n + 2 * MFMA_TILE_ROWS - 1) / MFMA_TILE_ROWS * MFMA_TILE_ROWS;
            float* d_slab = dalloc<float>(n_alloc * ld, 0x40);
            float* d_inv = dalloc<float>(n_alloc, 0x40);
            uint8_t* d_flags = dalloc<uint8_t>(n_alloc, 0);
            IngestStats* d_stats = dalloc<IngestStats>(1, 0);
            CK(launch_ingest(s, d_master, d_slab, d_inv, d_flags, d_stats, n, dim, ld));
            IngestStats st{};
            CK(hipMemcpyAsync(&st, d_stats, sizeof st, hipMemcpyDeviceToHost, s));
            CK(hipStreamSynchronize(s));
            if (st.n_out_of_domain) {
                printf("FAIL %u rows outside the fast-path domain\n", st.n_out_of_domain);
                return 3;
            }
            memcpy(&R, &st.max_norm_bits, 8);
            // per-row buffers in whole 64-row tiles plus one more tile, the rows past n filled with 0x40 bytes (bf16 / f32
            // ~3.0): a row let through past n_rows shows up with a large key
            d_slab16 = dalloc<uint16_t>(n_alloc * ldb, 0x40);
            d_nrm16 = dalloc<float>(n_alloc, 0x40);
            d_sqn16 = dalloc<float>(n_alloc, 0x40);
            // whole query chunks, as the launcher pads them: a launch sequence holds 16 chunks (mfma_sequence_queries)
            const uint32_t qpc = mfma_sequence_queries(dim) / 16u;
            nq_pad = (nq + qpc - 1) / qpc * qpc;
        }

        for (uint32_t mi = 0; mi < n_metrics; ++mi) {
            const int metric = (int)hdr[2 + mi];
            std::vector<double> min_scores;
            Cand32* d_cand = nullptr;
            uint32_t* d_cnt = nullptr;
            std::vector<std::vector<uint32_t>> thr_in(n_thr);
            if (kind == PASS)
                for (auto& t : thr_in) rd(fi, t, nq);
            if (kind == CHAIN) rd(fi, min_scores, nq);

            // ---- what the pass writes is collected here and written behind the header (which needs nq_pad) ----
            std::vector<unsigned char> body;
            auto put = [&](const void* p, size_t bytes) {
                const unsigned char* c = static_cast<const unsigned char*>(p);
                body.insert(body.end(), c, c + bytes);
            };
            auto put_dev = [&](const void* dev, size_t bytes) {
                std::vector<unsigned char> h(bytes);
                CK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
                put(h.data(), bytes);
            };
            if (kind != TAIL) {
                if (!mfma_scan_supported(dim, metric)) {
                    printf("FAIL no MFMA filter for metric %d\n", metric);
                    return 2;
                }
                for (uint32_t ti = 0; ti < n_thr; ++ti) {
                    std::vector<float> thr(nq), pred(nq);
                    std::vector<uint32_t> thr_bits(nq), staged(nq, 1);
                    for (uint32_t q = 0; q < nq; ++q) {
                        if (kind == CHAIN) {
                            float t = INFINITY;
                            if (range_key_threshold(metric, ldb, R, qn[q], min_scores[q], IN_EXTRA_MFMA, &t) == RANGE_KEYS_ALL) {
                                t = INFINITY;  // every row a candidate: not the filter's job (search_range_batch_mfma peels it off)
                                staged[q] = 0;
                            }
                            thr[q] = t;
                        } else {
                            memcpy(&thr[q], &thr_in[ti][q], 4);
                        }
                        thr_bits[q] = f32_bits(thr[q]);
                        pred[q] = thr[q] == -INFINITY ? -INFINITY : ordered_to_f32(f32_to_ordered(thr[q]) - 1u);
                    }
                    if (ti == 0) CK(launch_rows_bf16_frag(s, d_master, 0, n, dim, d_slab16, d_nrm16, d_sqn16));
                    MfmaScratch w;
                    w.nq_cap = nq;
                    w.nq_pad_cap = nq_pad;
                    w.q_bf16 = dalloc<uint16_t>((size_t)nq_pad * ldb);
                    w.thr = dalloc<float>(nq_pad);
                    w.cnt = dalloc<uint32_t>(nq_pad);
                    w.cand = dalloc<Cand32>((size_t)nq * cap);
                    CK(hipMemcpy(w.thr, thr.data(), nq * 4, hipMemcpyHostToDevice));
                    MfmaLaunchInfo li;
                    CK(launch_mfma_range_candidates(s, metric, d_slab16, d_nrm16, d_sqn16, d_q, nq, n, dim, w, cap, &li));
                    CK(hipStreamSynchronize(s));
                    const uint32_t info[4] = {(uint32_t)li.ksteps, (uint32_t)li.chunks, (uint32_t)li.grid_x, (uint32_t)li.stages};
                    put(info, sizeof info);
                    put(thr_bits.data(), nq * 4);
                    put(staged.data(), nq * 4);
                    // cnt[0 .. nq_pad) and, as its guard, the GUARD bytes the launcher must not have cleared
                    put_dev(w.cnt, (size_t)nq_pad * 4 + GUARD);
                    put_dev(w.cand, (size_t)nq * cap * sizeof(Cand32) + GUARD);
                    if (flags & 2u) {
                        const float* d_pred = upload(pred.data(), nq);
                        double* d_bk = dalloc<double>((size_t)nq * cap);
                        double* d_bp = dalloc<double>(nq);
                        CK(dispatch_metric(metric, [&](auto M) -> hipError_t {
                            constexpr int MM = decltype(M)::value;
                            hipLaunchKernelGGL((k_audit_bounds<MM>), dim3((uint32_t)(((size_t)nq * cap + 255) / 256)), dim3(256), 0, s,
                                               w.cand, d_pred, nq, cap, ldb, R, d_qn, (double)IN_EXTRA_MFMA, d_bk, d_bp);
                            return hipGetLastError();
                        }));
                        CK(hipStreamSynchronize(s));
                        put_dev(d_bk, (size_t)nq * cap * 8);
                        put_dev(d_bp, (size_t)nq * 8);
                    }
                    d_cand = w.cand;
                    d_cnt = w.cnt;
                }
            }
            if (flags & 1u) {
                double* d_exact = dalloc<double>(n * nq);
                uint32_t* d_nan = dalloc<uint32_t>(1, 0);
                for (uint32_t q = 0; q < nq; ++q)
                    CK(launch_exact_scan(s, metric, d_master, d_q + (size_t)q * dim, n, dim, d_exact + (size_t)q * n, d_nan));
                CK(hipStreamSynchronize(s));
                put_dev(d_exact, n * nq * 8);
            }
            const uint32_t out_n = (kind == PASS) ? 0u : ((size_t)nq * emit_cap ? nq * emit_cap : 1u);
            if (kind != PASS) {
                if (kind == TAIL) {
                    std::vector<uint32_t> pos, cnt;
                    rd(fi, pos, (size_t)nq * cap);
                    rd(fi, cnt, nq);
                    rd(fi, min_scores, nq);
                    std::vector<Cand32> cand((size_t)nq * cap);
                    for (size_t i = 0; i < cand.size(); ++i) {
                        cand[i].key = 0.0f;
                        cand[i].pos = pos[i];
                    }
                    d_cand = upload(cand.data(), cand.size());
                    d_cnt = upload(cnt.data(), cnt.size());
                }
                const double* d_min = upload(min_scores.data(), nq);
                uint32_t* d_ctr = dalloc<uint32_t>((size_t)nq * RBATCH_CTR_WORDS, 0);
                uint32_t* d_out_pos = dalloc<uint32_t>(out_n);
                double* d_out_scores = dalloc<double>(out_n);
                double* d_sv_score = dalloc<double>((size_t)nq * RBATCH_SEG);
                uint32_t* d_sv_pos = dalloc<uint32_t>((size_t)nq * RBATCH_SEG);
                CK(launch_range_batch_tail(s, metric, d_cand, d_cnt, cap, nq, d_master, d_q, d_min, dim, n, emit_cap, d_sv_score,
                                           d_sv_pos, d_ctr, d_out_pos, d_out_scores));
                CK(hipStreamSynchronize(s));
                put_dev(d_ctr, (size_t)nq * RBATCH_CTR_WORDS * 4 + GUARD);
                put_dev(d_out_pos, (size_t)out_n * 4 + GUARD);
                put_dev(d_out_scores, (size_t)out_n * 8 + GUARD);
                put_dev(d_sv_score, (size_t)nq * RBATCH_SEG * 8 + GUARD);
                put_dev(d_sv_pos, (size_t)nq * RBATCH_SEG * 4 + GUARD);
            }
            const uint32_t oh[12] = {MAGIC, kind, (uint32_t)metric, nq, nq_pad, n32, ldb, cap, emit_cap, n_thr, flags, out_n};
            wr(fo, oh, sizeof oh);
            wr(fo, &R, 8);
            wr(fo, qn.data(), (size_t)nq * 8);
            wr(fo, body.data(), body.size());
            printf("case %u metric %d: kind %u, %u queries, %llu rows\n", ci, metric, kind, nq, (unsigned long long)n);
        }
        CK(hipStreamSynchronize(s));
        for (void* p : g_live) CK(hipFree(p));
        g_live.clear();
    }
    fclose(fi);
    fclose(fo);
    printf("audit ok\n");
    return 0;
}
