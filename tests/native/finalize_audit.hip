// Audit of the list merge, finalize and selection launchers on synthetic candidate lists (test tool, not shipped; driven by
// tests/test_gpu_finalize_audit.py).  Every case hands hand-made sorted lists (or a score array) to ONE of the library's own
// launchers -- launch_merge_finalize, launch_merge_finalize_multi, launch_batch_finalize, a chain of launch_exact_select
// rounds -- and dumps everything the launcher could have written.  Result blocks, sink planes and the score scratch are
// filled with 0xA5 bytes before the launch, so the test also sees what was NOT written.  Every judgement is made in Python.
//
//   finalize_audit <case file> <output file>
//   finalize_audit tau <metric> <ld> <R bits> <Q bits> <s bits> <in_extra code> [the same six again ...]
//       host only: one line "<found> <tau bits>" per set -- range_tau<METRIC>(ld, R, Q, s, &tau, in_extra), the LARGEST f32
//       key whose shipped bound is below the score s.  f64 arguments and the f32 result are hexadecimal bit patterns.
//
// case file (little endian): u32 magic 'VLFN', u32 n_cases, then per case
//   u32 h[20]: mode, metric, nq, n_lists, n_parts, dim, m_rows, k, seq, sink, ks, q0, in_extra code, flag word, n_rounds,
//              expect_refuse, n_bkeys, n_entries, 0, 0
//   u64 n_rows, u64 n_scores, u64 row_offset, f64 R
//   FINALIZE / MULTI / BATCH: f64 master[m_rows][dim] (m_rows = 0: the previous case's rows), f64 q[nq][dim], f64 q_norm[nq],
//       u32 len[lists], f32 key[n_entries], u32 pos[n_entries] (the lists' real entries, list after list; the tool pads
//       every list to 64 with sentinels), f32 bkey[n_bkeys], u32 bq[n_bkeys], and with a sink u64 pos_to_id[rows].
//       lists = nq * n_lists (FINALIZE, query-major), n_lists (MULTI: n_lists is the total over the partitions), nq (BATCH)
//   SELECT: f64 scores[n_scores], u32 k_r[n_rounds]
// output file: u32 magic, u32 n_cases, then per case
//   u32 magic, mode, launcher status, n_blocks, n_bkeys, sink queries (q0 + nq, 0 without a sink); f64 in_extra;
//   SearchResultBlock[n_blocks] (FINALIZE / BATCH: nq; MULTI: 4; SELECT: n_rounds); with a sink u64 cnt[q0 + nq],
//   score_bits, gpos, ids [(q0 + nq) * ks] each; BATCH: f64 score_scratch[nq][64];
//   f64 B_device[n_bkeys], f64 B_host[n_bkeys]: bound_for_key<METRIC>(bkey[i], ld, R, q_norm[bq[i]], in_extra)
// Status only on stdout, "audit ok" last; exit status 0 = every stage ran, 2 = the case was refused and nothing launched.
//
// Safe on a shared card by construction: a case is refused unless every listed position is below the number of master
// rows the tool allocated and every count fits the buffers the launchers are documented to take, so a kernel that picks
// the wrong candidate reads a wrong row, never unmapped memory.  No retries; every HIP call is checked.
#include "../../vectorlite_amd/csrc/kernels.hip"
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"

#include <cstdio>
#include <vector>

using namespace vl;

namespace {

enum Mode : uint32_t { FINALIZE = 0, MULTI = 1, BATCH = 2, SELECT = 3 };
constexpr uint32_t MAGIC = 0x4e464c56u;  // "VLFN"
constexpr int FILL = 0xA5;
constexpr double IN_EXTRA[4] = {0.0, IN_EXTRA_I8_SINGLE, IN_EXTRA_BF16_SINGLE, IN_EXTRA_MFMA};

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

[[noreturn]] void refuse(uint32_t c, const char* why)
{
    printf("REFUSED case %u: %s\n", c, why);
    exit(2);
}

template <int METRIC>
__global__ void k_audit_bounds(const float* __restrict__ keys, const uint32_t* __restrict__ bq, uint32_t n, uint32_t ld, double R,
                               const double* __restrict__ q_norms, double in_extra, double* __restrict__ b)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = bound_for_key<METRIC>(keys[i], ld, R, q_norms[bq[i]], in_extra);
}

double host_bound(int metric, float key, uint32_t ld, double R, double Q, double in_extra)
{
    switch (metric) {
    case COSINE: return bound_for_key<COSINE>(key, ld, R, Q, in_extra);
    case EUCLIDEAN: return bound_for_key<EUCLIDEAN>(key, ld, R, Q, in_extra);
    case MANHATTAN: return bound_for_key<MANHATTAN>(key, ld, R, Q, in_extra);
    default: return bound_for_key<DOT>(key, ld, R, Q, in_extra);
    }
}

// device buffer of `count` elements (at least one), every byte = fill
template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t count = 0;
    DBuf(size_t n, int fill) : count(n)
    {
        CK(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
        CK(hipMemset(p, fill, (n ? n : 1) * sizeof(T)));
    }
    ~DBuf() { (void)hipFree(p); }
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    void up(const std::vector<T>& v)
    {
        if (v.size() > count) {
            printf("FAIL upload past the buffer\n");
            exit(1);
        }
        if (!v.empty()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    std::vector<T> down() const
    {
        std::vector<T> v(count);
        if (count) CK(hipMemcpy(v.data(), p, count * sizeof(T), hipMemcpyDeviceToHost));
        return v;
    }
};

FILE* g_in = nullptr;
FILE* g_out = nullptr;

template <typename T>
std::vector<T> rd(size_t count)
{
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, g_in) != count) {
        printf("FAIL short case file\n");
        exit(2);
    }
    return v;
}

void wr(const void* p, size_t bytes)
{
    if (bytes && fwrite(p, 1, bytes, g_out) != bytes) {
        printf("FAIL short write\n");
        exit(1);
    }
}
template <typename T>
void wr(const std::vector<T>& v)
{
    wr(v.data(), v.size() * sizeof(T));
}

uint64_t hex64(const char* s) { return strtoull(s, nullptr, 16); }
double as_f64(uint64_t b)
{
    double d;
    memcpy(&d, &b, 8);
    return d;
}

int tau_main(int argc, char** argv)
{
    if (argc < 8 || (argc - 2) % 6 != 0) {
        printf("usage: finalize_audit tau <metric> <ld> <R bits> <Q bits> <s bits> <in_extra code> ...\n");
        return 2;
    }
    for (int a = 2; a + 6 <= argc; a += 6) {
        const int metric = atoi(argv[a]);
        const uint32_t ld = (uint32_t)strtoul(argv[a + 1], nullptr, 10);
        const uint32_t code = (uint32_t)strtoul(argv[a + 5], nullptr, 10);
        if (metric < 0 || metric > 3 || code > 3) return 2;
        float tau = 0.0f;
        const bool found = range_tau(metric, ld, as_f64(hex64(argv[a + 2])), as_f64(hex64(argv[a + 3])), as_f64(hex64(argv[a + 4])),
                                     &tau, IN_EXTRA[code]);
        uint32_t bits;
        memcpy(&bits, &tau, 4);
        printf("%d %08x\n", found ? 1 : 0, bits);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && strcmp(argv[1], "tau") == 0) return tau_main(argc, argv);
    if (argc != 3) {
        printf("usage: finalize_audit <case> <out>\n");
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    if (!g_in) {
        printf("FAIL cannot open %s\n", argv[1]);
        return 2;
    }
    const std::vector<uint32_t> fh = rd<uint32_t>(2);
    if (fh[0] != MAGIC || fh[1] == 0 || fh[1] > 4096) {
        printf("FAIL bad case header\n");
        return 2;
    }
    const uint32_t n_cases = fh[1];
    g_out = fopen(argv[2], "wb");
    if (!g_out) {
        printf("FAIL cannot open %s\n", argv[2]);
        return 2;
    }
    wr(fh);

    hipStream_t s;
    CK(hipStreamCreate(&s));
    // allocated as the library allocates them: the launchers' merge levels live in the tails
    DBuf<Cand32> d_part(PARTIALS32_ENTRIES, 0);
    DBuf<Cand64> d_part64(PARTIALS64_ENTRIES, 0);
    DBuf<uint32_t> d_nan(1, 0);
    std::vector<Cand32> h_part;
    double* d_master = nullptr;  // the rows of the current (or an earlier) case
    uint64_t master_rows = 0;
    uint32_t master_dim = 0;

    for (uint32_t c = 0; c < n_cases; ++c) {
        const std::vector<uint32_t> h = rd<uint32_t>(20);
        const std::vector<uint64_t> h64 = rd<uint64_t>(4);
        const uint32_t mode = h[0], nq = h[2], n_lists = h[3], n_parts = h[4], dim = h[5], m_rows = h[6], k = h[7], seq = h[8];
        const bool with_sink = h[9] != 0;
        const uint32_t ks = h[10], q0 = h[11], code = h[12], flag_word = h[13], n_rounds = h[14], n_bkeys = h[16], n_entries = h[17];
        const bool expect_refuse = h[15] != 0;
        const int metric = (int)h[1];
        const uint64_t n_rows = h64[0], n_scores = h64[1], row_offset = h64[2];
        const double R = as_f64(h64[3]);
        if (mode > SELECT || metric < 0 || metric > 3 || code > 3) refuse(c, "mode / metric / in_extra code");
        const double in_extra = IN_EXTRA[code];

        if (mode == SELECT) {
            if (n_scores == 0 || n_scores > (1ull << 26) || n_rounds == 0 || n_rounds > (uint32_t)SELECT_MAX_ROUNDS)
                refuse(c, "SELECT: score count or rounds");
            const std::vector<double> scores = rd<double>(n_scores);
            const std::vector<uint32_t> kr = rd<uint32_t>(n_rounds);
            for (uint32_t r = 0; r < n_rounds; ++r)
                if (kr[r] > (uint32_t)KP) refuse(c, "SELECT: k above KP");
            DBuf<double> d_scores(n_scores, 0);
            d_scores.up(scores);
            DBuf<SearchResultBlock> d_blocks(n_rounds, FILL);
            CK(hipMemcpy(d_nan.p, &flag_word, 4, hipMemcpyHostToDevice));
            hipError_t rc = hipSuccess;
            for (uint32_t r = 0; r < n_rounds && rc == hipSuccess; ++r)
                rc = launch_exact_select(s, d_scores.p, n_scores, kr[r], d_part64.p, d_nan.p, d_blocks.p + r,
                                         r ? d_blocks.p + (r - 1) : nullptr);
            CK(hipStreamSynchronize(s));
            if (rc != hipSuccess && !expect_refuse) {
                printf("FAIL case %u: launch_exact_select: %s\n", c, hipGetErrorString(rc));
                return 1;
            }
            const uint32_t oh[6] = {MAGIC, mode, (uint32_t)rc, n_rounds, 0, 0};
            wr(oh, sizeof oh);
            wr(&in_extra, 8);
            wr(d_blocks.down());
            printf("case %u: SELECT n %llu rounds %u status %d\n", c, (unsigned long long)n_scores, n_rounds, (int)rc);
            continue;
        }

        // ---- the three list modes ----
        if (dim == 0 || dim > 4096 || nq == 0) refuse(c, "dim / nq");
        uint64_t lists_all = 0;
        if (mode == FINALIZE) {
            // without a merge level (n_lists <= 64) the launcher touches the lists alone: 512 queries x 64 lists, which the
            // library's scan never leaves (it caps 512 queries at 32 lists each), get a buffer of their own size below
            if (n_lists == 0 || n_lists > (uint32_t)SCAN_MAX_GRID ||
                (uint64_t)nq * n_lists > (n_lists <= 64 ? (uint64_t)SCAN_BATCH_MAX_QUERIES * 64 : (uint64_t)PARTIALS32_LISTS))
                refuse(c, "FINALIZE: lists past the partial-list area");
            if (n_lists > 64 && nq > (uint32_t)SCAN_BATCH_QB) refuse(c, "FINALIZE: a merge level serves at most QB queries");
            if (k > (uint32_t)KP) refuse(c, "FINALIZE: k above KP");
            if (seq && nq != 1) refuse(c, "FINALIZE: a stamped search is one query");
            lists_all = (uint64_t)nq * n_lists;
        } else if (mode == MULTI) {
            if (nq != 1 || n_lists == 0 || n_lists > (uint32_t)SCAN_MAX_GRID || n_parts > 8) refuse(c, "MULTI: lists / parts");
            if (k > (uint32_t)KMULTI_MAX) refuse(c, "MULTI: k above KMULTI_MAX");
            if (seq || with_sink || code) refuse(c, "MULTI takes no stamp, sink or in_extra");
            lists_all = n_lists;
        } else {
            if (nq > 4096 || k > (uint32_t)KP || seq) refuse(c, "BATCH: nq / k / seq");
            lists_all = nq;
        }
        if (with_sink && ((uint64_t)q0 + nq > (1u << 20) || ks > 4096)) refuse(c, "sink shape");
        if (m_rows) {
            const std::vector<double> rows = rd<double>((size_t)m_rows * dim);
            if (d_master) CK(hipFree(d_master));
            CK(hipMalloc(&d_master, rows.size() * 8));
            CK(hipMemcpy(d_master, rows.data(), rows.size() * 8, hipMemcpyHostToDevice));
            master_rows = m_rows;
            master_dim = dim;
        }
        if (!d_master || master_dim != dim) refuse(c, "no master rows of this dim");
        std::vector<double> q = rd<double>((size_t)nq * dim);
        const std::vector<double> qn = rd<double>(nq);
        const std::vector<uint32_t> len = rd<uint32_t>(lists_all);
        const std::vector<float> keys = rd<float>(n_entries);
        const std::vector<uint32_t> pos = rd<uint32_t>(n_entries);
        const std::vector<float> bkeys = rd<float>(n_bkeys);
        const std::vector<uint32_t> bq = rd<uint32_t>(n_bkeys);
        std::vector<unsigned long long> pos_to_id;
        if (with_sink) pos_to_id = rd<unsigned long long>(master_rows);
        uint64_t total = 0;
        for (uint64_t l = 0; l < lists_all; ++l) {
            if (len[l] > (uint32_t)KP) refuse(c, "a list longer than KP");
            total += len[l];
        }
        if (total != n_entries) refuse(c, "list lengths do not add up");
        for (uint32_t i = 0; i < n_entries; ++i)
            if (pos[i] >= master_rows || keys[i] != keys[i]) refuse(c, "a position past the master rows, or a NaN key");
        for (uint32_t i = 0; i < n_bkeys; ++i)
            if (bq[i] >= nq) refuse(c, "bound query index");

        h_part.assign(lists_all * KP, Cand32{-INFINITY, POS_SENTINEL});
        for (uint64_t l = 0, e = 0; l < lists_all; ++l)
            for (uint32_t j = 0; j < len[l]; ++j, ++e) h_part[l * KP + j] = Cand32{keys[e], pos[e]};
        DBuf<Cand32> d_wide(lists_all > PARTIALS32_LISTS ? lists_all * KP : 0, 0);
        DBuf<Cand32>& d_lists = lists_all > PARTIALS32_LISTS ? d_wide : d_part;
        CK(hipMemset(d_part.p, 0, PARTIALS32_ENTRIES * sizeof(Cand32)));
        d_lists.up(h_part);

        q.insert(q.end(), qn.begin(), qn.end());
        DBuf<double> d_q(q.size(), 0);
        d_q.up(q);
        const double* d_qn = d_q.p + (size_t)nq * dim;

        const uint32_t n_blocks = mode == MULTI ? (uint32_t)KMULTI_PARTS : nq;
        DBuf<SearchResultBlock> d_blocks(n_blocks, FILL);
        SearchResultBlock* pinned = nullptr;  // a stamped search writes its block to pinned host memory, as the library does
        if (seq) {
            CK(hipHostMalloc(&pinned, sizeof(SearchResultBlock) * n_blocks));
            memset(pinned, FILL, sizeof(SearchResultBlock) * n_blocks);
        }
        SearchResultBlock* out = seq ? pinned : d_blocks.p;

        const size_t sink_q = with_sink ? (size_t)q0 + nq : 0;
        DBuf<unsigned long long> d_cnt(sink_q, FILL), d_sb(sink_q * ks, FILL), d_gp(sink_q * ks, FILL), d_ids(sink_q * ks, FILL);
        DBuf<unsigned long long> d_p2i(pos_to_id.size(), 0);
        d_p2i.up(pos_to_id);
        ShardRecordSink sink;
        if (with_sink) {
            sink.cnt = d_cnt.p;
            sink.score_bits = d_sb.p;
            sink.gpos = d_gp.p;
            sink.ids = d_ids.p;
            sink.pos_to_id = d_p2i.p;
            sink.row_offset = row_offset;
            sink.ks = ks;
            sink.q0 = q0;
        }
        DBuf<double> d_scratch(mode == BATCH ? (size_t)nq * KP : 0, FILL);

        hipError_t rc;
        if (mode == FINALIZE)
            rc = launch_merge_finalize(s, metric, d_lists.p, (int)n_lists, (int)nq, d_master, d_q.p, d_qn, dim, n_rows, k, R, out,
                                       in_extra, seq, with_sink ? &sink : nullptr);
        else if (mode == MULTI)
            rc = launch_merge_finalize_multi(s, metric, d_lists.p, (int)n_lists, (int)n_parts, d_master, d_q.p, d_qn, dim, n_rows, k,
                                             R, out);
        else
            rc = launch_batch_finalize(s, metric, d_lists.p, (int)nq, d_master, d_q.p, d_qn, dim, n_rows, k, R, out, in_extra,
                                       d_scratch.p, with_sink ? &sink : nullptr);
        CK(hipStreamSynchronize(s));
        if (rc != hipSuccess && !expect_refuse) {
            printf("FAIL case %u: launcher: %s\n", c, hipGetErrorString(rc));
            return 1;
        }

        DBuf<float> d_bk(n_bkeys, 0);
        DBuf<uint32_t> d_bq(n_bkeys, 0);
        DBuf<double> d_b(n_bkeys, 0);
        d_bk.up(bkeys);
        d_bq.up(bq);
        const uint32_t ld = (dim + 3u) & ~3u;
        if (n_bkeys) {
            CK(dispatch_metric(metric, [&](auto M) -> hipError_t {
                constexpr int MM = decltype(M)::value;
                hipLaunchKernelGGL((k_audit_bounds<MM>), dim3((n_bkeys + 255) / 256), dim3(256), 0, s, d_bk.p, d_bq.p, n_bkeys, ld, R, d_qn,
                                   in_extra, d_b.p);
                return hipGetLastError();
            }));
            CK(hipStreamSynchronize(s));
        }
        std::vector<double> b_host(n_bkeys);
        for (uint32_t i = 0; i < n_bkeys; ++i) b_host[i] = host_bound(metric, bkeys[i], ld, R, qn[bq[i]], in_extra);

        const uint32_t oh[6] = {MAGIC, mode, (uint32_t)rc, n_blocks, n_bkeys, (uint32_t)sink_q};
        wr(oh, sizeof oh);
        wr(&in_extra, 8);
        if (seq) wr(pinned, sizeof(SearchResultBlock) * n_blocks);
        else wr(d_blocks.down());
        if (with_sink) {
            wr(d_cnt.down());
            wr(d_sb.down());
            wr(d_gp.down());
            wr(d_ids.down());
        }
        if (mode == BATCH) wr(d_scratch.down());
        wr(d_b.down());
        wr(b_host);
        if (pinned) CK(hipHostFree(pinned));
        printf("case %u: mode %u metric %d nq %u lists %u status %d\n", c, mode, metric, nq, n_lists, (int)rc);
    }
    if (d_master) CK(hipFree(d_master));
    fclose(g_in);
    fclose(g_out);
    printf("audit ok\n");
    return 0;
}
