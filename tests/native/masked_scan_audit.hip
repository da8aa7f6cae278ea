// Audit of the lists the three masked scans of an exclusion filter write (test tool, not shipped; driven by
// tests/test_gpu_masked_scan_audit.py).  Ingests one case (rows, one query, a set of keep bitmaps), and for every mask,
// metric and stage (f32, bf16, int8) runs the masked kernel ONCE over the whole slab, merges its lists with the library's
// k_merge_lists and writes the 64-entry list -- and, beside it, the yardstick list:
//   f32         k_scan_subset on the ascending kept positions;
//   bf16, int8  the unmasked kernel of the same stage on a second, compacted copy of the slab that holds only the kept
//               rows (converted from the gathered f64 rows: the conversion is per row), positions mapped back through the
//               kept list.
// Last, the resolution kernels of an exclusion token run once on the case's id table and id set -- k_filter_count and
// k_filter_compact with the predicate inverted, k_filter_bits -- and their count, bitmap and list are written out.
// Every check is made by the Python test.
//
//   masked_scan_audit <case file> <output file>
//
// case file (little endian): u32 magic 'VLMA', u32 n_metrics, u32 metrics[4], u32 n, u32 dim, u32 n_masks, u32 stages
//                            (bit 0 f32, bit 1 bf16, bit 2 int8), u32 n_set, f64 rows[n][dim], f64 query[dim],
//                            u64 masks[n_masks][(n + 63) / 64], u64 pos_ids[n], u64 set[n_set] (ascending, unique)
// output file, one block per (mask, metric, stage) in that nesting order, stages 0 (f32), 1 (bf16), 2 (int8):
//                            u32 magic, u32 mask, u32 metric, u32 stage, u32 ran (0: the stage does not serve the metric or
//                            dim; no lists follow), i32 variant, u32 m, u32 yardstick (0: m == 0, no yardstick list),
//                            f32 key[64], u32 pos[64], then f32 yard_key[64], u32 yard_pos[64] when yardstick == 1
//              then the resolution: u32 magic, u32 m, u64 keep[(n + 63) / 64], u32 plist[m]
// Status only on stdout; exit status 0 = every stage ran.
#include "../../vectorlite_amd/csrc/kernels.hip"
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace vl;

namespace {

constexpr uint32_t MAGIC = 0x414d4c56u;  // "VLMA"

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

// n_lists sorted lists -> one sorted list at out, through the library's merge level k_merge_lists (at least one pass, so
// the output is always compact)
void merge_to_one(hipStream_t s, const Cand32* lists, int n_lists, Cand32* buf0, Cand32* buf1, Cand32* out)
{
    Cand32* bufs[2] = {buf0, buf1};
    size_t stride = (size_t)n_lists * KP;
    int ping = 0;
    do {
        const int blocks = (n_lists + 63) / 64;
        Cand32* dst = blocks == 1 ? out : bufs[ping];
        hipLaunchKernelGGL((k_merge_lists<float, Cand32>), dim3(blocks, 1), dim3(1024), 0, s, lists, n_lists, stride, dst,
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

// one 64-entry list; map != nullptr: positions are indices into map[0..m) (the compacted copy) and are mapped back
void write_list(FILE* f, const Cand32* d_list, const uint32_t* map, uint32_t m)
{
    Cand32 list[KP];
    CK(hipMemcpy(list, d_list, sizeof list, hipMemcpyDeviceToHost));
    float keys[KP];
    uint32_t pos[KP];
    for (int i = 0; i < KP; ++i) {
        keys[i] = list[i].key;
        pos[i] = list[i].pos;
        if (map && pos[i] != POS_SENTINEL) {
            if (pos[i] >= m) {
                printf("FAIL the compacted scan returned position %u of %u rows\n", pos[i], m);
                exit(1);
            }
            pos[i] = map[pos[i]];
        }
    }
    wr(f, keys, sizeof keys);
    wr(f, pos, sizeof pos);
}

// the three per-row arrays of one converted copy, n_alloc rows (rows past the converted ones are 0x40 bytes)
struct Bf16Copy {
    void* slab;
    float *nrm, *sqn;
};
struct I8Copy {
    void* slab;
    float *sr, *nrm;
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        printf("usage: masked_scan_audit <case> <out>\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) {
        printf("FAIL cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t hdr[11];
    if (fread(hdr, 4, 11, fi) != 11 || hdr[0] != MAGIC) {
        printf("FAIL bad case header\n");
        return 2;
    }
    const uint32_t n_metrics = hdr[1], n32 = hdr[6], dim = hdr[7], n_masks = hdr[8], stages = hdr[9], n_set = hdr[10];
    const uint64_t n = n32;
    if (n_metrics < 1 || n_metrics > 4 || n == 0 || n > (1u << 20) || dim == 0 || dim > 4096 || n_masks == 0 || n_masks > 256 ||
        stages == 0 || stages > 7 || n_set > (1u << 20)) {
        printf("FAIL bad case parameters\n");
        return 2;
    }
    const uint32_t words = (uint32_t)((n + 63) / 64);
    std::vector<double> rows(n * dim), q(dim);
    std::vector<unsigned long long> masks((size_t)n_masks * words);
    std::vector<unsigned long long> pos_ids(n), id_set(n_set);
    if (fread(rows.data(), 8, rows.size(), fi) != rows.size() || fread(q.data(), 8, q.size(), fi) != q.size() ||
        fread(masks.data(), 8, masks.size(), fi) != masks.size() || fread(pos_ids.data(), 8, pos_ids.size(), fi) != pos_ids.size() ||
        fread(id_set.data(), 8, id_set.size(), fi) != id_set.size()) {
        printf("FAIL short case file\n");
        return 2;
    }
    fclose(fi);
    for (uint32_t i = 1; i < n_set; ++i)
        if (id_set[i - 1] >= id_set[i]) {
            printf("FAIL the id set is not ascending and unique\n");
            return 2;
        }
    // a keep bitmap has no bit at or past n (the resolution's own bitmap, written at the end, is checked by the test)
    if (n % 64)
        for (uint32_t k = 0; k < n_masks; ++k)
            if (masks[(size_t)k * words + words - 1] >> (n % 64)) {
                printf("FAIL mask %u has bits past the last row\n", k);
                return 2;
            }

    const uint32_t ld = (dim + 3u) & ~3u;
    if (!scan_masked_supported(ld)) {
        printf("FAIL no masked f32 scan at stride %u\n", ld);
        return 2;
    }
    hipStream_t s;
    CK(hipStreamCreate(&s));
    // rows past n are filled with 0x40 bytes (f32 ~3.0), so a scan that lets a row past the end through gives it a large key
    const uint64_t n_alloc = n + 128;
    double* d_master = dalloc<double>(n * dim);
    CK(hipMemcpy(d_master, rows.data(), n * dim * 8, hipMemcpyHostToDevice));
    double* d_cmaster = dalloc<double>(n * dim);  // the kept rows, gathered
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
    // the query the way the library hands it over: f32 in the kernel arguments, or f64 in device memory past that stride
    double* d_q = dalloc<double>(dim + 1);
    CK(hipMemcpy(d_q, q.data(), (size_t)dim * 8, hipMemcpyHostToDevice));
    const bool qarg = scan_takes_qarg(ld);
    std::vector<float> q32(ld, 0.0f);
    for (uint32_t c = 0; c < dim; ++c) q32[c] = (float)q[c];

    const bool any16 = (stages & 2) && (scan_bf16_supported(dim, COSINE) || scan_bf16_supported(dim, EUCLIDEAN));
    const bool any8 = (stages & 4) && scan_i8_supported(dim, COSINE);
    const uint32_t ldb = (any16 || any8) ? mfma_ldb(dim) : 0;
    std::vector<float> q16(ldb ? ldb : 1, 0.0f);
    for (uint32_t c = 0; c < dim && c < ldb; ++c) q16[c] = (float)q[c];
    I8Query q8;
    if (any8) prepare_i8_query(q.data(), dim, &q8);
    Bf16Copy full16{}, part16{};
    I8Copy full8{}, part8{};
    if (any16) {
        for (Bf16Copy* c : {&full16, &part16}) {
            c->slab = dalloc<uint16_t>(n_alloc * ldb, 0x40);
            c->nrm = dalloc<float>(n_alloc, 0x40);
            c->sqn = dalloc<float>(n_alloc, 0x40);
        }
        CK(launch_rows_bf16(s, d_master, n, dim, full16.slab, full16.nrm, full16.sqn));
    }
    if (any8) {
        for (I8Copy* c : {&full8, &part8}) {
            c->slab = dalloc<uint8_t>(n_alloc * ldb, 0x40);
            c->sr = dalloc<float>(n_alloc * 2, 0x40);
            c->nrm = dalloc<float>(n_alloc, 0x40);
        }
        CK(launch_rows_i8(s, d_master, n, dim, full8.slab, full8.sr, full8.nrm));
    }
    CK(hipStreamSynchronize(s));

    unsigned long long* d_keep = dalloc<unsigned long long>(words);
    uint32_t* d_kept = dalloc<uint32_t>(n);
    Cand32* d_part = dalloc<Cand32>(PARTIALS32_ENTRIES);
    Cand32* d_m0 = dalloc<Cand32>((size_t)SCAN_MAX_GRID);
    Cand32* d_m1 = dalloc<Cand32>((size_t)SCAN_MAX_GRID);
    Cand32* d_list = dalloc<Cand32>(KP);
    Cand32* d_yard = dalloc<Cand32>(KP);

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) {
        printf("FAIL cannot open %s\n", argv[2]);
        return 2;
    }
    std::vector<uint32_t> kept;
    std::vector<double> crows;
    for (uint32_t k = 0; k < n_masks; ++k) {
        const unsigned long long* mask = masks.data() + (size_t)k * words;
        kept.clear();
        for (uint32_t p = 0; p < n32; ++p)
            if ((mask[p >> 6] >> (p & 63)) & 1ull) kept.push_back(p);
        const uint32_t m = (uint32_t)kept.size();
        CK(hipMemcpy(d_keep, mask, (size_t)words * 8, hipMemcpyHostToDevice));
        if (m) {
            CK(hipMemcpy(d_kept, kept.data(), (size_t)m * 4, hipMemcpyHostToDevice));
            crows.resize((size_t)m * dim);
            for (uint32_t i = 0; i < m; ++i) memcpy(crows.data() + (size_t)i * dim, rows.data() + (size_t)kept[i] * dim, (size_t)dim * 8);
            CK(hipMemcpy(d_cmaster, crows.data(), crows.size() * 8, hipMemcpyHostToDevice));
            if (any16) CK(launch_rows_bf16(s, d_cmaster, m, dim, part16.slab, part16.nrm, part16.sqn));
            if (any8) CK(launch_rows_i8(s, d_cmaster, m, dim, part8.slab, part8.sr, part8.nrm));
            CK(hipStreamSynchronize(s));
        }
        for (uint32_t mi = 0; mi < n_metrics; ++mi) {
            const int metric = (int)hdr[2 + mi];
            for (uint32_t stage = 0; stage < 3; ++stage) {
                const bool ran = stage == 0   ? (stages & 1) != 0
                                 : stage == 1 ? (stages & 2) && scan_bf16_supported(dim, metric)
                                              : (stages & 4) && scan_i8_supported(dim, metric);
                int variant = 0, grid = 0, ygrid = 0;
                if (ran) {
                    if (stage == 0) {
                        ScanPlan plan{}, lone{};
                        CK(launch_scan_masked(s, metric, d_slab, d_inv, d_keep, n, d_q, dim, ld, d_part, &plan, qarg ? q32.data() : nullptr));
                        merge_to_one(s, d_part, plan.grid, d_m0, d_m1, d_list);
                        CK(hipStreamSynchronize(s));
                        variant = plan.variant;
                        if (m) {
                            CK(launch_scan_subset(s, metric, d_slab, d_inv, d_kept, m, d_q, dim, ld, d_part, &lone, qarg ? q32.data() : nullptr));
                            merge_to_one(s, d_part, lone.grid, d_m0, d_m1, d_yard);
                        }
                    } else if (stage == 1) {
                        CK(launch_scan_bf16_masked(s, metric, full16.slab, full16.nrm, full16.sqn, d_keep, n, dim, d_part, &grid, q16.data(),
                                                   &variant));
                        merge_to_one(s, d_part, grid, d_m0, d_m1, d_list);
                        CK(hipStreamSynchronize(s));
                        if (m) {
                            CK(launch_scan_bf16(s, metric, part16.slab, part16.nrm, part16.sqn, nullptr, m, dim, d_part, &ygrid, q16.data()));
                            merge_to_one(s, d_part, ygrid, d_m0, d_m1, d_yard);
                        }
                    } else {
                        CK(launch_scan_i8_masked(s, metric, full8.slab, full8.sr, full8.nrm, d_keep, q8, n, dim, d_part, &grid, &variant));
                        merge_to_one(s, d_part, grid, d_m0, d_m1, d_list);
                        CK(hipStreamSynchronize(s));
                        if (m) {
                            CK(launch_scan_i8(s, metric, part8.slab, part8.sr, part8.nrm, q8, m, dim, d_part, &ygrid));
                            merge_to_one(s, d_part, ygrid, d_m0, d_m1, d_yard);
                        }
                    }
                    CK(hipStreamSynchronize(s));
                }
                const uint32_t oh[8] = {MAGIC, k, (uint32_t)metric, stage, ran ? 1u : 0u, (uint32_t)variant, m, (ran && m) ? 1u : 0u};
                wr(fo, oh, sizeof oh);
                if (ran) {
                    write_list(fo, d_list, nullptr, 0);
                    if (m) write_list(fo, d_yard, stage == 0 ? nullptr : kept.data(), m);
                }
            }
        }
    }
    {   // the resolution of an exclusion token over (pos_ids, id_set), as resolve_filter and ensure_plist launch it
        unsigned long long* d_pos_ids = dalloc<unsigned long long>(n);
        unsigned long long* d_set = dalloc<unsigned long long>(n_set ? n_set : 1);
        CK(hipMemcpy(d_pos_ids, pos_ids.data(), n * 8, hipMemcpyHostToDevice));
        if (n_set) CK(hipMemcpy(d_set, id_set.data(), (size_t)n_set * 8, hipMemcpyHostToDevice));
        uint32_t* d_counts = dalloc<uint32_t>((size_t)FILTER_COUNTS_MAX + 1);
        unsigned long long* d_bits = dalloc<unsigned long long>(words, 0xA5);  // a word the kernel skips keeps the pattern
        uint32_t* d_plist = dalloc<uint32_t>(n, 0xFF);
        CK(launch_filter_count(s, d_pos_ids, n, n_set ? d_set : nullptr, n_set, d_counts, d_counts + FILTER_COUNTS_MAX, true));
        uint32_t m = 0;
        CK(hipMemcpyAsync(&m, d_counts + FILTER_COUNTS_MAX, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        if (m > n32) {
            printf("FAIL the count found %u rows of %u\n", m, n32);
            return 3;
        }
        CK(launch_filter_bits(s, d_pos_ids, n, n_set ? d_set : nullptr, n_set, d_bits));
        if (m) CK(launch_filter_compact(s, d_pos_ids, n, n_set ? d_set : nullptr, n_set, d_counts, m, d_plist, true));
        CK(hipStreamSynchronize(s));
        std::vector<unsigned long long> h_bits(words);
        std::vector<uint32_t> h_plist(m);
        CK(hipMemcpy(h_bits.data(), d_bits, (size_t)words * 8, hipMemcpyDeviceToHost));
        if (m) CK(hipMemcpy(h_plist.data(), d_plist, (size_t)m * 4, hipMemcpyDeviceToHost));
        const uint32_t rh[2] = {MAGIC, m};
        wr(fo, rh, sizeof rh);
        wr(fo, h_bits.data(), (size_t)words * 8);
        wr(fo, h_plist.data(), (size_t)m * 4);
    }
    fclose(fo);
    printf("audit ok: %u masks, %u metrics\n", n_masks, n_metrics);
    return 0;
}
