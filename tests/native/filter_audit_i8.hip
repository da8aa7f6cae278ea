// Audit of the int8 single-query filter against its exactness bound (test tool, not shipped; driven by
// tests/test_gpu_filter_audit_i8.py).  Two modes:
//
//   filter_audit_i8 rows <n> <dim> <seed>
//     n rows generated on the host (i.i.d. normal, splitmix64 + Box-Muller), the first ADVERSARIAL_ROWS of them replaced by
//     edge cases; the library's launch_rows_i8 converts them on the device; the host then recomputes, in long double,
//     every row's true residual |x/|x| - s k| and checks r >= it, the byte range, the scale (max|x^| / s <= 127), the
//     padding, zero rows and the f32 row norm.  Prints one "rows ..." summary line and "audit ok" (status only: the
//     Python test reads the line).
//
//   filter_audit_i8 keys <case file> <output file>
//     As tests/native/filter_audit.hip for the int8 filter: the library's own stages on one case (ingest for R,
//     launch_rows_i8, prepare_i8_query, launch_scan_i8, the lists merged to one per query, the shipped bound_for_key with
//     IN_EXTRA_I8_SINGLE on the device, the exact f64 scan of every row).  Every check is made by the Python test.
//     case file: u32 magic 'VLA8', u32 n_metrics, u32 metrics[2], u32 n, u32 dim, u32 nq, f64 rows[n][dim], f64 queries[nq][dim]
//     output: u32 ldb, u8 bytes[n][ldb], f32 sr[n][2], f32 nrm[n]; then per metric: u32 magic, u32 metric, u32 nq, u32 n,
//     u32 ld, u32 grid, f64 R, f64 in_extra, f64 Q[nq], per query {f32 inv_scale, f32 qd, f32 d, u16 h[ldb]},
//     f32 key[nq][64], u32 pos[nq][64], f64 B_t64[nq], f64 B_key[nq][64], f64 exact[nq][n]
#include "../../vectorlite_amd/csrc/kernels.hip"
#include "../../vectorlite_amd/csrc/mfma_scan.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace vl;

namespace {

constexpr uint32_t MAGIC = 0x38414c56u;  // "VLA8"
constexpr int ADVERSARIAL_ROWS = 24;

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            printf("FAIL %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

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

void merge_to_one(hipStream_t s, const Cand32* lists, int n_lists, size_t stride, Cand32* buf0, Cand32* buf1, Cand32* out)
{
    Cand32* bufs[2] = {buf0, buf1};
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

// the int8 copy of n rows: bytes [n][ldb], (s, r) [n][2], |row| [n]
struct Copy {
    std::vector<uint8_t> bytes;
    std::vector<float> sr, nrm;
};

Copy convert(hipStream_t s, const double* d_master, uint64_t n, uint32_t dim)
{
    const uint32_t ldb = mfma_ldb(dim);
    // one spare row of 0x40 bytes past the end on every array: a conversion that overran would show in it
    uint8_t* d_b = dalloc<uint8_t>((n + 1) * ldb, 0x40);
    float* d_sr = dalloc<float>((n + 1) * 2, 0x40);
    float* d_nr = dalloc<float>(n + 1, 0x40);
    CK(launch_rows_i8(s, d_master, n, dim, d_b, d_sr, d_nr));
    CK(hipStreamSynchronize(s));
    Copy c;
    c.bytes.resize((n + 1) * ldb);
    c.sr.resize((n + 1) * 2);
    c.nrm.resize(n + 1);
    CK(hipMemcpy(c.bytes.data(), d_b, c.bytes.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(c.sr.data(), d_sr, c.sr.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(c.nrm.data(), d_nr, c.nrm.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(d_b));
    CK(hipFree(d_sr));
    CK(hipFree(d_nr));
    return c;
}

uint64_t splitmix(uint64_t& x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

double uniform01(uint64_t& x) { return ((double)(splitmix(x) >> 11) + 0.5) * 0x1.0p-53; }

double normal(uint64_t& x) { return std::sqrt(-2.0 * std::log(uniform01(x))) * std::cos(6.283185307179586 * uniform01(x)); }

// edge cases of the conversion, all inside the fast-path domain (|v| <= 2^40, norm 0 or >= 2^-40)
void adversarial(double* r, int which, uint32_t dim, uint64_t& rng)
{
    for (uint32_t c = 0; c < dim; ++c) r[c] = 0.0;
    const double t = 0x1.0p-20;
    switch (which) {
    case 0: break;                                                                 // zero row
    case 1: r[dim / 2] = 0x1.0p-40; break;                                         // one-hot at the smallest norm
    case 2: r[0] = -0x1.0p40; break;                                               // one-hot at the largest value
    case 3: for (uint32_t c = 0; c < dim; ++c) r[c] = 1.0; break;                  // all equal: k = 127 everywhere
    case 4: for (uint32_t c = 0; c < dim; ++c) r[c] = (c & 1) ? -0x1.0p40 : 0x1.0p40; break;
    case 5: for (uint32_t c = 0; c < dim; ++c) r[c] = 0x1.0p-40 / std::sqrt((double)dim) * 1.0001; break;
    case 6:  // x^ / s at (almost exactly) k + 1/2 in every column: the rounding's worst residual
        r[0] = 127.0 * t;
        for (uint32_t c = 1; c < dim; ++c) r[c] = ((double)(c % 127) + 0.5) * t * ((c & 2) ? -1.0 : 1.0);
        break;
    case 7:  // one huge value and f64 subnormals
        r[1] = 0x1.0p40;
        for (uint32_t c = 2; c < dim; ++c) r[c] = 4.9406564584124654e-324 * (double)(1 + (splitmix(rng) & 0xFFFFF));
        break;
    case 8:  // norm ~2^-40 spread thin, with f64 subnormals mixed in
        for (uint32_t c = 0; c < dim; ++c) r[c] = (c % 3 == 0) ? 1e-310 : 0x1.0p-39 / std::sqrt((double)dim);
        break;
    case 9:  // the largest entry negative, just above a power of two over 127
        for (uint32_t c = 0; c < dim; ++c) r[c] = normal(rng) * 0.01;
        r[dim - 1] = -1.0 - 0x1.0p-40;
        break;
    case 10:  // two equal maxima of opposite sign, the rest tiny
        r[0] = 1.0;
        r[dim - 1] = -1.0;
        for (uint32_t c = 1; c + 1 < dim; ++c) r[c] = 1e-9 * normal(rng);
        break;
    case 11:  // values on the int8 grid exactly: residual 0 in exact arithmetic
        for (uint32_t c = 0; c < dim; ++c) r[c] = (double)((int)(splitmix(rng) % 255) - 127) * 0x1.0p-7;
        r[0] = 127.0 * 0x1.0p-7;
        break;
    case 12:  // a max/127 that is not an f32: the scale is rounded up
        for (uint32_t c = 0; c < dim; ++c) r[c] = normal(rng);
        r[3] = 10.0 / 3.0;
        break;
    case 13:  // gaussian at 2^39
        for (uint32_t c = 0; c < dim; ++c) r[c] = normal(rng) * 0x1.0p39 / std::sqrt((double)dim);
        break;
    case 14:  // gaussian at 2^-39
        for (uint32_t c = 0; c < dim; ++c) r[c] = normal(rng) * 0x1.0p-39;
        break;
    case 15:  // every column just below the rounding boundary k + 1/2 from above and below alternately
        r[0] = 127.0;
        for (uint32_t c = 1; c < dim; ++c) r[c] = (double)(c % 100) + ((c & 1) ? 0.5 - 0x1.0p-30 : 0.5 + 0x1.0p-30);
        break;
    default:  // sparse rows: a few columns of mixed magnitude
        for (int j = 0; j < 1 + which % 5; ++j)
            r[splitmix(rng) % dim] = normal(rng) * std::ldexp(1.0, (int)(splitmix(rng) % 60) - 30);
        if (which % 7 == 0) r[0] = 0x1.0p40;
        break;
    }
}

int rows_mode(uint64_t n, uint32_t dim, uint64_t seed)
{
    const uint32_t ldb = mfma_ldb(dim);
    std::vector<double> rows(n * dim);
    uint64_t rng = seed * 0x2545F4914F6CDD1Dull + 1;
    for (uint64_t i = 0; i < n * dim; ++i) rows[i] = normal(rng);
    for (int a = 0; a < ADVERSARIAL_ROWS && (uint64_t)a < n; ++a) adversarial(&rows[(size_t)a * dim], a, dim, rng);
    hipStream_t s;
    CK(hipStreamCreate(&s));
    double* d_master = dalloc<double>(n * dim);
    CK(hipMemcpy(d_master, rows.data(), n * dim * 8, hipMemcpyHostToDevice));
    const Copy c = convert(s, d_master, n, dim);

    uint64_t bad_r = 0, bad_byte = 0, bad_scale = 0, bad_pad = 0, bad_zero = 0, bad_norm = 0, bad_tail = 0;
    long double worst_ratio = 0.0L, min_margin = 1e30L, worst_adv_ratio = 0.0L;
    long double sum_r = 0.0L, max_r = 0.0L, max_true = 0.0L;
    for (uint64_t i = 0; i < n; ++i) {
        const double* x = &rows[i * dim];
        const uint8_t* b = &c.bytes[i * ldb];
        const float s_ = c.sr[2 * i], r_ = c.sr[2 * i + 1];
        long double ss = 0.0L, mx = 0.0L;
        for (uint32_t k = 0; k < dim; ++k) ss += (long double)x[k] * (long double)x[k];
        const long double nrm = sqrtl(ss);
        for (uint32_t k = dim; k < ldb; ++k) bad_pad += b[k] != 128;
        if (nrm == 0.0L) {
            bool z = s_ == 0.0f && r_ == 0.0f && c.nrm[i] == 0.0f;
            for (uint32_t k = 0; k < dim; ++k) z = z && b[k] == 128;
            bad_zero += !z;
            continue;
        }
        long double res = 0.0L;
        for (uint32_t k = 0; k < dim; ++k) {
            const long double xh = (long double)x[k] / nrm;
            mx = fmaxl(mx, fabsl(xh));
            bad_byte += b[k] == 0;  // k = -128 is never written
            const long double d = xh - (long double)s_ * (long double)((int)b[k] - 128);
            res += d * d;
        }
        const long double true_r = sqrtl(res);
        if (!((long double)r_ >= true_r)) ++bad_r;
        if (!(mx / (long double)s_ <= 127.0L)) ++bad_scale;
        // |row| rounded once to f32: within half an f32 ulp (2^-24 relative) of the exact norm, plus the f64 norm's error
        if (!(fabsl((long double)c.nrm[i] - nrm) <= nrm * (0x1.0p-24L + (long double)(dim + 8) * 0x1.0p-53L))) ++bad_norm;
        const long double ratio = r_ > 0.0f ? true_r / (long double)r_ : (true_r > 0.0L ? 1e30L : 0.0L);
        worst_ratio = fmaxl(worst_ratio, ratio);
        if (i < (uint64_t)ADVERSARIAL_ROWS) worst_adv_ratio = fmaxl(worst_adv_ratio, ratio);
        min_margin = fminl(min_margin, (long double)r_ - true_r);
        sum_r += r_;
        max_r = fmaxl(max_r, (long double)r_);
        max_true = fmaxl(max_true, true_r);
    }
    for (uint32_t k = 0; k < ldb; ++k) bad_tail += c.bytes[n * ldb + k] != 0x40;
    // the spare row's floats keep their fill, 0x40404040 = 3.0039...
    bad_tail += c.sr[2 * n] != 3.00392150878906250f || c.sr[2 * n + 1] != 3.00392150878906250f || c.nrm[n] != 3.00392150878906250f;
    printf("rows n=%llu dim=%u ldb=%u bad_r=%llu bad_byte=%llu bad_scale=%llu bad_pad=%llu bad_zero=%llu bad_norm=%llu "
           "bad_tail=%llu worst_ratio=%.15Lg worst_adversarial_ratio=%.15Lg min_margin=%.6Lg mean_r=%.6Lg max_r=%.6Lg "
           "max_true_residual=%.6Lg r_bound=%.6g\n",
           (unsigned long long)n, dim, ldb, (unsigned long long)bad_r, (unsigned long long)bad_byte,
           (unsigned long long)bad_scale, (unsigned long long)bad_pad, (unsigned long long)bad_zero,
           (unsigned long long)bad_norm, (unsigned long long)bad_tail, worst_ratio, worst_adv_ratio, min_margin,
           sum_r / (long double)n, max_r, max_true, std::sqrt((double)ldb) / 254.0);
    CK(hipFree(d_master));
    printf("audit ok\n");
    return 0;
}

int keys_mode(const char* case_path, const char* out_path)
{
    FILE* fi = fopen(case_path, "rb");
    if (!fi) {
        printf("FAIL cannot open %s\n", case_path);
        return 2;
    }
    uint32_t hdr[7];
    if (fread(hdr, 4, 7, fi) != 7 || hdr[0] != MAGIC) {
        printf("FAIL bad case header\n");
        return 2;
    }
    const uint32_t n_metrics = hdr[1], n32 = hdr[4], dim = hdr[5], nq = hdr[6];
    const uint64_t n = n32;
    if (n_metrics < 1 || n_metrics > 2 || n == 0 || dim == 0 || nq == 0 || nq > 64) {
        printf("FAIL bad case parameters\n");
        return 2;
    }
    std::vector<double> rows(n * dim), qs((size_t)nq * dim + nq);
    if (fread(rows.data(), 8, rows.size(), fi) != rows.size() || fread(qs.data(), 8, (size_t)nq * dim, fi) != (size_t)nq * dim) {
        printf("FAIL short case file\n");
        return 2;
    }
    fclose(fi);
    for (uint32_t q = 0; q < nq; ++q) {  // sequential sum of squares, as the host stages a single query
        double ss = 0.0;
        for (uint32_t c = 0; c < dim; ++c) ss += qs[(size_t)q * dim + c] * qs[(size_t)q * dim + c];
        qs[(size_t)nq * dim + q] = sqrt(ss);
    }
    const uint32_t ld = (dim + 3u) & ~3u;  // the n of every bound (rank_check_emit)
    const uint32_t ldb = mfma_ldb(dim);
    hipStream_t s;
    CK(hipStreamCreate(&s));
    double* d_master = dalloc<double>(n * dim);
    CK(hipMemcpy(d_master, rows.data(), n * dim * 8, hipMemcpyHostToDevice));
    double* d_q = dalloc<double>(qs.size());
    CK(hipMemcpy(d_q, qs.data(), qs.size() * 8, hipMemcpyHostToDevice));
    const double* d_qn = d_q + (size_t)nq * dim;
    // R: the ingest's max row norm, as the library has it
    float* d_slab = dalloc<float>(n * ld);
    float* d_inv = dalloc<float>(n);
    uint8_t* d_flags = dalloc<uint8_t>(n);
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

    // the int8 copy the scan reads: converted by the library, then uploaded again exactly as written
    const Copy c = convert(s, d_master, n, dim);
    uint8_t* d_b = dalloc<uint8_t>(n * ldb);
    float* d_sr = dalloc<float>(n * 2);
    float* d_nr = dalloc<float>(n);
    CK(hipMemcpy(d_b, c.bytes.data(), n * ldb, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_sr, c.sr.data(), n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_nr, c.nrm.data(), n * 4, hipMemcpyHostToDevice));

    Cand32* d_part = dalloc<Cand32>(PARTIALS32_ENTRIES);
    Cand32* d_m0 = dalloc<Cand32>((size_t)SCAN_MAX_GRID);
    Cand32* d_m1 = dalloc<Cand32>((size_t)SCAN_MAX_GRID);
    Cand32* d_lists = dalloc<Cand32>((size_t)nq * KP);
    double* d_bt = dalloc<double>(nq);
    double* d_bk = dalloc<double>((size_t)nq * KP);
    double* d_exact = dalloc<double>(n * nq);
    uint32_t* d_nan = dalloc<uint32_t>(1);

    FILE* fo = fopen(out_path, "wb");
    if (!fo) {
        printf("FAIL cannot open %s\n", out_path);
        return 2;
    }
    wr(fo, &ldb, 4);
    wr(fo, c.bytes.data(), n * ldb);
    wr(fo, c.sr.data(), n * 8);
    wr(fo, c.nrm.data(), n * 4);
    std::vector<I8Query> prep(nq);
    for (uint32_t q = 0; q < nq; ++q) prepare_i8_query(qs.data() + (size_t)q * dim, dim, &prep[q]);
    for (uint32_t mi = 0; mi < n_metrics; ++mi) {
        const int metric = (int)hdr[2 + mi];
        if (!scan_i8_supported(dim, metric)) {
            printf("FAIL no int8 scan for dim %u metric %d\n", dim, metric);
            return 2;
        }
        const double in_extra = IN_EXTRA_I8_SINGLE;
        int grid = 0;
        for (uint32_t q = 0; q < nq; ++q) {
            CK(launch_scan_i8(s, metric, d_b, d_sr, d_nr, prep[q], n, dim, d_part, &grid));
            merge_to_one(s, d_part, grid, (size_t)grid * KP, d_m0, d_m1, d_lists + (size_t)q * KP);
            CK(hipStreamSynchronize(s));
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
        const uint32_t oh[6] = {MAGIC, (uint32_t)metric, nq, n32, ld, (uint32_t)grid};
        wr(fo, oh, sizeof oh);
        wr(fo, &R, 8);
        wr(fo, &in_extra, 8);
        wr(fo, qs.data() + (size_t)nq * dim, (size_t)nq * 8);
        for (uint32_t q = 0; q < nq; ++q) {
            const float f3[3] = {prep[q].inv_scale, prep[q].qd, prep[q].d};
            wr(fo, f3, 12);
            wr(fo, prep[q].h, (size_t)ldb * 2);
        }
        wr(fo, keys.data(), keys.size() * 4);
        wr(fo, pos.data(), pos.size() * 4);
        wr(fo, bt.data(), bt.size() * 8);
        wr(fo, bk.data(), bk.size() * 8);
        wr(fo, exact.data(), exact.size() * 8);
        printf("metric %d: %u queries, grid %d\n", metric, nq, grid);
    }
    fclose(fo);
    printf("audit ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 5 && strcmp(argv[1], "rows") == 0) {
        const uint64_t n = strtoull(argv[2], nullptr, 10);
        const uint32_t dim = (uint32_t)strtoul(argv[3], nullptr, 10);
        if (n == 0 || n > 4000000 || dim == 0 || dim > (uint32_t)SCAN8_QARG_HALVES) {
            printf("FAIL bad rows parameters\n");
            return 2;
        }
        return rows_mode(n, dim, strtoull(argv[4], nullptr, 10));
    }
    if (argc == 4 && strcmp(argv[1], "keys") == 0) return keys_mode(argv[2], argv[3]);
    printf("usage: filter_audit_i8 rows <n> <dim> <seed> | keys <case> <out>\n");
    return 2;
}
